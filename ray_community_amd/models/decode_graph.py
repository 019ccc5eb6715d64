"""The decode step as a replayable HIP graph: ``DecodeRunner``.

``Llama.decode_step`` builds five small device tensors from Python lists and then makes about ten
launches per layer, each a Python call; at decode sizes the step is bound by that, not by the
kernels. The runner keeps everything that changes per step in static device buffers (tokens,
context lengths, block table), fills them with one copy from a pinned staging buffer, and runs a
body that reads nothing else: ``ops.rope_kv_append_decode_`` derives position and slot on the
device, so neither a positions nor a slots tensor exists. The body is captured once per block-table
width with ``torch.cuda.graph`` and replayed; what the kernels compute is what the uncaptured body
computes, bit for bit.

Widths are bucketed: ``W`` is the smallest power of two holding the batch's longest block list,
at least 16 blocks and at most ``ceil(max_seq_len / page)``. ``ops.paged_attention_decode`` picks its
split count from the table's width, so a bucket keeps that count near what the real context lengths
ask for; the kernel never reads a table entry past a sequence's length, so the padding is free. One
graph per ``W``, all in one memory pool.

The first step at a width runs the body eagerly on a side stream (the library load, the hipBLASLt
handles and workspaces and the RoPE table must exist before a capture; it is a real step), the
second captures and replays. The captured region is one stream, a linear chain of kernels.

A round the graph cannot serve runs ``Llama.decode_step`` and is counted in ``stats``: one in which
a row names a LoRA adapter (the routing is built on the host per call). ``stats`` is ``{"graphs",
"replays", "eager_warm", "eager_fallback"}``.

A captured graph holds the addresses of the modules' tensors. ``Llama.module_epoch`` changes when a
module is swapped (``quantize_weights_``, ``enable_lora_``) or the parameters move; the runner then
drops its graphs. In-place updates (``load_state_dict``) keep their addresses and need nothing.
"""
from __future__ import annotations

import torch

from .. import ops

MIN_WIDTH = 16  # blocks: the smallest block-table bucket


def new_stats():
    return {"graphs": 0, "replays": 0, "eager_warm": 0, "eager_fallback": 0}


class DecodeRunner:
    """``runner.step(tokens, seq_ids)`` is ``model.decode_step(tokens, cache, seq_ids)`` for a fixed
    batch size over static buffers. ``capture=False``, or a model that is not on a GPU, runs the
    same body uncaptured. The returned logits ``[batch, V]`` are the runner's static output: the
    next step overwrites them."""

    def __init__(self, model, cache, batch: int, *, capture: bool = True):
        if int(batch) < 1:
            raise ValueError("batch must be >= 1")
        self.model, self.cache, self.batch = model, cache, int(batch)
        w = model.embed.weight
        self.device = w.device
        self.capture = bool(capture) and w.is_cuda
        self.stats = new_stats()
        cfg, page, B = model.cfg, cache.page_size, self.batch
        self.max_width = -(-cfg.max_seq_len // page)
        # one int32 buffer: tokens (as int64) | context_lens | block_table (the widest bucket; a
        # narrower one is a [B, W] view of the same words), so a step's inputs go up in one copy
        self._table_at = 3 * B
        words = self._table_at + B * self.max_width
        self._dev = torch.zeros(words, dtype=torch.int32, device=self.device)
        self._host = torch.zeros(words, dtype=torch.int32, pin_memory=w.is_cuda)
        self.tokens = self._dev[: 2 * B].view(torch.int64)
        self.context_lens = self._dev[2 * B: 3 * B]
        self._np = self._host.numpy()
        self._tokens_h = self._np[: 2 * B].view("int64")
        self._lens_h = self._np[2 * B: 3 * B]
        self.logits = torch.zeros(B, cfg.vocab_size, dtype=w.dtype, device=self.device)
        self._uploaded = torch.cuda.Event() if w.is_cuda else None
        self._pool = None
        self._graphs, self._warm = {}, set()
        self._epoch = model.module_epoch

    # ---------------------------------------------------------------------------------- buffers
    def block_table(self, width: int):
        """The static ``[batch, width]`` block table of a bucket."""
        return self._dev[self._table_at: self._table_at + self.batch * width].view(self.batch, width)

    def width_for(self, blocks: int) -> int:
        """The bucket of a batch whose longest block list has ``blocks`` entries."""
        w = MIN_WIDTH
        while w < blocks:
            w *= 2
        return max(1, min(w, self.max_width))

    def widths(self):
        """Every bucket, narrowest first."""
        out, w = [], self.width_for(1)
        while w not in out:
            out.append(w)
            w = self.width_for(w + 1)
        return out

    def _upload(self, width, tokens, seq_ids):
        B = self.batch
        if self._uploaded is not None:
            self._uploaded.synchronize()  # the last copy out of the staging buffer is over
        table = self._np[self._table_at: self._table_at + B * width].reshape(B, width)
        self.cache.fill_decode_inputs(seq_ids, self._lens_h, table)
        on_device = torch.is_tensor(tokens) and tokens.device.type != "cpu"
        if not on_device:
            self._tokens_h[:] = tokens.tolist() if torch.is_tensor(tokens) else [int(t) for t in tokens]
        n = self._table_at + B * width
        self._dev[:n].copy_(self._host[:n], non_blocking=True)
        if self._uploaded is not None:
            self._uploaded.record()
        if on_device:
            self.tokens.copy_(tokens.reshape(-1))

    # ------------------------------------------------------------------------------------- body
    def _body(self, width):
        """Embedding, the layers and the logits, reading the static buffers only."""
        model, cache = self.model, self.cache
        cfg = model.cfg
        D, Hq, Hk = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
        cs = model.rope_table(self.device)
        table, lens = self.block_table(width), self.context_lens

        def attn(i, blk, h):
            ks, vs = cache.scales(i)
            qkv = ops.rope_kv_append_decode_(blk.attn.qkv(h), cs, cache.k[i], cache.v[i], table, lens, Hq, Hk, D,
                                             k_scale=ks, v_scale=vs)
            return blk.attn.o(ops.paged_attention_decode(qkv, cache.k[i], cache.v[i], table, lens, Hq, Hk, D,
                                                         k_scale=ks, v_scale=vs))

        self.logits.copy_(model.logits(model._run_layers(model.embed(self.tokens), attn)))

    def _run(self, width, replay=True):
        if not self.capture:
            self._body(width)
            return
        graph = self._graphs.get(width)
        if graph is None and width not in self._warm:
            cur = torch.cuda.current_stream(self.device)
            side = torch.cuda.Stream(self.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._body(width)
            cur.wait_stream(side)
            self._warm.add(width)
            self.stats["eager_warm"] += 1
            return
        if graph is None:
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=self._pool):
                self._body(width)
            self._graphs[width] = graph
            self.stats["graphs"] += 1
        if replay:  # a capture records the step without running it
            graph.replay()
            self.stats["replays"] += 1

    def _check_epoch(self):
        if self._epoch != self.model.module_epoch:
            self._graphs.clear()
            self._warm.clear()
            self._epoch = self.model.module_epoch

    # ----------------------------------------------------------------------------------- public
    @torch.inference_mode()
    def step(self, tokens, seq_ids, *, adapters=None):
        """One new token per sequence, as ``Llama.decode_step``: the ``max_seq_len`` check, all or
        nothing allocation (``KVCacheFull`` leaves the cache as it was), then the body. With an
        adapter named in ``adapters`` the round runs ``decode_step`` itself."""
        model, cache, B = self.model, self.cache, self.batch
        if len(tokens) != B or len(seq_ids) != B or (adapters is not None and len(adapters) != B):
            raise ValueError(f"tokens, seq_ids and adapters must have the runner's batch size {B}")
        if adapters is not None and any(a is not None for a in adapters):
            self.stats["eager_fallback"] += 1
            return model.decode_step(tokens, cache, seq_ids, adapters=adapters)
        self._check_epoch()
        if max(cache.length(s) if s is not None else 0 for s in seq_ids) >= model.cfg.max_seq_len:
            raise ValueError(f"sequence would exceed max_seq_len {model.cfg.max_seq_len}")
        model._allocate(cache, [(s, 1) for s in seq_ids])
        width = self.width_for(max(cache.blocks_held(s) if s is not None else 0 for s in seq_ids))
        self._upload(width, tokens, seq_ids)
        self._run(width)
        return self.logits

    def count_fallback(self):
        """A round that went around the runner (a speculative verify round through ``extend``)."""
        self.stats["eager_fallback"] += 1

    @torch.inference_mode()
    def warmup(self):
        """Capture every bucket now, for servers that want no capture latency in flight. Runs the
        body with every row inactive (context length 0), which writes nothing to the cache."""
        self._check_epoch()
        if not self.capture:
            return self
        self._dev.zero_()
        for width in self.widths():
            if width not in self._graphs:
                if width not in self._warm:
                    self._run(width)
                self._run(width, replay=False)
        torch.cuda.current_stream(self.device).synchronize()
        return self


def runner_for(model, cache, batch: int, *, capture: bool = True) -> DecodeRunner:
    """The runner of ``(model, cache, batch)``, kept with the cache so that callers that come back
    with the same cache (``Llama.generate(cache=...)``) reuse its graphs."""
    runners = cache.__dict__.setdefault("_decode_runners", {})
    key = (id(model), int(batch), bool(capture))
    runner = runners.get(key)
    if runner is None or runner.model is not model:
        runner = runners[key] = DecodeRunner(model, cache, batch, capture=capture)
    return runner
