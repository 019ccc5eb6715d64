"""Llama-3 decoder (the model behind the Ray Train Llama-3-8B DDP headline benchmark).

MI355X-first layout choices:
  * fused QKV projection ([T, (Hq + 2*Hkv) * D]) with RoPE applied IN PLACE on its q/k heads
    by one HIP kernel (no q/k copies);
  * fused gate|up projection feeding the HIP SwiGLU kernel;
  * residual add fused into the following RMSNorm (HIP kernel emits both the new residual
    stream and the normalised activations; its backward adds the residual gradient);
  * HIP cross-entropy writing dlogits in place over the 128k-vocab logits, or (``fused_ce``)
    lm_head + CE fused chunk by chunk so the T x 128k logits are never materialised;
  * activations kept resident (no recomputation) — 288 GB HBM holds a full 8B replica with
    fp32 master weights + AdamW states + seq-4096 activations per GPU.
Attention is the framework's own MFMA flash-attention HIP kernels (``ops.attention``: causal,
GQA, XCD-grouped workgroup order); GEMMs are hipBLASLt via torch.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..parallel.fused_linear import FusedEmbedding, FusedWgradLinear, swiglu_down
from . import lora as _lora
from .quant import QuantLinear, quantize_weights_


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    max_seq_len: int = 8192
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    tie_embeddings: bool = False
    init_std: float = 0.02
    name: str = "llama"
    attn_impl: str = "hip"  # "hip" (gfx950 flash attention kernels) | "sdpa" (torch SDPA / aotriton)
    fused_ce: bool = False  # chunked lm_head + one-pass HIP CE (parallel/fused_linear.py): no T x V logits
    ce_chunk: int = 0       # tokens per fused-CE chunk (0: <= 1 GiB of logits per chunk)

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    def num_params(self) -> int:
        H, I, V, L = self.hidden_size, self.intermediate_size, self.vocab_size, self.num_layers
        kv = self.num_kv_heads * self.head_dim
        per_layer = H * (H + 2 * kv) + H * H + 2 * H * I + I * H + 2 * H
        emb = V * H * (1 if self.tie_embeddings else 2)
        return L * per_layer + emb + H

    def flops_per_token(self, seq_len: int) -> float:
        """Training FLOPs/token: 6 * matmul params + causal attention (fwd+bwd)."""
        H, L = self.hidden_size, self.num_layers
        n_matmul = self.num_params() - self.vocab_size * H * (0 if self.tie_embeddings else 1) - (2 * L + 1) * H
        attn = 6 * L * H * seq_len  # 12*L*H*S/2 (causal): QK^T + PV, fwd + 2x bwd
        return 6 * n_matmul + attn


PRESETS = {
    "llama3-8b": LlamaConfig(name="llama3-8b"),
    "llama3-70b": LlamaConfig(hidden_size=8192, intermediate_size=28672, num_layers=80, num_heads=64, num_kv_heads=8,
                              name="llama3-70b"),
    "llama3-1b": LlamaConfig(hidden_size=2048, intermediate_size=8192, num_layers=16, num_heads=32, num_kv_heads=8,
                             tie_embeddings=True, name="llama3-1b"),
    "llama3-tiny": LlamaConfig(vocab_size=1024, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4,
                               num_kv_heads=2, max_seq_len=256, name="llama3-tiny"),
}


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x, residual=None):
        return ops.rms_norm(x, self.weight, self.eps, residual)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        D = cfg.head_dim
        self.qkv = FusedWgradLinear(cfg.hidden_size, (cfg.num_heads + 2 * cfg.num_kv_heads) * D)
        self.o = FusedWgradLinear(cfg.num_heads * D, cfg.hidden_size)

    def forward(self, x, cs, B, S, positions=None):
        cfg = self.cfg
        D, Hq, Hk = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
        qkv = self.qkv(x)  # [T, (Hq+2Hk)*D]
        qkv = ops.apply_rope_(qkv, cs, S, Hq, Hk, D, positions)
        return self.causal_attention(qkv, B, S)

    def causal_attention(self, qkv, B, S):
        """Causal self-attention + output projection on the rotated fused ``qkv`` [B*S, W]."""
        cfg = self.cfg
        D, Hq, Hk = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
        T = B * S
        if qkv.is_cuda and cfg.attn_impl == "hip" and ops.flash_attention_supported(S, D, Hq, Hk):
            # gfx950 flash attention straight off the fused projection; backward fills dqkv directly
            return self.o(ops.flash_attention_qkv(qkv, B, S, Hq, Hk, D, causal=True))
        q = qkv[:, : Hq * D].view(B, S, Hq, D).transpose(1, 2)
        k = qkv[:, Hq * D: (Hq + Hk) * D].view(B, S, Hk, D).transpose(1, 2)
        v = qkv[:, (Hq + Hk) * D:].view(B, S, Hk, D).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=(Hk != Hq))
        o = o.transpose(1, 2).reshape(T, Hq * D)
        return self.o(o)


class MLP(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.gate_up = FusedWgradLinear(cfg.hidden_size, 2 * cfg.intermediate_size)
        self.down = FusedWgradLinear(cfg.intermediate_size, cfg.hidden_size)

    def forward(self, x):
        # On the flat-gradient GPU path SwiGLU also writes act^T (the down projection's wgrad
        # operand), and the backward's down dgrad GEMM applies the SwiGLU backward in its epilogue,
        # writing d(gate|up) and its transpose for the gate_up wgrad (parallel/fused_linear.py).
        if isinstance(self.down, (QuantLinear, _lora.LoraLinear)):  # fp8 weights / LoRA (inference only): the two separate ops
            return self.down(ops.swiglu(self.gate_up(x)))
        return swiglu_down(self.gate_up(x), self.down)


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.attn_norm = RMSNorm(cfg.hidden_size, cfg.norm_eps)
        self.attn = Attention(cfg)
        self.mlp_norm = RMSNorm(cfg.hidden_size, cfg.norm_eps)
        self.mlp = MLP(cfg)


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        # untied: the lookup's gradient goes straight into the flat buffer; tied, the weight also
        # gets the lm-head gradient, so both must meet in autograd's single accumulation
        self.embed = (nn.Embedding if cfg.tie_embeddings else FusedEmbedding)(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList([Block(cfg) for _ in range(cfg.num_layers)])
        self.norm = RMSNorm(cfg.hidden_size, cfg.norm_eps)
        self.lm_head = None if cfg.tie_embeddings else FusedWgradLinear(cfg.hidden_size, cfg.vocab_size)
        self._cs = {}
        # bumped by whatever replaces a module or moves the parameters: a captured decode graph
        # (models/decode_graph.py) holds their addresses and is dropped when this changes
        self.module_epoch = 0
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self):
        std = self.cfg.init_std
        out_std = std / math.sqrt(2 * self.cfg.num_layers)
        for name, p in self.named_parameters():
            if p.dim() == 1:
                p.fill_(1.0)
            elif name.endswith("o.weight") or name.endswith("down.weight"):
                p.normal_(0.0, out_std)
            else:
                p.normal_(0.0, std)

    def quantize_weights_(self, dtype="fp8"):
        """Quantise the linears' weights in place for inference (``models/quant.py``): ``"fp8"``
        halves their bytes; ``prefill`` / ``extend`` / ``decode_step`` / ``generate`` then run
        ``ops.linear_w8``. Idempotent. Training paths are not available afterwards."""
        self.module_epoch += 1
        return quantize_weights_(self, dtype)

    def enable_lora_(self, max_adapters: int, max_rank: int):
        """Make room for ``max_adapters`` LoRA adapters of up to ``max_rank`` per projection
        (``models/lora.py``): ``qkv``, ``o``, ``gate_up`` and ``down`` of every block become
        ``LoraLinear``s around their base modules (before or after ``quantize_weights_``), and
        ``prefill`` / ``extend`` / ``decode_step`` / ``generate`` take ``adapters=``. With no adapter
        named every logit keeps its bits. Training paths are not available afterwards."""
        self.module_epoch += 1
        return _lora.enable_lora_(self, max_adapters, max_rank)

    def _apply(self, fn, recurse=True):
        self.module_epoch += 1  # ``.to(device)`` and its kin give the parameters new storage
        return super()._apply(fn, recurse)

    def load_adapter(self, name, adapter):
        """Copy a ``LoraAdapter`` into a free slot under ``name``. ``AdapterSlotsFull`` when there is
        none; ``ValueError`` on a rank above ``max_rank``, a shape mismatch or a duplicate name."""
        return _lora.load_adapter(self, name, adapter)

    def unload_adapter(self, name):
        return _lora.unload_adapter(self, name)

    def loaded_adapters(self):
        """Names of the loaded adapters (empty without ``enable_lora_``)."""
        bank = getattr(self, "lora", None)
        return sorted(bank.slots, key=bank.slots.get) if bank is not None else []

    def rope_table(self, device):
        key = str(device)
        t = self._cs.get(key)
        if t is None:
            t = ops.rope_cos_sin(self.cfg.max_seq_len, self.cfg.head_dim, self.cfg.rope_theta).to(device)
            self._cs[key] = t
        return t

    def _run_layers(self, residual, attn):
        """The layer stack on the embedded tokens ``[T, H]`` with ``attn(i, blk, h)`` as the
        attention; returns the final-normed hidden states ``[T, H]``."""
        h = self.layers[0].attn_norm(residual) if len(self.layers) else residual
        for i, blk in enumerate(self.layers):
            a = attn(i, blk, h)
            h, residual = blk.mlp_norm(a, residual=residual)
            m = blk.mlp(h)
            nxt = self.layers[i + 1].attn_norm if i + 1 < len(self.layers) else self.norm
            h, residual = nxt(m, residual=residual)
        if not len(self.layers):
            h = self.norm(residual)
        return h

    def hidden_states(self, tokens, positions=None):
        B, S = tokens.shape
        cs = self.rope_table(tokens.device)
        return self._run_layers(self.embed(tokens).view(B * S, -1), lambda i, blk, h: blk.attn(h, cs, B, S, positions))

    def logits(self, h):
        if self.lm_head is not None:
            return self.lm_head(h)
        return F.linear(h, self.embed.weight)

    def forward(self, tokens, labels=None, positions=None):
        h = self.hidden_states(tokens, positions)
        if labels is not None and self.cfg.fused_ce and h.is_cuda:
            if self.lm_head is not None:  # through the module call so wrapper hooks still fire
                return self.lm_head(h, labels=labels.reshape(-1), ce_chunk=self.cfg.ce_chunk)
            from ..parallel.fused_linear import linear_cross_entropy

            return linear_cross_entropy(h, self.embed.weight, labels.reshape(-1), chunk_tokens=self.cfg.ce_chunk)
        logits = self.logits(h)
        if labels is None:
            return logits.view(*tokens.shape, -1)
        return ops.cross_entropy(logits, labels.reshape(-1), inplace_backward=True)

    # ------------------------------------------------------------------------------ inference
    # Generation over a paged KV cache (models/kv_cache.py). Under inference mode the fused-wgrad
    # linears and the fused embedding are plain ``F.linear`` / ``F.embedding`` (their autograd
    # paths are taken only when gradients are enabled), so the training modules are used as is.
    @staticmethod
    def _allocate(cache, pairs):
        """Cache slots for a batch of ``(seq_id, n_tokens)`` pairs, one list per pair. A ``None``
        id is an inactive slot of a fixed-size batch: it takes nothing and gets slot -1. All or
        nothing: a failed call (``KVCacheFull``) leaves the cache as it was."""
        slots, done = [], []
        try:
            for s, n in pairs:
                slots.append(cache.allocate(s, n) if s is not None else [-1] * n)
                done.append((s, n))
        except Exception:
            for s, n in reversed(done):
                if s is not None:
                    cache.rollback(s, n)
            raise
        return slots

    def _cached_forward(self, tokens, cache, slots, rope, attend, rows=None, adapters=None):
        """The body of a forward over ``cache``: embed the flat ``tokens`` ``[T]``, run the layers
        and return the logits of ``rows`` (indices into ``T``; ``None``: every row). Each layer
        rotates its fused qkv with ``rope = (seq_len, positions)`` (``ops.apply_rope_``), appends
        K/V at ``slots`` ``[T]`` and takes ``attend(i, blk, qkv)`` (which may read q in place from
        the fused rows) as the projected attention output ``[T, H]``. ``adapters``: a LoRA adapter
        name or ``None`` per row of ``tokens``, routed for the duration of the call."""
        cfg = self.cfg
        D, Hq, Hk = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
        cs = self.rope_table(tokens.device)
        seq_len, positions = rope

        def attn(i, blk, h):
            qkv = ops.apply_rope_(blk.attn.qkv(h), cs, seq_len, Hq, Hk, D, positions)
            ks, vs = cache.scales(i)
            ops.kv_cache_append_(cache.k[i], cache.v[i], qkv, slots, Hq, Hk, D, k_scale=ks, v_scale=vs)
            return attend(i, blk, qkv)

        with _lora.route(self, adapters, tokens.device):
            h = self._run_layers(self.embed(tokens), attn)
        return self.logits(h if rows is None else h[rows])

    @torch.inference_mode()
    def prefill(self, tokens, lengths, cache, seq_ids, *, adapters=None):
        """Run the prompts through the model, fill ``cache`` and return the logits ``[B, V]`` of
        each sequence's last real token.

        ``tokens``: ``[B, S]`` right-padded token ids (or a list of token lists, then ``lengths``
        may be ``None``); ``lengths``: real length per row. The batch is right-padded to a
        multiple of 128 and run through the ordinary causal forward (right padding cannot reach a
        real token through a causal mask); padded tokens get slot -1, i.e. are not cached.
        ``adapters``: a loaded LoRA adapter's name or ``None`` per sequence (``enable_lora_``)."""
        cfg = self.cfg
        dev = self.embed.weight.device
        if not torch.is_tensor(tokens):
            rows = [list(r) for r in tokens]
            lengths = [len(r) for r in rows] if lengths is None else lengths
            width = max(len(r) for r in rows)
            tokens = torch.tensor([r + [0] * (width - len(r)) for r in rows], dtype=torch.long)
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        B = tokens.shape[0]
        if len(lengths) != B or len(seq_ids) != B or (adapters is not None and len(adapters) != B):
            raise ValueError("tokens, lengths, seq_ids and adapters must agree on the batch size")
        if min(lengths) < 1 or max(lengths) > tokens.shape[1]:
            raise ValueError("every prompt needs between 1 and tokens.shape[1] tokens")
        S = -(-max(lengths) // 128) * 128
        if S > cfg.max_seq_len:
            raise ValueError(f"prompt of {max(lengths)} tokens pads to {S} > max_seq_len {cfg.max_seq_len}")
        padded = torch.zeros(B, S, dtype=torch.long, device=dev)
        keep = min(S, tokens.shape[1])
        padded[:, :keep] = tokens[:, :keep].to(dev)
        slots = torch.full((B, S), -1, dtype=torch.int32)
        for b, s in enumerate(self._allocate(cache, zip(seq_ids, lengths))):
            slots[b, :len(s)] = torch.tensor(s, dtype=torch.int32)
        slots = slots.reshape(-1).to(dev)
        last = torch.tensor([b * S + n - 1 for b, n in enumerate(lengths)], dtype=torch.long, device=dev)
        if adapters is not None:  # per row; the padding rows take none
            adapters = [a if s < n else None for a, n in zip(adapters, lengths) for s in range(S)]
        # the B x S x V logits are never formed
        return self._cached_forward(padded.view(-1), cache, slots, (S, None),
                                    lambda i, blk, qkv: blk.attn.causal_attention(qkv, B, S), last, adapters)

    @torch.inference_mode()
    def decode_step(self, tokens, cache, seq_ids, *, adapters=None):
        """One new token per sequence: append its K/V to ``cache`` and return logits ``[B, V]``.
        A ``None`` in ``seq_ids`` is an inactive slot of a fixed-size batch (context length 0,
        nothing cached; its logits row is meaningless). ``adapters``: a LoRA adapter name or
        ``None`` per row."""
        cfg = self.cfg
        dev = self.embed.weight.device
        tokens = torch.as_tensor(tokens, dtype=torch.long).reshape(-1).to(dev)
        B = tokens.shape[0]
        if len(seq_ids) != B or (adapters is not None and len(adapters) != B):
            raise ValueError("tokens, seq_ids and adapters must agree on the batch size")
        pos = [cache.length(s) if s is not None else 0 for s in seq_ids]
        if max(pos) >= cfg.max_seq_len:
            raise ValueError(f"sequence would exceed max_seq_len {cfg.max_seq_len}")
        slots = torch.tensor([s[0] for s in self._allocate(cache, [(s, 1) for s in seq_ids])], dtype=torch.int32,
                             device=dev)
        positions = torch.tensor(pos, dtype=torch.int32, device=dev)
        block_table, context_lens = cache.block_table(seq_ids), cache.context_lens(seq_ids)
        D, Hq, Hk = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads

        def attend(i, blk, qkv):
            ks, vs = cache.scales(i)
            return blk.attn.o(ops.paged_attention_decode(qkv, cache.k[i], cache.v[i], block_table, context_lens,
                                                         Hq, Hk, D, k_scale=ks, v_scale=vs))

        return self._cached_forward(tokens, cache, slots, (1, positions), attend, None, adapters)

    @torch.inference_mode()
    def extend(self, tokens, cache, seq_ids, all_logits: bool = False, num_splits=1, *, adapters=None):
        """Append several new tokens to each sequence and return the logits ``[B, V]`` of each
        sequence's last new token, or with ``all_logits`` the logits ``[sum(len), V]`` of every fed
        row in packed order (draft verification). ``num_splits`` goes to
        ``ops.paged_attention_extend`` (``None``: its heuristic). ``adapters``: a LoRA adapter name
        or ``None`` per sequence, applied to each of its rows.

        ``tokens`` is a list of non-empty token lists; each ``seq_id`` may be new or already cached
        at any length (a prompt chunk, a further chat turn, draft tokens to verify). The batch is
        packed ragged (``sum(len)`` rows, no padding) and attends through
        ``ops.paged_attention_extend`` over the cache, which already holds the new tokens' K/V by
        then. Allocation is all or nothing: on ``KVCacheFull`` the cache is what it was."""
        cfg = self.cfg
        dev = self.embed.weight.device
        rows = [[int(t) for t in r] for r in tokens]
        B = len(rows)
        if len(seq_ids) != B or (adapters is not None and len(adapters) != B):
            raise ValueError("tokens, seq_ids and adapters must agree on the batch size")
        if B == 0 or min(len(r) for r in rows) < 1:
            raise ValueError("extend needs at least one sequence and at least one new token per sequence")
        if len(set(seq_ids)) != B:
            raise ValueError("a sequence may appear once per extend call")
        start = [cache.length(s) for s in seq_ids]
        if max(p + len(r) for p, r in zip(start, rows)) > cfg.max_seq_len:
            raise ValueError(f"sequence would exceed max_seq_len {cfg.max_seq_len}")
        slots = self._allocate(cache, [(s, len(r)) for s, r in zip(seq_ids, rows)])
        flat = torch.tensor([t for r in rows for t in r], dtype=torch.long, device=dev)
        slots = torch.tensor([x for s in slots for x in s], dtype=torch.int32, device=dev)
        positions = torch.tensor([p + i for p, r in zip(start, rows) for i in range(len(r))], dtype=torch.int32,
                                 device=dev)
        cu = list(itertools.accumulate([len(r) for r in rows], initial=0))
        cu_q_lens = torch.tensor(cu, dtype=torch.int32, device=dev)
        max_q_len = max(len(r) for r in rows)
        block_table, context_lens = cache.block_table(seq_ids), cache.context_lens(seq_ids)
        D, Hq, Hk = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads

        def attend(i, blk, qkv):
            ks, vs = cache.scales(i)
            return blk.attn.o(ops.paged_attention_extend(qkv, cache.k[i], cache.v[i], block_table, context_lens,
                                                         cu_q_lens, max_q_len, Hq, Hk, D, num_splits=num_splits,
                                                         k_scale=ks, v_scale=vs))

        last = None if all_logits else torch.tensor([c - 1 for c in cu[1:]], dtype=torch.long, device=dev)
        if adapters is not None:
            adapters = [a for a, r in zip(adapters, rows) for _ in r]
        return self._cached_forward(flat, cache, slots, (1, positions), attend, last, adapters)

    @torch.inference_mode()
    def generate(self, prompts, max_new_tokens, temperature: float = 0.0, top_k: int = 0, eos_token_id=None,
                 seed=None, cache=None, prefill_chunk=None, top_p: float = 1.0, min_p: float = 0.0,
                 fused_sampling: bool = False, speculative=None, kv_cache_dtype=None, adapters=None,
                 repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                 logprobs=None, graph_decode: bool = False):
        """Generate up to ``max_new_tokens`` tokens after each prompt (a list of token-id lists);
        returns the new tokens per prompt. Greedy at ``temperature == 0``, otherwise sampled
        (optionally from the ``top_k`` logits) with a generator seeded by ``seed``. A sequence
        stops after emitting ``eos_token_id``. ``cache``: a ``PagedKVCache`` to use (its blocks are
        released on exit); by default one just large enough is made. ``prefill_chunk``: feed the
        prompts through ``extend``, at most that many tokens per sequence per call, instead of
        one ``prefill``.

        ``top_p`` (nucleus) and ``min_p`` restrict the sampled set further (``ops.sample_logits``
        has the exact rules). They, or ``fused_sampling=True``, select the batched sampler: one
        ``ops.sample_logits`` call per step over all rows, every row seeded with ``seed`` (0 if
        ``None``) and stepped by the number of tokens produced so far, so a row's tokens are a
        function of ``seed`` and its own logits only. Without any of the three the
        ``sample_tokens`` path runs, with the token streams it always gave.

        ``speculative`` (``models/speculative.py``): ``None`` is the loop above; an ``int k`` drafts
        up to ``k`` tokens per sequence and step by prompt lookup (``NgramProposer``), a proposer
        object is used as given. The request then samples through ``ops.sample_logits`` as with
        ``fused_sampling=True``, and its stream is that call's stream wherever ``extend`` and
        ``decode_step`` agree on the logits; ``self.spec_stats`` holds the run's counts.

        ``kv_cache_dtype`` (``None`` / ``"auto"`` / ``"fp8"``) is the dtype of the cache made here
        (a ``cache`` passed in keeps its own). Under fp8, ``prefill`` attends over the fresh,
        unquantised K/V while ``extend`` and ``decode_step`` read the quantised cache, so a
        ``prefill_chunk`` stream may differ from the unchunked one. The speculative guarantee
        holds: the verify ``extend`` and ``decode_step`` read the same quantised bytes.

        ``adapters``: one loaded LoRA adapter name or ``None`` per prompt (``enable_lora_``,
        ``load_adapter``); every forward call of the request routes that sequence's rows to it.

        ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` (``ops.penalize_logits``
        has the exact rules; prompt and produced tokens count for repetition, produced tokens for the
        other two) act on every step's logits before the draw, on the GPU. ``logprobs``: ``None``, or
        the number ``0..20`` of alternatives to record per produced token; the call then returns
        ``(tokens, logprobs)`` with one ``(token, logprob, [(id, logprob), ...])`` entry per token
        (``ops.token_logprobs``: temperature 1, before top-k / top-p / min-p, after the penalties).
        A non-neutral penalty or ``logprobs`` selects the batched sampler like ``fused_sampling``.

        ``graph_decode=True`` runs the decode steps through a ``DecodeRunner``
        (``models/decode_graph.py``): static input buffers and one captured HIP graph per block-table
        bucket, replayed per step; the same body uncaptured when the model is not on a GPU. LoRA
        rounds and speculative verify rounds run as without it. A runner belongs to a cache, so pass
        ``cache=`` to keep its graphs from one call to the next."""
        from .decoding import Sampling, Stream, _seeded_generator, decode_round, sample_rows, sample_tokens
        from .kv_cache import PagedKVCache
        from .speculative import new_stats, resolve_speculative

        proposer, num_draft = resolve_speculative(speculative)
        sampling = Sampling(temperature, top_k, top_p, min_p, seed, fused_sampling or proposer is not None,
                            repetition_penalty, presence_penalty, frequency_penalty, logprobs)
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("prefill_chunk must be >= 1")
        prompts = [list(p) for p in prompts]
        if adapters is not None and len(adapters) != len(prompts):
            raise ValueError("adapters needs one entry per prompt")
        if adapters is not None and all(a is None for a in adapters):
            adapters = None
        akw = {} if adapters is None else {"adapters": list(adapters)}
        if not prompts or max_new_tokens <= 0:
            return ([[] for _ in prompts], [[] for _ in prompts]) if logprobs is not None else [[] for _ in prompts]
        dev = self.embed.weight.device
        if max(len(p) for p in prompts) + max_new_tokens > self.cfg.max_seq_len:
            raise ValueError(f"prompt + max_new_tokens exceeds max_seq_len {self.cfg.max_seq_len}")
        if cache is None:
            page = 16
            blocks = sum(-(-(len(p) + max_new_tokens) // page) for p in prompts)
            cache = PagedKVCache(self.cfg, blocks, page, device=dev, dtype=self.embed.weight.dtype,
                                 kv_dtype=kv_cache_dtype)
        sample = sample_rows
        if not sampling.fused:
            gen = _seeded_generator(dev, temperature, seed)

            def sample(logits, picks):
                # one batched draw on one generator over all rows, those of finished sequences
                # included: the ``sample_tokens`` streams this path always gave
                nxt = sample_tokens(logits, sampling.temperature, sampling.top_k, gen).tolist()
                return [nxt[row] for _, row in picks]

        ids = [("generate", next(_SEQ_IDS)) for _ in prompts]
        streams = [Stream(sid, list(p), max_new_tokens, sampling, eos_token_id, adapter=a)
                   for sid, p, a in zip(ids, prompts, adapters or [None] * len(prompts))]
        slots = list(streams)
        stats = new_stats()
        if proposer is not None:
            self.spec_stats = stats
        rkw = {}
        if graph_decode:
            from .decode_graph import runner_for

            rkw["runner"] = runner_for(self, cache, len(prompts))

        def settle(emitted):
            for b, _, finished in emitted:
                if finished:
                    cache.free(ids[b])
                    slots[b] = None

        try:
            if prefill_chunk is None:
                logits = self.prefill(prompts, None, cache, ids, **akw)
            else:
                logits = self._chunked_prefill(prompts, cache, ids, int(prefill_chunk), adapters)
            first = sample(logits, [(st, b) for b, st in enumerate(streams)])
            settle([(b, [tok], st.advance([tok])) for b, (st, tok) in enumerate(zip(streams, first))])
            while any(st is not None for st in slots):
                settle(decode_round(self, cache, slots, proposer, num_draft, stats, sample, **rkw))
        finally:
            for sid in ids:
                cache.free(sid)
        out = [st.history[len(p):] for st, p in zip(streams, prompts)]
        return (out, [st.logprobs for st in streams]) if logprobs is not None else out

    def _chunked_prefill(self, prompts, cache, ids, chunk, adapters=None):
        """``prefill`` through ``extend``: ``chunk`` tokens per unfinished prompt per call."""
        logits = [None] * len(prompts)
        for off in range(0, max(len(p) for p in prompts), chunk):
            idx = [b for b, p in enumerate(prompts) if off < len(p)]
            akw = {} if adapters is None else {"adapters": [adapters[b] for b in idx]}
            lg = self.extend([prompts[b][off: off + chunk] for b in idx], cache, [ids[b] for b in idx], **akw)
            for j, b in enumerate(idx):
                if off + chunk >= len(prompts[b]):
                    logits[b] = lg[j]
        return torch.stack(logits)


_SEQ_IDS = itertools.count()


# sampling lives with the decode round; these names stay importable from here
from .decoding import _seeded_generator, sample_tokens, use_fused_sampling  # noqa: E402,F401


def build_llama(name_or_cfg="llama3-8b", device=None, dtype=torch.bfloat16, weight_dtype=None, **overrides) -> Llama:
    """``weight_dtype``: ``None`` / ``"auto"`` keep the linears in ``dtype``; ``"fp8"`` quantises them
    (``Llama.quantize_weights_``) after the cast."""
    cfg = PRESETS[name_or_cfg] if isinstance(name_or_cfg, str) else name_or_cfg
    if overrides:
        cfg = LlamaConfig(**{**cfg.__dict__, **overrides})
    if device is not None and str(device).startswith("cuda"):
        with torch.device(device):
            m = Llama(cfg)
    else:
        m = Llama(cfg)
    return m.to(dtype=dtype).quantize_weights_(weight_dtype)
