"""Llama token streaming on Serve: one replica = one model + one continuous-batching engine.

    app = LlamaDeployment.bind("llama3-1b", state_dict_path="/ckpt/model.pt", device="cuda")
    handle = serve.run(app, route_prefix="/llm")
    for tok in handle.options(method_name="generate", stream=True).remote([1, 2, 3], max_new_tokens=32):
        ...

Concurrent requests share the engine's decode batch (``models.GenerationEngine``): a background
asyncio task steps the engine on a worker thread and hands every produced token to its request's
queue, so tokens reach callers one by one. Token ids in, token ids out: no tokenizer.
"""
from __future__ import annotations

import asyncio
import concurrent.futures
import json

from .api import deployment


class _LlamaDeployment:
    def __init__(self, model="llama3-tiny", state_dict_path=None, device="cpu", dtype="bfloat16", max_slots: int = 8,
                 num_blocks=None, page_size: int = 16, seed: int = 0, default_max_new_tokens: int = 16,
                 prefill_chunk=None, fused_sampling: bool = False, speculative=None, kv_cache_dtype=None,
                 cache_bytes=None, weight_dtype=None, lora=None, adapters=None, graph_decode: bool = False):
        """``model``: a preset name or a ``LlamaConfig``; ``state_dict_path``: optional
        ``torch.save``d state dict (without one the weights are initialised from ``seed``);
        ``prefill_chunk``: prompt tokens the engine spends per step (chunked prefill: a long prompt
        no longer pauses the running streams for its whole prefill); ``None`` prefills in one go;
        ``fused_sampling``: every request samples through the engine's batched sampler
        (``ops.sample_logits``: one launch a step) instead of only those that set ``top_p`` / ``min_p``;
        ``speculative``: draft tokens per step by prompt lookup (or a proposer object), verified in
        one forward (``GenerationEngine(speculative=...)``; implies ``fused_sampling``);
        ``num_blocks`` (default 256) or ``cache_bytes`` size the KV cache and ``kv_cache_dtype``
        (``"fp8"``: quantised pages, about half the bytes per token) picks its dtype, as in
        ``GenerationEngine``; ``weight_dtype`` (``None`` / ``"auto"`` / ``"fp8"``): ``"fp8"`` quantises
        the linears' weights once the state dict is loaded (``Llama.quantize_weights_``: half the
        weight bytes, activations stay in ``dtype``); ``lora={"max_adapters": n, "max_rank": r}``
        makes room for LoRA adapters (``Llama.enable_lora_``, after the quantisation) that requests
        select by name, and ``adapters={"name": path}`` preloads ``LoraAdapter.save``d files;
        ``graph_decode``: the engine replays its decode step as a captured HIP graph
        (``GenerationEngine(graph_decode=True)``; on a CPU model the same step runs uncaptured)."""
        import torch

        from ..models import GenerationEngine, LoraAdapter, build_llama, weight_bytes

        torch.manual_seed(seed)
        self.model = build_llama(model, device=device, dtype=getattr(torch, dtype) if isinstance(dtype, str) else dtype)
        if state_dict_path is not None:
            self.model.load_state_dict(torch.load(state_dict_path, map_location=device))
        self.model.quantize_weights_(weight_dtype)
        self.lora = None
        if lora is not None:
            self.lora = {"max_adapters": int(lora["max_adapters"]), "max_rank": int(lora["max_rank"])}
            self.model.enable_lora_(**self.lora)
        elif adapters:
            raise ValueError("adapters= needs lora={'max_adapters': n, 'max_rank': r}")
        for name, path in (adapters or {}).items():
            self.model.load_adapter(name, LoraAdapter.load(path))
        self.model.eval()
        self.weight_dtype = "fp8" if weight_dtype == "fp8" else None
        self.weight_bytes = weight_bytes(self.model)
        self.engine = GenerationEngine(self.model, max_slots=max_slots, num_blocks=num_blocks, page_size=page_size,
                                       prefill_chunk=prefill_chunk, fused_sampling=fused_sampling,
                                       speculative=speculative, kv_cache_dtype=kv_cache_dtype,
                                       cache_bytes=cache_bytes, **({"graph_decode": True} if graph_decode else {}))
        self.default_max_new_tokens = int(default_max_new_tokens)
        # one model thread: the engine is not re-entrant, and per-thread GPU library state stays warm
        self._exec = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="llama-engine")
        # request id -> (queue, max_new_tokens, tokens routed so far, wants logprobs). Entries are added on the engine
        # thread (generate.add) and read / removed on the event loop: single dict operations, which the
        # GIL makes atomic, and an entry is complete before its request can produce a token.
        self._queues = {}
        self._driver = None
        self._cancelled = 0  # requests dropped because their consumer went away

    async def _drive(self):
        """Step the engine while it has work; route each token to its request's queue."""
        loop = asyncio.get_running_loop()
        try:
            while self._queues or self.engine.has_work():
                events = await loop.run_in_executor(self._exec, self.engine.step)
                lps = {}  # request id -> iterator over its new logprob entries, aligned with its events
                for rid, tok, finished in events:
                    entry = self._queues.get(rid)
                    if entry is not None:
                        entry[2] += 1
                        if entry[3]:
                            if rid not in lps:
                                lps[rid] = iter(self.engine.pop_logprobs(rid))
                            _, lp, top = next(lps[rid])
                            tok = {"token": tok, "logprob": lp, "top_logprobs": [[i, v] for i, v in top]}
                        entry[0].put_nowait((tok, finished))
                    else:
                        self.engine.pop_logprobs(rid)  # the consumer went away: nobody will ask for them
                if not events and not self.engine.num_prefilling:
                    await asyncio.sleep(0.001)  # everything is waiting for cache blocks
        except BaseException as e:  # a failed step fails every open stream instead of hanging it
            for entry in self._queues.values():
                entry[0].put_nowait(e)
            raise
        finally:
            self._driver = None

    async def generate(self, prompt_tokens, max_new_tokens=None, temperature: float = 0.0, top_k: int = 0,
                       eos_token_id=None, seed=None, top_p: float = 1.0, min_p: float = 0.0, adapter=None,
                       repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                       frequency_penalty: float = 0.0, logprobs=None):
        """Async generator of the new token ids of one request (sampling arguments as in
        ``GenerationEngine.add_request``). ``adapter``: the name of a loaded LoRA adapter; without
        one, a non-empty ``serve.get_multiplexed_model_id()`` of the request is the name. With
        ``logprobs`` (``0..20`` alternatives) every item is ``{"token": id, "logprob": lp,
        "top_logprobs": [[id, lp], ...]}`` instead of a bare id."""
        from .multiplex import get_multiplexed_model_id

        if adapter is None and self.lora is not None:
            adapter = get_multiplexed_model_id() or None
        loop = asyncio.get_running_loop()
        n = self.default_max_new_tokens if max_new_tokens is None else int(max_new_tokens)
        q = asyncio.Queue()

        def add():  # on the engine thread, so no step can run between queueing and registering
            rid = self.engine.add_request(list(prompt_tokens), n, temperature=temperature, top_k=top_k,
                                          eos_token_id=eos_token_id, seed=seed, top_p=top_p, min_p=min_p,
                                          repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                                          frequency_penalty=frequency_penalty, logprobs=logprobs,
                                          **({} if adapter is None else {"adapter": adapter}))
            self._queues[rid] = [q, n, 0, logprobs is not None]
            return rid

        rid = await loop.run_in_executor(self._exec, add)
        if self._driver is None:
            self._driver = asyncio.ensure_future(self._drive())
        finished = False
        try:
            while not finished:
                item = await q.get()
                if isinstance(item, BaseException):
                    finished = True  # the engine failed: nothing left to cancel
                    raise RuntimeError(f"generation failed: {item!r}")
                tok, finished = item
                yield tok
        finally:
            del self._queues[rid]
            if not finished:  # the consumer went away: give the slot and the cache blocks back
                self._cancelled += 1
                loop.run_in_executor(self._exec, self.engine.cancel, rid)

    async def load_adapter(self, name, path):
        """Load a ``LoraAdapter.save``d file under ``name`` (on the engine thread, between steps)."""
        from ..models import LoraAdapter

        loop = asyncio.get_running_loop()
        await loop.run_in_executor(self._exec, lambda: self.engine.load_adapter(name, LoraAdapter.load(path)))
        return self.model.loaded_adapters()

    async def unload_adapter(self, name):
        """Free an adapter's slot; fails while a request or a prefix uses it."""
        loop = asyncio.get_running_loop()
        await loop.run_in_executor(self._exec, self.engine.unload_adapter, name)
        return self.model.loaded_adapters()

    async def status(self):
        """Engine occupancy and, per open stream, how far it is: ``{"active", "waiting", "streams":
        [{"request_id", "max_new_tokens", "produced"}], "cancelled"}``; a deployment with
        ``prefill_chunk`` set adds ``"prefill_chunk"`` and ``"prefilling"`` (requests still in
        their prompt), one with ``fused_sampling`` adds ``"fused_sampling": True``, one with
        ``speculative`` adds ``"speculative": {"num_draft", **engine.spec_stats}``, one with an fp8
        cache adds ``"kv_cache_dtype": "fp8"``, ``"num_blocks"`` and ``"cache_bytes"``, one with fp8
        weights adds ``"weight_dtype": "fp8"`` and ``"weight_bytes"`` (the model's parameters and buffers),
        one with ``lora`` adds ``"lora": {"max_adapters", "max_rank", "loaded": [...], "bank_bytes"}``,
        one with ``graph_decode`` adds ``"graph_decode": {"graphs", "replays", "eager_warm", "eager_fallback"}``."""
        streams = [{"request_id": rid, "max_new_tokens": e[1], "produced": e[2]}
                   for rid, e in list(self._queues.items())]
        st = {"active": self.engine.num_active, "waiting": len(self.engine.waiting), "streams": streams,
              "cancelled": self._cancelled}
        if self.engine.prefill_chunk is not None:
            st.update(prefill_chunk=self.engine.prefill_chunk, prefilling=self.engine.num_prefilling)
        if self.engine.fused_sampling:
            st.update(fused_sampling=True)
        if self.engine.num_draft:
            st.update(speculative={"num_draft": self.engine.num_draft, **self.engine.spec_stats})
        cache = self.engine.cache
        if cache.fp8:
            st.update(kv_cache_dtype="fp8", num_blocks=cache.num_blocks, cache_bytes=cache.nbytes)
        if self.weight_dtype is not None:
            st.update(weight_dtype=self.weight_dtype, weight_bytes=self.weight_bytes)
        if self.lora is not None:
            from ..models.lora import bank_bytes

            st.update(lora={**self.lora, "loaded": self.model.loaded_adapters(), "bank_bytes": bank_bytes(self.model)})
        if self.engine.runner is not None:
            st.update(graph_decode=dict(self.engine.runner.stats))
        return st

    async def __call__(self, request):
        """HTTP: JSON body ``{"prompt_tokens": [...], "max_new_tokens": n}`` (optionally
        ``temperature``, ``top_k``, ``top_p``, ``min_p``, ``eos_token_id``, ``seed``, ``adapter``,
        ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty``, ``logprobs``) -> newline-delimited
        token ids, or with ``logprobs`` one JSON object ``{"token", "logprob", "top_logprobs"}`` per line."""
        body = json.loads(await request.body())
        kw = {k: body[k] for k in ("max_new_tokens", "temperature", "top_k", "top_p", "min_p", "eos_token_id", "seed",
                                          "adapter", "repetition_penalty", "presence_penalty", "frequency_penalty",
                                          "logprobs")
              if k in body}

        async def lines():
            async for tok in self.generate(body["prompt_tokens"], **kw):
                yield f"{json.dumps(tok) if isinstance(tok, dict) else tok}\n"

        return lines()


LlamaDeployment = deployment(_LlamaDeployment, name="LlamaDeployment")
