"""Continuous batching for Llama generation: a fixed number of decode slots over one paged cache.

``GenerationEngine.step()`` admits waiting requests (one prefill for the newly admitted ones),
runs one ``decode_step`` over all slots (inactive slots ride along at context length 0) and
retires finished sequences, freeing their blocks. Pure Python over ``PagedKVCache`` and the
``Llama`` inference methods; it runs on whatever device the model is on.

With ``prefill_chunk`` set, an admitted request is *prefilling*: every step feeds at most that
many prompt tokens (arrival order, one ``Llama.extend`` call) before the decode step, so a long
prompt no longer stalls the running streams for its whole prefill. ``register_prefix`` keeps a
prompt prefix in a pinned sequence whose whole pages later requests share (``PagedKVCache.fork``)
instead of recomputing and storing them again.

The decode phase of a step is one ``decode_round`` (``models/decoding.py``, shared with
``Llama.generate``) over the slots that are past their prompt. With ``speculative`` set
(``models/speculative.py``), a round in which at least one live slot has a draft is one
``Llama.extend`` over the live slots' ``[last token] + draft`` rows: every request emits the tokens
the batched sampler would have drawn one step at a time, and the rejected drafts are rolled back
out of the cache.
"""
from __future__ import annotations

import itertools
from collections import deque
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from .decoding import Sampling, Stream, _seeded_generator, decode_round, sample_rows
from .kv_cache import PagedKVCache
from .speculative import new_stats, resolve_speculative


@dataclass(kw_only=True)
class _Request(Stream):
    """A ``Stream`` (``history`` starts as shared prefix + prompt) with its admission and prefill state."""
    rid: int
    blocks: int                     # blocks the finished sequence will hold
    # chunked prefill / shared prefix (models.Llama.extend); unused on the plain prefill path
    feed: List[int] = field(default_factory=list)   # tokens to run through extend
    fed: int = 0                                    # ... of which this many are cached
    prefilling: bool = False
    prefix: Optional["_Prefix"] = None              # held until the prefill is over
    forked: bool = False
    shared: int = 0                                 # blocks shared with the prefix (not in ``blocks``)


@dataclass
class _Prefix:
    handle: int
    tokens: List[int]
    seq_id: tuple
    blocks: int
    fed: int = 0
    users: int = 0           # requests accepted with this prefix whose prefill is not over
    reserved: bool = False   # its blocks are counted in the admission budget
    released: bool = False
    adapter: Optional[str] = None   # the LoRA adapter its K/V was computed with


_NO_LIMIT = 1 << 62


class GenerationEngine:
    def __init__(self, model, cache: Optional[PagedKVCache] = None, max_slots: int = 8,
                 num_blocks: Optional[int] = None, page_size: int = 16, prefill_chunk: Optional[int] = None,
                 fused_sampling: bool = False, speculative=None, kv_cache_dtype=None,
                 cache_bytes: Optional[int] = None, graph_decode: bool = False):
        """``speculative``: ``None``, a number of draft tokens per step (prompt lookup,
        ``NgramProposer``) or a proposer object; it implies ``fused_sampling``, since a draft is
        verified by re-drawing its token with ``ops.sample_logits``.

        The engine's own cache has ``num_blocks`` blocks (default 256), or as many as fit into
        ``cache_bytes`` (``PagedKVCache.block_bytes``; giving both is an error), of
        ``kv_cache_dtype`` (``None`` / ``"auto"``: the model's dtype; ``"fp8"``: e4m3 pages with
        per-token scales, ``(D + 4) / 2D`` of the bf16 bytes per block). Under fp8, ``prefill``
        attends over the fresh, unquantised K/V while ``extend`` and ``decode_step`` read the
        quantised cache, so a ``prefill_chunk`` stream may differ from the unchunked one;
        speculative decoding keeps its guarantee, since the verify ``extend`` and ``decode_step``
        read the same quantised bytes.

        ``graph_decode=True`` runs the decode step of every round through a ``DecodeRunner`` over the
        engine's cache and ``max_slots`` rows (``models/decode_graph.py``: static buffers, one
        captured HIP graph per block-table bucket; the uncaptured body when the model is not on a
        GPU). ``self.runner.stats`` counts graphs, replays and the rounds that ran eagerly."""
        if num_blocks is not None and cache_bytes is not None:
            raise ValueError("give num_blocks or cache_bytes, not both")
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("prefill_chunk must be >= 1")
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        self._proposer, self.num_draft = resolve_speculative(speculative)
        self.fused_sampling = bool(fused_sampling) or self._proposer is not None
        self.spec_stats = new_stats()
        self._prefixes = {}
        self._logprobs = {}   # request id -> entries not popped yet (requests with ``logprobs`` only)
        self.model = model
        w = model.embed.weight
        if cache is None:
            if cache_bytes is not None:
                num_blocks = int(cache_bytes) // PagedKVCache.block_bytes(model.cfg, page_size, w.dtype, kv_cache_dtype)
                if num_blocks < 1:
                    raise ValueError(f"cache_bytes = {cache_bytes} holds no block of this model")
            cache = PagedKVCache(model.cfg, 256 if num_blocks is None else num_blocks, page_size, device=w.device,
                                 dtype=w.dtype, kv_dtype=kv_cache_dtype)
        self.cache = cache
        self.slots: List[Optional[_Request]] = [None] * int(max_slots)
        self.waiting = deque()
        self._ids = itertools.count()
        self.runner = None
        if graph_decode:
            from .decode_graph import DecodeRunner

            self.runner = DecodeRunner(model, cache, len(self.slots))
        self._round_kw = {} if self.runner is None else {"runner": self.runner}

    # -------------------------------------------------------------------------------- requests
    def _check_adapter(self, adapter):
        if adapter is not None and adapter not in getattr(self.model, "loaded_adapters", lambda: [])():
            raise ValueError(f"unknown adapter {adapter!r}: load it first (load_adapter)")

    def load_adapter(self, name, adapter):
        """``Llama.load_adapter`` on the engine's model."""
        return self.model.load_adapter(name, adapter)

    def adapter_users(self, name) -> int:
        """Waiting and active requests and registered prefixes that use adapter ``name``."""
        reqs = [r for r in list(self.waiting) + self.slots if r is not None]
        return sum(o.adapter == name for o in reqs + list(self._prefixes.values()))

    def unload_adapter(self, name):
        """Free the adapter's slot; refused while a request or a registered prefix uses it."""
        users = self.adapter_users(name)
        if users:
            raise RuntimeError(f"adapter {name!r} is in use by {users} request(s) / prefix(es)")
        self.model.unload_adapter(name)

    def register_prefix(self, tokens, adapter: Optional[str] = None) -> int:
        """Register a prompt prefix (system prompt, few-shot header) that requests can share;
        returns its handle. The prefix is prefilled once into a pinned sequence, lazily, by the
        first ``step()`` that needs it and through the same ``prefill_chunk`` budget. Its cached K/V
        belongs to ``adapter`` (a loaded LoRA adapter or ``None``): requests naming the prefix must
        name the same adapter."""
        self._check_adapter(adapter)
        tokens = [int(t) for t in tokens]
        if not tokens:
            raise ValueError("a prefix needs at least one token")
        if len(tokens) >= self.model.cfg.max_seq_len:
            raise ValueError(f"prefix of {len(tokens)} tokens leaves no room under max_seq_len "
                             f"{self.model.cfg.max_seq_len}")
        handle = next(self._ids)
        self._prefixes[handle] = _Prefix(handle, tokens, ("engine-prefix", id(self), handle),
                                         -(-len(tokens) // self.cache.page_size), adapter=adapter)
        return handle

    def release_prefix(self, handle: int) -> None:
        """Unpin a prefix: no new request may name it, and its blocks go back once the last
        request sharing them retires."""
        pfx = self._prefixes.pop(handle, None)
        if pfx is None:
            raise ValueError(f"unknown or released prefix handle {handle!r}")
        pfx.released = True
        self._drop_prefix_if_unused(pfx)

    def _drop_prefix_if_unused(self, pfx: "_Prefix"):
        if pfx.released and pfx.users == 0:
            self.cache.free(pfx.seq_id)  # shared pages live on until their last sharer retires
            pfx.fed, pfx.reserved = 0, False

    def _unhold_prefix(self, req: "_Request"):
        if req.prefix is not None:
            pfx, req.prefix = req.prefix, None
            pfx.users -= 1
            self._drop_prefix_if_unused(pfx)

    def add_request(self, prompt, max_new_tokens: int, temperature: float = 0.0, top_k: int = 0, eos_token_id=None,
                    seed=None, prefix: Optional[int] = None, top_p: float = 1.0, min_p: float = 0.0,
                    adapter: Optional[str] = None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                    frequency_penalty: float = 0.0, logprobs: Optional[int] = None) -> int:
        """Queue a request; returns its id. It is admitted by a later ``step()`` once a slot is
        free and the cache can hold its whole sequence (prompt + ``max_new_tokens``). With
        ``prefix`` (a ``register_prefix`` handle) ``prompt`` is the suffix after that prefix: the
        request shares the prefix's whole cache pages and needs blocks only for the rest.

        ``top_p`` / ``min_p`` (``ops.sample_logits``) or the engine's ``fused_sampling`` put the
        request on the batched sampler: all such rows of a step's logits are sampled by one call,
        each with ``seed`` (0 if ``None``) and its own count of produced tokens as the step.

        ``adapter``: a loaded LoRA adapter's name (``Llama.load_adapter``); every forward row of the
        request is routed to it. With a ``prefix`` it must be the prefix's adapter.

        ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` (``ops.penalize_logits``;
        a shared prefix counts as prompt) and ``logprobs`` (``None``, or ``0..20`` alternatives per
        token, fetched with ``pop_logprobs``) also put the request on the batched sampler."""
        self._check_adapter(adapter)
        sampling = Sampling(temperature, top_k, top_p, min_p, seed, self.fused_sampling, repetition_penalty,
                            presence_penalty, frequency_penalty, logprobs)
        prompt = [int(t) for t in prompt]
        if not prompt or max_new_tokens < 1:
            raise ValueError("a request needs a non-empty prompt and max_new_tokens >= 1")
        pfx = None
        if prefix is not None:
            pfx = self._prefixes.get(prefix)
            if pfx is None:
                raise ValueError(f"unknown or released prefix handle {prefix!r}")
            if pfx.adapter != adapter:
                raise ValueError(f"prefix {prefix!r} was registered with adapter {pfx.adapter!r}, the request names "
                                 f"{adapter!r}: cached K/V belongs to the adapter it was computed with")
        page = self.cache.page_size
        whole = len(pfx.tokens) // page * page if pfx is not None else 0
        total = (len(pfx.tokens) if pfx is not None else 0) + len(prompt) + int(max_new_tokens)
        if total > self.model.cfg.max_seq_len:
            raise ValueError(f"prompt + max_new_tokens = {total} exceeds max_seq_len {self.model.cfg.max_seq_len}")
        if self.prefill_chunk is None and pfx is None:
            padded = -(-len(prompt) // 128) * 128  # what prefill pads the prompt to
            if padded > self.model.cfg.max_seq_len:
                raise ValueError(f"prompt of {len(prompt)} tokens pads to {padded} > max_seq_len "
                                 f"{self.model.cfg.max_seq_len}")
        blocks = -(-total // page) - whole // page  # shared pages are the prefix's, not the request's
        if blocks + (pfx.blocks if pfx is not None else 0) > self.cache.num_blocks:
            raise ValueError(f"request needs {blocks} cache blocks, the cache has {self.cache.num_blocks}")
        gen = _seeded_generator(self.model.embed.weight.device, temperature, seed)
        rid = next(self._ids)
        req = _Request(seq_id=("engine", id(self), rid), history=list(prompt), max_new_tokens=int(max_new_tokens),
                       sampling=sampling, eos_token_id=eos_token_id, generator=gen, rid=rid, blocks=blocks,
                       feed=prompt, adapter=adapter)
        if pfx is not None:
            req.prefix = pfx
            pfx.users += 1
            req.feed = pfx.tokens[whole:] + prompt  # the partly filled page is recomputed per request
            req.history = pfx.tokens + prompt
            req.prompt_len = len(req.history)
        self.waiting.append(req)
        return rid

    def cancel(self, request_id: int) -> bool:
        """Drop a request, waiting or active: its slot and cache blocks are free at once and it
        produces no further tokens. Returns False if the request is unknown or already finished."""
        for req in self.waiting:
            if req.rid == request_id:
                self.waiting.remove(req)
                self._unhold_prefix(req)
                return True
        for slot, req in enumerate(self.slots):
            if req is not None and req.rid == request_id:
                self._retire(slot)
                self._logprobs.pop(request_id, None)
                return True
        return False

    def pop_logprobs(self, request_id: int) -> list:
        """The ``(token, logprob, [(id, logprob), ...])`` entries of a request with ``logprobs`` that
        were produced since the last call, one per ``step()`` event of that request and in their
        order; ``[]`` if there are none."""
        return self._logprobs.pop(request_id, [])

    def has_work(self) -> bool:
        return bool(self.waiting) or any(r is not None for r in self.slots)

    @property
    def num_active(self) -> int:
        return sum(r is not None for r in self.slots)

    @property
    def num_prefilling(self) -> int:
        return sum(r is not None and r.prefilling for r in self.slots)

    def _reserved(self) -> int:
        """Blocks the active requests (and the prefixes they wait for) may still take."""
        own = sum(r.blocks + r.shared - self.cache.blocks_held(r.seq_id) for r in self.slots if r is not None)
        pfx = {id(r.prefix): r.prefix for r in list(self.slots) + list(self.waiting)
               if r is not None and r.prefix is not None and r.prefix.reserved}
        return own + sum(p.blocks - self.cache.blocks_held(p.seq_id) for p in pfx.values())

    # ------------------------------------------------------------------------------------ step
    def _emit(self, slot: int, toks, finished: bool, events):
        """The events of one request's tokens of one round (only the last can finish it); a
        finished request retires."""
        req = self.slots[slot]
        rid = req.rid
        events.extend((rid, tok, finished and n + 1 == len(toks)) for n, tok in enumerate(toks))
        if req.sampling.logprobs is not None:
            self._logprobs.setdefault(rid, []).extend(req.logprobs[-len(toks):])
        if finished:
            self._retire(slot)

    def _retire(self, slot: int):
        req = self.slots[slot]
        self.cache.free(req.seq_id)
        self._unhold_prefix(req)
        self.slots[slot] = None

    def _requeue(self, slots):
        """Back to the head of the queue, in arrival order, with nothing cached."""
        for slot in sorted(slots, key=lambda s: self.slots[s].rid, reverse=True):
            req = self.slots[slot]
            self.cache.free(req.seq_id)
            req.fed, req.prefilling, req.forked, req.shared = 0, False, False, 0
            self.waiting.appendleft(req)
            self.slots[slot] = None

    def _admit(self):
        """Give free slots to waiting requests, in arrival order, as prefilling: a request that
        does not fit waits (and keeps its place)."""
        budget = self.cache.num_free_blocks - self._reserved()
        while self.waiting and None in self.slots:
            req = self.waiting[0]
            pfx = req.prefix if req.prefix is not None and not req.prefix.reserved else None
            need = req.blocks + (pfx.blocks if pfx is not None else 0)
            if need > budget:
                break
            self.waiting.popleft()
            budget -= need
            if pfx is not None:
                pfx.reserved = True
            self.slots[self.slots.index(None)] = req
            req.prefilling = True

    def _feed(self, call, items, events):
        """One prefill call over ``items`` ``(slot or None, request or prefix, tokens)``:
        ``call(token lists, cache, seq_ids)`` gives one logits row per item (it gets ``adapters=``
        only if an item has a LoRA adapter). A request whose prompt
        is now cached emits its first token and retires or stays; returns the ids of those that
        stay. If the call fails it cached nothing (it is all or nothing): its requests go back to
        the head of the queue in arrival order, so no slot decodes a sequence that was never
        prefilled."""
        try:
            akw = {"adapters": [o.adapter for _, o, _ in items]} if any(o.adapter is not None for _, o, _ in items) else {}
            logits = call([t for _, _, t in items], self.cache, [o.seq_id for _, o, _ in items], **akw)
        except Exception:
            self._requeue([slot for slot, _, _ in items if slot is not None])
            raise
        done, emit = set(), []
        for i, (slot, obj, toks) in enumerate(items):
            obj.fed += len(toks)
            if slot is not None and obj.fed >= len(obj.feed):
                emit.append((slot, obj, i))
        for (slot, obj, _), tok in zip(emit, sample_rows(logits, [(obj, i) for _, obj, i in emit])):
            obj.prefilling = False
            self._unhold_prefix(obj)
            finished = obj.advance([tok])
            self._emit(slot, [tok], finished, events)
            if not finished:
                done.add(obj.rid)
        return done

    def _prefill(self, events):
        """The prompt work of one step. Requests with neither ``prefill_chunk`` nor a prefix take
        one ``prefill`` call for their whole prompts and decode in this same step. The others are
        fed up to ``prefill_chunk`` prompt tokens, in arrival order and in one ``extend`` call; a
        request whose prefix is not cached yet waits while the prefix takes its turn. Returns the
        ids of the requests that finished their prompt through ``extend``: they decode from the
        next step on."""
        if self.prefill_chunk is None:
            plain = [(s, r, r.feed) for s, r in enumerate(self.slots)
                     if r is not None and r.prefilling and r.prefix is None]
            if plain:
                self._feed(lambda toks, cache, ids, **kw: self.model.prefill(toks, None, cache, ids, **kw), plain, events)
        pre = sorted((s for s, r in enumerate(self.slots) if r is not None and r.prefilling),
                     key=lambda s: self.slots[s].rid)
        budget = self.prefill_chunk if self.prefill_chunk is not None else _NO_LIMIT
        items, busy = [], set()
        for slot in pre:
            if budget <= 0:
                break
            req = self.slots[slot]
            pfx = req.prefix
            if pfx is not None and not req.forked:
                if pfx.fed < len(pfx.tokens):
                    if pfx.handle not in busy:
                        n = min(budget, len(pfx.tokens) - pfx.fed)
                        items.append((None, pfx, pfx.tokens[pfx.fed: pfx.fed + n]))
                        busy.add(pfx.handle)
                        budget -= n
                    continue
                whole = len(pfx.tokens) // self.cache.page_size * self.cache.page_size
                self.cache.fork(pfx.seq_id, req.seq_id, whole)
                req.forked, req.shared = True, whole // self.cache.page_size
            n = min(budget, len(req.feed) - req.fed)
            items.append((slot, req, req.feed[req.fed: req.fed + n]))
            budget -= n
        return self._feed(self.model.extend, items, events) if items else set()

    def _decode(self, joined, events):
        """One decode round over the slots; requests still in their prompt, or that left it through
        ``extend`` in this step (``joined``), ride along as inactive slots."""
        live = [r if r is not None and not r.prefilling and r.rid not in joined else None for r in self.slots]
        for slot, toks, finished in decode_round(self.model, self.cache, live, self._proposer, self.num_draft,
                                                 self.spec_stats, **self._round_kw):
            self._emit(slot, toks, finished, events)

    def step(self) -> List[Tuple[int, int, bool]]:
        """Admit, prefill, decode once, retire. Returns ``(request_id, token, finished)`` for every
        token produced in this step, in production order."""
        events: List[Tuple[int, int, bool]] = []
        self._admit()
        self._decode(self._prefill(events), events)
        return events
