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

With ``speculative`` set (``models/speculative.py``), the decode phase of a step in which at least
one live slot has a draft is one ``Llama.extend`` over the live slots' ``[last token] + draft``
rows: every request emits the tokens the batched sampler would have drawn one step at a time, and
the rejected drafts are rolled back out of the cache.
"""
from __future__ import annotations

import itertools
from collections import deque
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from .. import ops
from .kv_cache import PagedKVCache
from .llama import _seeded_generator, sample_tokens, use_fused_sampling
from .speculative import accept, draft_for, new_stats, resolve_speculative


@dataclass
class _Request:
    rid: int
    prompt: List[int]
    max_new_tokens: int
    temperature: float
    top_k: int
    eos_token_id: Optional[int]
    generator: Optional[torch.Generator]
    blocks: int                      # blocks the finished sequence will hold
    produced: int = 0
    last: int = 0                    # last emitted token (the next decode input)
    seq_id: tuple = field(default=())
    # chunked prefill / shared prefix (models.Llama.extend); unused on the plain prefill path
    feed: List[int] = field(default_factory=list)   # tokens to run through extend
    fed: int = 0                                    # ... of which this many are cached
    prefilling: bool = False
    prefix: Optional["_Prefix"] = None              # held until the prefill is over
    forked: bool = False
    shared: int = 0                                 # blocks shared with the prefix (not in ``blocks``)
    # batched sampler (ops.sample_logits): stepped by ``produced``, so the stream is a function of
    # the seed and the request's own logits, never of its slot or its neighbours
    top_p: float = 1.0
    min_p: float = 0.0
    seed: int = 0
    fused: bool = False
    # shared prefix + prompt + produced tokens: what a speculative proposer drafts from
    history: List[int] = field(default_factory=list)


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


_NO_LIMIT = 1 << 62


class GenerationEngine:
    def __init__(self, model, cache: Optional[PagedKVCache] = None, max_slots: int = 8, num_blocks: int = 256,
                 page_size: int = 16, prefill_chunk: Optional[int] = None, fused_sampling: bool = False,
                 speculative=None):
        """``speculative``: ``None``, a number of draft tokens per step (prompt lookup,
        ``NgramProposer``) or a proposer object; it implies ``fused_sampling``, since a draft is
        verified by re-drawing its token with ``ops.sample_logits``."""
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("prefill_chunk must be >= 1")
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        self._proposer, self.num_draft = resolve_speculative(speculative)
        self.fused_sampling = bool(fused_sampling) or self._proposer is not None
        self.spec_stats = new_stats()
        self._prefixes = {}
        self.model = model
        w = model.embed.weight
        self.cache = cache if cache is not None else PagedKVCache(model.cfg, num_blocks, page_size, device=w.device,
                                                                  dtype=w.dtype)
        self.slots: List[Optional[_Request]] = [None] * int(max_slots)
        self.waiting = deque()
        self._ids = itertools.count()
        self._sample = sample_tokens

    # -------------------------------------------------------------------------------- requests
    def register_prefix(self, tokens) -> int:
        """Register a prompt prefix (system prompt, few-shot header) that requests can share;
        returns its handle. The prefix is prefilled once into a pinned sequence, lazily, by the
        first ``step()`` that needs it and through the same ``prefill_chunk`` budget."""
        tokens = [int(t) for t in tokens]
        if not tokens:
            raise ValueError("a prefix needs at least one token")
        if len(tokens) >= self.model.cfg.max_seq_len:
            raise ValueError(f"prefix of {len(tokens)} tokens leaves no room under max_seq_len "
                             f"{self.model.cfg.max_seq_len}")
        handle = next(self._ids)
        self._prefixes[handle] = _Prefix(handle, tokens, ("engine-prefix", id(self), handle),
                                         -(-len(tokens) // self.cache.page_size))
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
                    seed=None, prefix: Optional[int] = None, top_p: float = 1.0, min_p: float = 0.0) -> int:
        """Queue a request; returns its id. It is admitted by a later ``step()`` once a slot is
        free and the cache can hold its whole sequence (prompt + ``max_new_tokens``). With
        ``prefix`` (a ``register_prefix`` handle) ``prompt`` is the suffix after that prefix: the
        request shares the prefix's whole cache pages and needs blocks only for the rest.

        ``top_p`` / ``min_p`` (``ops.sample_logits``) or the engine's ``fused_sampling`` put the
        request on the batched sampler: all such rows of a step's logits are sampled by one call,
        each with ``seed`` (0 if ``None``) and its own count of produced tokens as the step."""
        fused = use_fused_sampling(self.fused_sampling, top_p, min_p)
        ops.check_sampling_params([float(temperature)] if fused else [], [int(top_k)] if fused else [],
                                  [float(top_p)], [float(min_p)])
        prompt = [int(t) for t in prompt]
        if not prompt or max_new_tokens < 1:
            raise ValueError("a request needs a non-empty prompt and max_new_tokens >= 1")
        pfx = None
        if prefix is not None:
            pfx = self._prefixes.get(prefix)
            if pfx is None:
                raise ValueError(f"unknown or released prefix handle {prefix!r}")
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
        req = _Request(rid, prompt, int(max_new_tokens), float(temperature), int(top_k), eos_token_id, gen, blocks,
                       seq_id=("engine", id(self), rid), top_p=float(top_p), min_p=float(min_p),
                       seed=0 if seed is None else int(seed), fused=fused)
        if pfx is not None:
            req.prefix = pfx
            pfx.users += 1
            req.feed = pfx.tokens[whole:] + prompt  # the partly filled page is recomputed per request
            req.history = pfx.tokens + prompt
        else:
            req.feed = prompt
            req.history = list(prompt)
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
                return True
        return False

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
    def _tokens(self, logits, picks):
        """The next token of every ``(request, row of logits)`` in ``picks``: the fused requests
        through one ``ops.sample_logits`` call and one host copy, the others one by one."""
        toks = [None] * len(picks)
        fused = [n for n, (req, _) in enumerate(picks) if req.fused]
        if fused:
            rows = [picks[n][1] for n in fused]
            reqs = [picks[n][0] for n in fused]
            if rows != list(range(logits.shape[0])):
                logits_f = logits[torch.tensor(rows, dtype=torch.long, device=logits.device)]
            else:
                logits_f = logits
            out = ops.sample_logits(logits_f, [r.temperature for r in reqs], [r.top_k for r in reqs],
                                    [r.top_p for r in reqs], [r.min_p for r in reqs], [r.seed for r in reqs],
                                    [r.produced for r in reqs]).tolist()
            for n, tok in zip(fused, out):
                toks[n] = int(tok)
        for n, (req, row) in enumerate(picks):
            if not req.fused:
                toks[n] = int(self._sample(logits[row][None], req.temperature, req.top_k, req.generator)[0])
        return toks

    def _emit(self, req: _Request, tok: int, events) -> bool:
        req.produced += 1
        req.last = tok
        req.history.append(tok)
        finished = req.produced >= req.max_new_tokens or (req.eos_token_id is not None and tok == req.eos_token_id)
        events.append((req.rid, tok, finished))
        return finished

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
        ``call(token lists, cache, seq_ids)`` gives one logits row per item. A request whose prompt
        is now cached emits its first token and retires or stays; returns the ids of those that
        stay. If the call fails it cached nothing (it is all or nothing): its requests go back to
        the head of the queue in arrival order, so no slot decodes a sequence that was never
        prefilled."""
        try:
            logits = call([t for _, _, t in items], self.cache, [o.seq_id for _, o, _ in items])
        except Exception:
            self._requeue([slot for slot, _, _ in items if slot is not None])
            raise
        done, emit = set(), []
        for i, (slot, obj, toks) in enumerate(items):
            obj.fed += len(toks)
            if slot is not None and obj.fed >= len(obj.feed):
                emit.append((slot, obj, i))
        for (slot, obj, _), tok in zip(emit, self._tokens(logits, [(obj, i) for _, obj, i in emit])):
            obj.prefilling = False
            self._unhold_prefix(obj)
            if self._emit(obj, tok, events):
                self._retire(slot)
            else:
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
                self._feed(lambda toks, cache, ids: self.model.prefill(toks, None, cache, ids), plain, events)
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
        """One decode step over the slots; requests still in their prompt, or that left it through
        ``extend`` in this step (``joined``), ride along as inactive slots."""
        live = [r is not None and not r.prefilling and r.rid not in joined for r in self.slots]
        if any(live) and self._proposer is not None:
            drafts = {slot: draft_for(self._proposer, self.num_draft, r.history, r.produced, r.max_new_tokens)
                      for slot, r in enumerate(self.slots) if live[slot]}
            if any(drafts.values()):
                return self._verify(drafts, events)
        if any(live):
            seq_ids = [r.seq_id if on else None for r, on in zip(self.slots, live)]
            tokens = [r.last if on else 0 for r, on in zip(self.slots, live)]
            logits = self.model.decode_step(tokens, self.cache, seq_ids)
            picks = [(req, slot) for slot, req in enumerate(self.slots) if live[slot]]
            for (req, slot), tok in zip(picks, self._tokens(logits, picks)):
                if self._emit(req, tok, events):
                    self._retire(slot)

    def _verify(self, drafts, events):
        """One verify step over the live slots (``drafts``: slot -> draft, possibly empty): feed
        ``[last] + draft`` per slot through one ``extend``, draw every row's token with the row's
        own parameters at step ``produced + j`` in one sampler call, emit the accepted prefix and
        the token after it, and roll the rejected drafts back.

        Admission arithmetic is untouched: ``draft_for`` caps a draft at ``max_new_tokens -
        produced - 1`` tokens, so the cached length stays below prompt + ``max_new_tokens``, which
        is what the request's blocks were reserved for; the extend cannot run out of blocks."""
        slots = sorted(drafts)
        reqs = [self.slots[s] for s in slots]
        rows = [[r.last] + drafts[s] for s, r in zip(slots, reqs)]
        logits = self.model.extend(rows, self.cache, [r.seq_id for r in reqs], all_logits=True, num_splits=None)
        per_row = [(r, j) for r, row in zip(reqs, rows) for j in range(len(row))]
        sampled = ops.sample_logits(logits, [r.temperature for r, _ in per_row], [r.top_k for r, _ in per_row],
                                    [r.top_p for r, _ in per_row], [r.min_p for r, _ in per_row],
                                    [r.seed for r, _ in per_row], [r.produced + j for r, j in per_row]).tolist()
        self.spec_stats["verify_steps"] += 1
        at = 0
        for slot, req, row in zip(slots, reqs, rows):
            draft = drafts[slot]
            toks = accept(draft, sampled[at: at + len(row)], req.max_new_tokens - req.produced, req.eos_token_id)
            at += len(row)
            self.spec_stats["drafted"] += len(draft)
            self.spec_stats["accepted"] += len(toks) - 1
            self.spec_stats["emitted"] += len(toks)
            finished = False
            for tok in toks:  # consecutive events of one request; only the last can finish it
                finished = self._emit(req, tok, events)
            if finished:
                self._retire(slot)
            else:
                self.cache.rollback(req.seq_id, len(draft) - (len(toks) - 1))  # the accepted drafts stay cached

    def step(self) -> List[Tuple[int, int, bool]]:
        """Admit, prefill, decode once, retire. Returns ``(request_id, token, finished)`` for every
        token produced in this step, in production order."""
        events: List[Tuple[int, int, bool]] = []
        self._admit()
        self._decode(self._prefill(events), events)
        return events
