"""Continuous batching for Llama generation: a fixed number of decode slots over one paged cache.

``GenerationEngine.step()`` admits waiting requests (one prefill for the newly admitted ones),
runs one ``decode_step`` over all slots (inactive slots ride along at context length 0) and
retires finished sequences, freeing their blocks. Pure Python over ``PagedKVCache`` and the
``Llama`` inference methods; it runs on whatever device the model is on.
"""
from __future__ import annotations

import itertools
from collections import deque
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from .kv_cache import PagedKVCache


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


class GenerationEngine:
    def __init__(self, model, cache: Optional[PagedKVCache] = None, max_slots: int = 8, num_blocks: int = 256,
                 page_size: int = 16):
        from .llama import sample_tokens

        self.model = model
        w = model.embed.weight
        self.cache = cache if cache is not None else PagedKVCache(model.cfg, num_blocks, page_size, device=w.device,
                                                                  dtype=w.dtype)
        self.slots: List[Optional[_Request]] = [None] * int(max_slots)
        self.waiting = deque()
        self._ids = itertools.count()
        self._sample = sample_tokens

    # -------------------------------------------------------------------------------- requests
    def add_request(self, prompt, max_new_tokens: int, temperature: float = 0.0, top_k: int = 0, eos_token_id=None,
                    seed=None) -> int:
        """Queue a request; returns its id. It is admitted by a later ``step()`` once a slot is
        free and the cache can hold its whole sequence (prompt + ``max_new_tokens``)."""
        prompt = [int(t) for t in prompt]
        if not prompt or max_new_tokens < 1:
            raise ValueError("a request needs a non-empty prompt and max_new_tokens >= 1")
        total = len(prompt) + int(max_new_tokens)
        if total > self.model.cfg.max_seq_len:
            raise ValueError(f"prompt + max_new_tokens = {total} exceeds max_seq_len {self.model.cfg.max_seq_len}")
        padded = -(-len(prompt) // 128) * 128  # what prefill pads the prompt to
        if padded > self.model.cfg.max_seq_len:
            raise ValueError(f"prompt of {len(prompt)} tokens pads to {padded} > max_seq_len "
                             f"{self.model.cfg.max_seq_len}")
        blocks = -(-total // self.cache.page_size)
        if blocks > self.cache.num_blocks:
            raise ValueError(f"request needs {blocks} cache blocks, the cache has {self.cache.num_blocks}")
        gen = None
        if temperature > 0:
            gen = torch.Generator(device=self.model.embed.weight.device)
            gen.manual_seed(0 if seed is None else int(seed))
        rid = next(self._ids)
        self.waiting.append(_Request(rid, prompt, int(max_new_tokens), float(temperature), int(top_k), eos_token_id,
                                     gen, blocks, seq_id=("engine", id(self), rid)))
        return rid

    def cancel(self, request_id: int) -> bool:
        """Drop a request, waiting or active: its slot and cache blocks are free at once and it
        produces no further tokens. Returns False if the request is unknown or already finished."""
        for req in self.waiting:
            if req.rid == request_id:
                self.waiting.remove(req)
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

    def _reserved(self) -> int:
        """Blocks the active requests may still take while they decode."""
        return sum(r.blocks - self.cache.blocks_held(r.seq_id) for r in self.slots if r is not None)

    # ------------------------------------------------------------------------------------ step
    def _emit(self, req: _Request, logits_row, events) -> bool:
        tok = int(self._sample(logits_row[None], req.temperature, req.top_k, req.generator)[0])
        req.produced += 1
        req.last = tok
        finished = req.produced >= req.max_new_tokens or (req.eos_token_id is not None and tok == req.eos_token_id)
        events.append((req.rid, tok, finished))
        return finished

    def _retire(self, slot: int):
        self.cache.free(self.slots[slot].seq_id)
        self.slots[slot] = None

    def step(self) -> List[Tuple[int, int, bool]]:
        """Admit, prefill, decode once, retire. Returns ``(request_id, token, finished)`` for every
        token produced in this step, in production order."""
        events: List[Tuple[int, int, bool]] = []
        # admit in arrival order: a request that does not fit waits (and keeps its place)
        admitted = []
        budget = self.cache.num_free_blocks - self._reserved()
        while self.waiting and None in self.slots and self.waiting[0].blocks <= budget:
            req = self.waiting.popleft()
            budget -= req.blocks
            slot = self.slots.index(None)
            self.slots[slot] = req
            admitted.append(slot)
        if admitted:
            reqs = [self.slots[s] for s in admitted]
            try:
                logits = self.model.prefill([r.prompt for r in reqs], None, self.cache, [r.seq_id for r in reqs])
            except Exception:
                # prefill cached nothing (it is all or nothing): the requests go back to the head of
                # the queue in arrival order, so no slot decodes a sequence that was never prefilled
                for slot in reversed(admitted):
                    self.waiting.appendleft(self.slots[slot])
                    self.slots[slot] = None
                raise
            for i, slot in enumerate(admitted):
                if self._emit(self.slots[slot], logits[i], events):
                    self._retire(slot)
        if any(r is not None for r in self.slots):
            seq_ids = [r.seq_id if r is not None else None for r in self.slots]
            tokens = [r.last if r is not None else 0 for r in self.slots]
            logits = self.model.decode_step(tokens, self.cache, seq_ids)
            for slot, req in enumerate(self.slots):
                if req is not None and self._emit(req, logits[slot], events):
                    self._retire(slot)
        return events
