"""The decode phase of Llama generation, shared by ``Llama.generate`` and ``GenerationEngine``:
a request's sampling parameters (``Sampling``), its decode state (``Stream``), the sampler choice
(``sample_rows``) and one decode round over a fixed set of slots (``decode_round``), plain or
speculative (``models/speculative.py``). The callers keep their own prompt phase, and free or
retire what a round finishes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from .. import ops
from .speculative import accept, draft_for


def _seeded_generator(device, temperature, seed):
    """The generator a request samples with: seeded (0 by default) on ``device``; ``None`` for
    greedy decoding (``temperature == 0``)."""
    if not temperature > 0:
        return None
    gen = torch.Generator(device=device)
    gen.manual_seed(0 if seed is None else int(seed))
    return gen


def use_fused_sampling(fused_sampling, top_p, min_p) -> bool:
    """Whether a request samples through ``ops.sample_logits``: on demand, or because it sets
    ``top_p`` or ``min_p``, which only that sampler implements. Out-of-range values also go there,
    to be refused by its checks."""
    return bool(fused_sampling) or not float(top_p) == 1.0 or not float(min_p) == 0.0


def sample_tokens(logits, temperature: float = 0.0, top_k: int = 0, generator=None):
    """Next token per row of ``logits`` [B, V]: argmax at ``temperature == 0``, else a sample of
    softmax(logits / temperature) restricted to the ``top_k`` largest logits (0: all)."""
    if temperature <= 0:
        return logits.argmax(dim=-1)
    x = logits.float() / float(temperature)
    if top_k and top_k < x.shape[-1]:
        kth = x.topk(int(top_k), dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    return torch.multinomial(torch.softmax(x, dim=-1), 1, generator=generator).reshape(-1)


@dataclass(frozen=True)
class Sampling:
    """How a request draws its tokens. ``fused`` goes in as "the batched sampler was asked for" and
    comes out as ``use_fused_sampling``; ``seed`` ``None`` is 0. The values are checked here and
    nowhere else (``temperature`` and ``top_k`` only for the batched sampler, which has the rules)."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    seed: Optional[int] = 0
    fused: bool = False

    def __post_init__(self):
        fused = use_fused_sampling(self.fused, self.top_p, self.min_p)
        for name, value in (("temperature", float(self.temperature)), ("top_k", int(self.top_k)),
                            ("top_p", float(self.top_p)), ("min_p", float(self.min_p)),
                            ("seed", int(self.seed or 0)), ("fused", fused)):
            object.__setattr__(self, name, value)
        ops.check_sampling_params([self.temperature] if fused else [], [self.top_k] if fused else [],
                                  [self.top_p], [self.min_p])


@dataclass
class Stream:
    """The decode state of one sequence. The batched sampler is stepped by ``produced``, so a
    stream's tokens are a function of its seed and its own logits, never of its slot or its
    neighbours."""
    seq_id: object
    history: List[int]               # prompt + produced tokens: the last one is the next decode input
    max_new_tokens: int
    sampling: Sampling
    eos_token_id: Optional[int] = None
    generator: Optional[torch.Generator] = None   # of the ``sample_tokens`` path
    produced: int = 0
    adapter: Optional[str] = None    # the LoRA adapter of every forward row of this sequence

    def advance(self, toks) -> bool:
        """Take the tokens of one round, of which only the last can end the stream; whether it did."""
        self.history.extend(toks)
        self.produced += len(toks)
        return self.produced >= self.max_new_tokens or (self.eos_token_id is not None
                                                        and toks[-1] == self.eos_token_id)


def _sample_fused(logits, rows):
    """One ``ops.sample_logits`` call and one host copy over ``rows`` ``(stream, step)``, one per
    row of ``logits``."""
    prm = [st.sampling for st, _ in rows]
    return ops.sample_logits(logits, [p.temperature for p in prm], [p.top_k for p in prm], [p.top_p for p in prm],
                             [p.min_p for p in prm], [p.seed for p in prm], [step for _, step in rows]).tolist()


def sample_rows(logits, picks):
    """The next token of every ``(stream, row of logits)`` in ``picks``: the fused streams through
    one ``ops.sample_logits`` call and one host copy, the others one by one with their generators."""
    toks = [None] * len(picks)
    fused = [n for n, (st, _) in enumerate(picks) if st.sampling.fused]
    if fused:
        rows = [picks[n][1] for n in fused]
        sub = logits if rows == list(range(logits.shape[0])) else logits[torch.tensor(rows, device=logits.device)]
        for n, tok in zip(fused, _sample_fused(sub, [(picks[n][0], picks[n][0].produced) for n in fused])):
            toks[n] = int(tok)
    for n, (st, row) in enumerate(picks):
        if not st.sampling.fused:
            prm = st.sampling
            toks[n] = int(sample_tokens(logits[row][None], prm.temperature, prm.top_k, st.generator)[0])
    return toks


def decode_round(model, cache, slots, proposer, num_draft, stats, sample=sample_rows):
    """One decode round over ``slots`` (a ``Stream`` or ``None`` per position); returns ``(slot,
    tokens, finished)`` for every live slot, in slot order, with the streams advanced. What
    finished is the caller's to free.

    If no live stream has a draft this is one ``decode_step`` over all slots (``None`` rides along
    as an inactive row) and one ``sample(logits, [(stream, row)])``. Otherwise it is a verify round:
    ``[last] + draft`` of every live stream through one ``extend``, every row's token drawn with
    the stream's own parameters at step ``produced + j`` in one sampler call, the accepted prefix
    and the token after it emitted, and the rejected drafts rolled back.

    ``draft_for`` caps a draft at ``max_new_tokens - produced - 1`` tokens, so the cached length
    stays below prompt + ``max_new_tokens``, which is what the sequence's blocks were sized (in the
    engine: reserved) for; the extend cannot run out of blocks.

    If some live stream has a LoRA ``adapter``, both calls carry ``adapters=[...]`` (one per row of
    ``decode_step``, one per sequence of ``extend``); otherwise the keyword is not passed at all."""
    live = [s for s, st in enumerate(slots) if st is not None]
    if not live:
        return []
    drafts = [draft_for(proposer, num_draft, slots[s].history, slots[s].produced, slots[s].max_new_tokens)
              if proposer is not None else [] for s in live]
    lora = any(slots[s].adapter is not None for s in live)
    if not any(drafts):
        akw = {"adapters": [st.adapter if st is not None else None for st in slots]} if lora else {}
        logits = model.decode_step([st.history[-1] if st is not None else 0 for st in slots], cache,
                                   [st.seq_id if st is not None else None for st in slots], **akw)
        toks = sample(logits, [(slots[s], s) for s in live])
        return [(s, [tok], slots[s].advance([tok])) for s, tok in zip(live, toks)]
    rows = [[slots[s].history[-1]] + draft for s, draft in zip(live, drafts)]
    akw = {"adapters": [slots[s].adapter for s in live]} if lora else {}
    logits = model.extend(rows, cache, [slots[s].seq_id for s in live], all_logits=True, num_splits=None, **akw)
    sampled = _sample_fused(logits, [(slots[s], slots[s].produced + j) for s, row in zip(live, rows)
                                     for j in range(len(row))])
    stats["verify_steps"] += 1
    out, at = [], 0
    for s, draft in zip(live, drafts):
        st = slots[s]
        toks = accept(draft, sampled[at: at + len(draft) + 1], st.max_new_tokens - st.produced, st.eos_token_id)
        at += len(draft) + 1
        stats["drafted"] += len(draft)
        stats["accepted"] += len(toks) - 1
        stats["emitted"] += len(toks)
        out.append((s, toks, st.advance(toks)))
        if not out[-1][2]:
            cache.rollback(st.seq_id, len(draft) - (len(toks) - 1))  # exactly the accepted drafts stay cached
    return out
