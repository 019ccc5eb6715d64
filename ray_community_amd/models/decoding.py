"""The decode phase of Llama generation, shared by ``Llama.generate`` and ``GenerationEngine``:
a request's sampling parameters (``Sampling``), its decode state (``Stream``), the sampler choice
(``sample_rows``) and one decode round over a fixed set of slots (``decode_round``), plain or
speculative (``models/speculative.py``). The callers keep their own prompt phase, and free or
retire what a round finishes.
"""
from __future__ import annotations

from dataclasses import dataclass, field
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


def use_fused_sampling(fused_sampling, top_p, min_p, repetition_penalty=1.0, presence_penalty=0.0,
                       frequency_penalty=0.0, logprobs=None) -> bool:
    """Whether a request samples through ``ops.sample_logits``: on demand, or because it sets
    ``top_p`` or ``min_p``, which only that sampler implements, a non-neutral penalty
    (``ops.penalize_logits``) or ``logprobs`` (``ops.token_logprobs``), which sit next to it.
    Out-of-range values also go there, to be refused by its checks."""
    return (bool(fused_sampling) or not float(top_p) == 1.0 or not float(min_p) == 0.0 or logprobs is not None
            or not float(repetition_penalty) == 1.0 or not float(presence_penalty) == 0.0
            or not float(frequency_penalty) == 0.0)


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
    nowhere else (``temperature`` and ``top_k`` only for the batched sampler, which has the rules).

    ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` (``ops.penalize_logits``;
    1 / 0 / 0 are neutral) act on the logits before the draw; ``logprobs``: ``None`` is off, an int
    in 0..20 records every produced token's log-probability and that many alternatives
    (``ops.token_logprobs``). Either puts the request on the batched sampler."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    seed: Optional[int] = 0
    fused: bool = False
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logprobs: Optional[int] = None

    def __post_init__(self):
        lp = self.logprobs
        if lp is not None and (isinstance(lp, bool) or not isinstance(lp, int) or not 0 <= lp <= ops.LOGPROBS_MAX_TOP):
            raise ValueError(f"logprobs must be None or an int in 0..{ops.LOGPROBS_MAX_TOP}, got {lp!r}")
        try:
            pen = [float(self.repetition_penalty), float(self.presence_penalty), float(self.frequency_penalty)]
        except (TypeError, ValueError):
            raise ValueError("repetition_penalty, presence_penalty and frequency_penalty must be numbers") from None
        ops.check_penalty_params(*([v] for v in pen))
        fused = use_fused_sampling(self.fused, self.top_p, self.min_p, *pen, lp)
        for name, value in (("temperature", float(self.temperature)), ("top_k", int(self.top_k)),
                            ("top_p", float(self.top_p)), ("min_p", float(self.min_p)),
                            ("seed", int(self.seed or 0)), ("fused", fused), ("repetition_penalty", pen[0]),
                            ("presence_penalty", pen[1]), ("frequency_penalty", pen[2])):
            object.__setattr__(self, name, value)
        ops.check_sampling_params([self.temperature] if fused else [], [self.top_k] if fused else [],
                                  [self.top_p], [self.min_p])

    @property
    def penalized(self) -> bool:
        return not (self.repetition_penalty == 1.0 and self.presence_penalty == 0.0 and self.frequency_penalty == 0.0)


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
    prompt_len: Optional[int] = None  # tokens of ``history`` that were given (``None``: all it starts with)
    # with ``sampling.logprobs``: ``(token, logprob, [(id, logprob), ...])`` per produced token
    logprobs: List[tuple] = field(default_factory=list)

    def __post_init__(self):
        if self.prompt_len is None:
            self.prompt_len = len(self.history)

    def advance(self, toks) -> bool:
        """Take the tokens of one round, of which only the last can end the stream; whether it did."""
        self.history.extend(toks)
        self.produced += len(toks)
        return self.produced >= self.max_new_tokens or (self.eos_token_id is not None
                                                        and toks[-1] == self.eos_token_id)


def _pack_histories(rows):
    """The flat token buffer and the ``(start, prompt_end, end)`` ranges of ``ops.penalize_logits``
    for ``rows`` ``(stream, step, ahead)``: one region per stream, ``history`` + its longest
    ``ahead``, shared by all rows of that stream."""
    regions, flat, ranges = {}, [], []
    for st, _, ahead in rows:
        reg = regions.get(id(st))
        if reg is None or len(ahead) > reg[1]:
            regions[id(st)] = (st, len(ahead), ahead)
    starts = {}
    for key, (st, _, ahead) in regions.items():
        starts[key] = len(flat)
        flat.extend(st.history)
        flat.extend(ahead)
    for st, _, ahead in rows:
        start = starts[id(st)]
        ranges.append((start, start + st.prompt_len, start + len(st.history) + len(ahead)))
    return flat, ranges


def _sample_fused(logits, rows):
    """The tokens of ``rows`` ``(stream, step, ahead)``, one per row of ``logits``, and their
    logprob entries (``None`` where the stream records none): one ``ops.sample_logits`` call and one
    host copy. ``ahead`` are the draft tokens between the stream's history and the row (``()``
    outside a verify round): a row is penalized over ``history + ahead``, its true history exactly
    when those drafts are accepted.

    If a row has a non-neutral penalty, the histories are packed and uploaded and one
    ``ops.penalize_logits`` call comes first; if a row records logprobs, one ``ops.token_logprobs``
    call on the tensor the sampler was given comes after, and its outputs ride in the host copy.
    Otherwise neither, and nothing else, happens."""
    prm = [st.sampling for st, _, _ in rows]
    if any(p.penalized for p in prm):
        flat, ranges = _pack_histories(rows)
        logits = ops.penalize_logits(logits, flat, ranges, [p.repetition_penalty for p in prm],
                                     [p.presence_penalty for p in prm], [p.frequency_penalty for p in prm])
    toks = ops.sample_logits(logits, [p.temperature for p in prm], [p.top_k for p in prm], [p.top_p for p in prm],
                             [p.min_p for p in prm], [p.seed for p in prm], [step for _, step, _ in rows])
    top_n = max((p.logprobs for p in prm if p.logprobs is not None), default=None)
    if top_n is None:
        return toks.tolist(), [None] * len(rows)
    lp, top_ids, top_lp = ops.token_logprobs(logits, toks, top_n)
    # one copy: ids and fp32 values are exact in float64
    host = torch.cat([toks[:, None].double(), lp[:, None].double(), top_ids.double(), top_lp.double()], dim=1).tolist()
    out, entries = [], []
    for p, r in zip(prm, host):
        out.append(int(r[0]))
        entries.append(None if p.logprobs is None else
                       (int(r[0]), r[1], [(int(i), v) for i, v in zip(r[2: 2 + p.logprobs],
                                                                       r[2 + top_n: 2 + top_n + p.logprobs])
                                        if i >= 0]))   # a vocabulary below ``logprobs`` entries has no more
    return out, entries


def sample_rows(logits, picks):
    """The next token of every ``(stream, row of logits)`` in ``picks``: the fused streams through
    one ``ops.sample_logits`` call and one host copy, the others one by one with their generators.
    A stream that records logprobs gets its entry appended: every caller emits exactly these tokens."""
    toks = [None] * len(picks)
    fused = [n for n, (st, _) in enumerate(picks) if st.sampling.fused]
    if fused:
        rows = [picks[n][1] for n in fused]
        sub = logits if rows == list(range(logits.shape[0])) else logits[torch.tensor(rows, device=logits.device)]
        got, entries = _sample_fused(sub, [(picks[n][0], picks[n][0].produced, ()) for n in fused])
        for n, tok, entry in zip(fused, got, entries):
            toks[n] = int(tok)
            if entry is not None:
                picks[n][0].logprobs.append(entry)
    for n, (st, row) in enumerate(picks):
        if not st.sampling.fused:
            prm = st.sampling
            toks[n] = int(sample_tokens(logits[row][None], prm.temperature, prm.top_k, st.generator)[0])
    return toks


def decode_round(model, cache, slots, proposer, num_draft, stats, sample=sample_rows, *, runner=None):
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
    ``decode_step``, one per sequence of ``extend``); otherwise the keyword is not passed at all.

    ``runner`` (a ``models.decode_graph.DecodeRunner`` over ``model``, ``cache`` and ``len(slots)``
    rows; ``graph_decode=True`` of the callers): its ``step`` takes the place of ``decode_step``. It
    runs a LoRA round through ``decode_step`` itself, and a verify round goes through ``extend`` as
    ever; the runner counts both as eager fallbacks."""
    live = [s for s, st in enumerate(slots) if st is not None]
    if not live:
        return []
    drafts = [draft_for(proposer, num_draft, slots[s].history, slots[s].produced, slots[s].max_new_tokens)
              if proposer is not None else [] for s in live]
    lora = any(slots[s].adapter is not None for s in live)
    if not any(drafts):
        akw = {"adapters": [st.adapter if st is not None else None for st in slots]} if lora else {}
        toks_in = [st.history[-1] if st is not None else 0 for st in slots]
        ids = [st.seq_id if st is not None else None for st in slots]
        if runner is not None:
            logits = runner.step(toks_in, ids, **akw)
        else:
            logits = model.decode_step(toks_in, cache, ids, **akw)
        toks = sample(logits, [(slots[s], s) for s in live])
        return [(s, [tok], slots[s].advance([tok])) for s, tok in zip(live, toks)]
    rows = [[slots[s].history[-1]] + draft for s, draft in zip(live, drafts)]
    akw = {"adapters": [slots[s].adapter for s in live]} if lora else {}
    if runner is not None:
        runner.count_fallback()
    logits = model.extend(rows, cache, [slots[s].seq_id for s in live], all_logits=True, num_splits=None, **akw)
    sampled, entries = _sample_fused(logits, [(slots[s], slots[s].produced + j, row[1: 1 + j])
                                              for s, row in zip(live, rows) for j in range(len(row))])
    stats["verify_steps"] += 1
    out, at = [], 0
    for s, draft in zip(live, drafts):
        st = slots[s]
        toks = accept(draft, sampled[at: at + len(draft) + 1], st.max_new_tokens - st.produced, st.eos_token_id)
        if st.sampling.logprobs is not None:  # row j drew emitted token j: an accepted draft or the one after
            st.logprobs.extend(entries[at: at + len(toks)])
        at += len(draft) + 1
        stats["drafted"] += len(draft)
        stats["accepted"] += len(toks) - 1
        stats["emitted"] += len(toks)
        out.append((s, toks, st.advance(toks)))
        if not out[-1][2]:
            cache.rollback(st.seq_id, len(draft) - (len(toks) - 1))  # exactly the accepted drafts stay cached
    return out
