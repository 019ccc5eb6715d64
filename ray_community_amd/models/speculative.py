"""Speculative decoding by re-drawing: propose a few draft tokens per sequence on the host, score
them all in one ``Llama.extend`` and keep the prefix the sampler would have produced anyway.

``ops.sample_logits`` makes a token a pure function of ``(seed, step, the row's logits)``, so a
draft is verified by drawing the token of its step from the verify forward's logits: if it equals
the draft, the next row's logits are those the plain loop would have computed, and so on. The
speculative stream is therefore the plain ``fused_sampling`` stream, token for token, for greedy and
for sampled requests, wherever ``extend`` and ``decode_step`` agree on the logits. For a
deterministic proposer this rule is also the optimal one: P(accept) = p_target(draft).

This module holds the host-side pieces (proposer, draft cap, acceptance rule, counters); the verify
round itself is ``decoding.decode_round``, which ``Llama.generate`` and ``GenerationEngine`` share.

A proposer is any object with ``propose(history: List[int], k: int) -> List[int]`` returning at
most ``k`` tokens (possibly none); an optional ``num_draft`` attribute bounds ``k`` (default 4).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

DEFAULT_NUM_DRAFT = 4


class NgramProposer:
    """Prompt lookup: continue the most recent earlier occurrence of the history's last n-gram.

    For ``n`` from ``max_ngram`` down to ``min_ngram``, the last ``n`` tokens of the history are
    searched for their most recent earlier occurrence (one starting before ``len - n``; it may
    overlap the suffix); the tokens that followed it, at most ``k``, are the draft. No match for
    any ``n`` gives no draft. Pure host Python, deterministic, stateless between calls."""

    def __init__(self, num_draft: int = DEFAULT_NUM_DRAFT, max_ngram: int = 3, min_ngram: int = 1):
        if int(num_draft) < 1:
            raise ValueError("num_draft must be >= 1")
        if not 1 <= int(min_ngram) <= int(max_ngram):
            raise ValueError("need 1 <= min_ngram <= max_ngram")
        self.num_draft, self.max_ngram, self.min_ngram = int(num_draft), int(max_ngram), int(min_ngram)

    def propose(self, history: Sequence[int], k: int) -> List[int]:
        history = list(history)
        size = len(history)
        if k <= 0:
            return []
        for n in range(min(self.max_ngram, size - 1), self.min_ngram - 1, -1):
            suffix = history[size - n:]
            for start in range(size - n - 1, -1, -1):
                if history[start: start + n] == suffix:
                    return history[start + n: start + n + k]
        return []


def resolve_speculative(speculative) -> Tuple[Optional[object], int]:
    """``(proposer, num_draft)`` of a ``speculative=`` argument: ``None`` is off, an ``int k >= 1``
    is ``NgramProposer(num_draft=k)``, anything else must have ``propose``."""
    if speculative is None:
        return None, 0
    if isinstance(speculative, int) and not isinstance(speculative, bool):
        if speculative < 1:
            raise ValueError("speculative must be >= 1 draft tokens")
        return NgramProposer(num_draft=speculative), speculative
    if not callable(getattr(speculative, "propose", None)):
        raise ValueError("speculative must be None, a number of draft tokens or an object with propose(history, k)")
    num_draft = int(getattr(speculative, "num_draft", DEFAULT_NUM_DRAFT))
    if num_draft < 1:
        raise ValueError("the proposer's num_draft must be >= 1")
    return speculative, num_draft


def draft_for(proposer, num_draft: int, history: List[int], produced: int, max_new_tokens: int) -> List[int]:
    """The draft of a sequence that has produced ``produced`` of its ``max_new_tokens``: at most
    ``min(num_draft, max_new_tokens - produced - 1)`` tokens. A verify step caches the last token
    and the draft, so this cap keeps the cached length below prompt + max_new_tokens, inside what
    the sequence was sized (and, in the engine, admitted) for."""
    k = min(num_draft, max_new_tokens - produced - 1)
    if k <= 0:
        return []
    return [int(t) for t in proposer.propose(list(history), k)][:k]


def accept(draft: Sequence[int], sampled: Sequence[int], room: int, eos_token_id=None) -> List[int]:
    """The tokens a verify step emits: ``sampled[j]`` is the token drawn from the logits after fed
    row ``j`` (row 0 the last emitted token, row ``j`` draft ``j - 1``). With ``n`` the length of
    the longest prefix with ``sampled[j] == draft[j]`` these are ``sampled[0..n]``, cut after an
    EOS and at ``room`` tokens. When nothing was cut, ``len(result) - 1 == n`` drafts stay cached
    and ``len(draft) - n`` are rolled back; a cut means the sequence is finished."""
    n = 0
    while n < len(draft) and sampled[n] == draft[n]:
        n += 1
    out = []
    for tok in sampled[: n + 1]:
        if len(out) >= room:
            break
        out.append(int(tok))
        if eos_token_id is not None and tok == eos_token_id:
            break
    return out


def new_stats() -> dict:
    return {"verify_steps": 0, "drafted": 0, "accepted": 0, "emitted": 0}
