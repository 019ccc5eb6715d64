"""Speculative decoding on the CPU reference path (llama3-tiny, fp32): the n-gram proposer,
``Llama.extend(all_logits=True)``, and the property that a request's stream with ``speculative``
set equals its stream with ``speculative=None, fused_sampling=True``.

The equality needs ``extend`` and ``decode_step`` to agree on every decision. They compute the same
logits by different reductions, about 1e-6 apart in fp32, so the test data keeps every decision of
the plain streams at least ``MARGIN`` = 1e-3 from flipping (``test_plain_streams_keep_their_margins``:
a condition on the data, checked with no step exempted, not a measurement of the code under test):
greedy steps by their top-2 logit gap, sampled steps by the distance of the step's uniform from
both edges of the chosen token's CDF interval under ``sample_kept_ref``. The model's lm_head is
scaled by ``LOGIT_SCALE`` so that next-token distributions are peaked: the unscaled random
llama3-tiny is nearly uniform over its 1024 tokens, where no CDF interval is even 2e-3 wide.
Prompts and the sampling seed were chosen on the CPU so that this holds; smallest margins of the
data below: greedy 7.3e-3 (logit units), sampled 1.1e-3 (CDF units).
"""
import functools
import math

import pytest
import torch

from ray_community_amd.models import GenerationEngine, NgramProposer, PagedKVCache, build_llama
from ray_community_amd.ops import reference as ref

MARGIN = 1e-3
LOGIT_SCALE = 12.0
N_NEW = 24
K = 4
V = 1024
MODES = {"greedy": dict(temperature=0.0, top_p=1.0, seed=0), "sampled": dict(temperature=0.9, top_p=0.9, seed=8)}


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    m = build_llama("llama3-tiny", dtype=torch.float32).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(LOGIT_SCALE)
    return m


def _rand(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (n,), generator=g).tolist()


def _repeats(n, seed, span=6):
    spans = [_rand(span, seed + i) for i in range(3)]
    order = _rand(n // span + 1, seed + 9)
    return [t for o in order for t in spans[o % 3]][:n]


PROMPTS = (tuple(_rand(7, 11)), tuple(_rand(40, 12)), tuple(_repeats(130, 13)))


@functools.lru_cache(maxsize=None)
def _plain(mode):
    """The reference streams: ``generate(speculative=None, fused_sampling=True)``."""
    return _model().generate([list(p) for p in PROMPTS], N_NEW, fused_sampling=True, **MODES[mode])


# ------------------------------------------------------------------------------ scripted proposers
class Scripted:
    """Drafts from the known plain continuation of whichever prompt the history starts with;
    ``wrong(call, j, k)`` says which draft positions to spoil."""

    def __init__(self, streams, prompts=PROMPTS, num_draft=K, wrong=lambda call, j, k: False):
        self.num_draft, self.wrong, self.calls = num_draft, wrong, 0
        self.full = [list(p) + list(s) for p, s in zip(prompts, streams)]
        self.plen = [len(p) for p in prompts]

    def propose(self, history, k):
        full = next(f for f, n in zip(self.full, self.plen) if history[:n] == f[:n])
        assert history == full[: len(history)], "the speculative stream left the plain one"
        draft = full[len(history): len(history) + k]
        out = [(t + 1) % V if self.wrong(self.calls, j, k) else t for j, t in enumerate(draft)]
        self.calls += 1
        return out


def _proposers(mode):
    plain = _plain(mode)
    return {"oracle": lambda: Scripted(plain),
            "always_wrong": lambda: Scripted(plain, wrong=lambda call, j, k: True),
            "wrong_in_turn": lambda: Scripted(plain, wrong=lambda call, j, k: j == (0, 1, k - 1)[call % 3]),
            "ngram": lambda: NgramProposer(K)}


# ------------------------------------------------------------------------------------ the proposer
def test_ngram_proposer():
    p = NgramProposer(num_draft=4, max_ngram=3, min_ngram=1)
    assert p.propose([1, 2, 3, 4, 5], 4) == []                          # no match
    assert p.propose([1, 2, 3, 9, 8, 3, 7, 1, 2, 3], 4) == [9, 8, 3, 7]  # longest n beats the more recent 1-gram
    assert p.propose([5, 6, 1, 0, 5, 6, 2, 0, 5, 6], 1) == [2]           # most recent among equal n
    assert p.propose([1, 2, 3, 4, 5, 6, 7, 1, 2], 3) == [3, 4, 5]        # cut by k
    assert p.propose([1, 2, 3, 4, 1, 2], 4) == [3, 4, 1, 2]              # runs to the end of the history
    assert p.propose([7, 7, 7], 4) == [7]                                # overlap with the suffix; cut by the end
    assert p.propose([1, 2, 1, 2], 0) == []                              # k = 0
    assert p.propose([], 4) == [] and p.propose([3], 4) == []            # nothing earlier to match
    assert NgramProposer(4, max_ngram=3, min_ngram=2).propose([1, 5, 1], 4) == []  # only a 1-gram matches
    assert NgramProposer(4, max_ngram=3, min_ngram=3).propose([1, 1], 4) == []     # shorter than min_ngram
    h = [1, 2, 3, 1, 2]
    assert p.propose(h, 2) == p.propose(h, 2) == [3, 1] and h == [1, 2, 3, 1, 2]   # stateless, input untouched
    for bad in (dict(num_draft=0), dict(min_ngram=0), dict(max_ngram=1, min_ngram=2)):
        with pytest.raises(ValueError):
            NgramProposer(**bad)


# --------------------------------------------------------------------------------- all_logits
def test_extend_all_logits():
    m = _model()
    prior = [_rand(n, 20 + n) for n in (3, 20, 33)]
    new = [_rand(n, 40 + n) for n in (5, 1, 18)]
    ids = ["a", "b", "c"]

    def prepared():
        cache = PagedKVCache(m.cfg, 24, 16, dtype=torch.float32)
        m.extend(prior, cache, ids)
        return cache

    every = m.extend(new, prepared(), ids, all_logits=True)
    assert tuple(every.shape) == (sum(len(r) for r in new), V)
    last = torch.tensor([4, 5, 23])
    # the same hidden rows through an lm_head GEMM of 3 rows instead of 24: equal up to fp32 summation order
    assert (every[last] - m.extend(new, prepared(), ids)).abs().max().item() < 1e-4
    cache = prepared()
    at = 0
    for b, row in enumerate(new):
        for tok in row:
            one = m.decode_step([tok], cache, [ids[b]])[0]
            assert (one - every[at]).abs().max().item() < 1e-4
            at += 1


# ------------------------------------------------------------------------------ the margin condition
def test_plain_streams_keep_their_margins():
    m = _model()
    smallest = {}
    for mode, prm in MODES.items():
        worst = math.inf
        for prompt, stream in zip(PROMPTS, _plain(mode)):
            assert len(stream) == N_NEW
            with torch.no_grad():
                logits = m(torch.tensor([list(prompt) + stream]))[0]
            for i, tok in enumerate(stream):
                x = logits[len(prompt) - 1 + i]
                if prm["temperature"] == 0:
                    top = x.topk(2)
                    assert int(top.indices[0]) == tok
                    margin = (top.values[0] - top.values[1]).item()
                else:
                    w, keep = ref.sample_kept_ref(x, prm["temperature"], 0, prm["top_p"], 0.0)
                    w = w * keep
                    cdf = w.cumsum(0) / w.sum()
                    u = ref.philox_uniforms([prm["seed"]], [i])[0].item()
                    assert keep[tok]
                    margin = min(u - (cdf[tok] - w[tok] / w.sum()).item(), cdf[tok].item() - u)
                assert margin >= MARGIN, (mode, len(prompt), i, margin)
                worst = min(worst, margin)
        smallest[mode] = worst
    print("smallest margins:", smallest)


# ------------------------------------------------------------------------------- stream equality
def _spec_generate(mode, proposer):
    m = _model()
    out = m.generate([list(p) for p in PROMPTS], N_NEW, speculative=proposer, **MODES[mode])
    return out, dict(m.spec_stats)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["oracle", "always_wrong", "wrong_in_turn", "ngram"])
def test_generate_stream_equality(mode, name):
    got, st = _spec_generate(mode, _proposers(mode)[name]())
    assert got == _plain(mode)
    assert st["accepted"] <= st["drafted"]
    if name in ("oracle", "always_wrong"):  # the sequences advance in lockstep: every verify step has all rows
        assert st["emitted"] == st["accepted"] + len(PROMPTS) * st["verify_steps"]
    if name == "oracle":
        assert st["verify_steps"] == math.ceil((N_NEW - 1) / (K + 1)) and st["accepted"] == st["drafted"] > 0
    if name == "always_wrong":
        # one token per verify step; the first token comes from the prompt and the last from a plain
        # decode step (no room left for a draft)
        assert st["accepted"] == 0 and st["verify_steps"] == N_NEW - 2 and st["emitted"] == len(PROMPTS) * (N_NEW - 2)
    if name == "wrong_in_turn":
        assert 0 < st["accepted"] < st["drafted"]


def _engine(speculative=None, prompts=PROMPTS, **kw):
    kw.setdefault("num_blocks", 64)
    return GenerationEngine(_model(), max_slots=4, fused_sampling=True, speculative=speculative, **kw)


def _drain(eng, check_events=True):
    streams, steps = {}, []
    while eng.has_work():
        ev = eng.step()
        steps.append(ev)
        runs = []  # [rid, length] of every run of consecutive events of one request
        for rid, tok, fin in ev:
            streams.setdefault(rid, []).append(tok)
            if runs and runs[-1][0] == rid:
                runs[-1][1] += 1
            else:
                runs.append([rid, 1])
        if check_events:
            for rid in {r for r, _ in runs}:
                mine = [n for r, n in runs if r == rid]
                # the decode phase's tokens are consecutive; a request that left its prompt through
                # ``prefill`` in this step has that one token earlier in the step
                assert len(mine) == 1 or (len(mine) == 2 and mine[0] == 1), runs
                flags = [fin for r, _, fin in ev if r == rid]
                assert not any(flags[:-1]), "finished is set on a request's last token only"
    return streams, steps


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["oracle", "always_wrong", "wrong_in_turn", "ngram"])
def test_engine_stream_equality(mode, name):
    prm = MODES[mode]
    eng = _engine(_proposers(mode)[name]())
    rids = [eng.add_request(list(p), N_NEW, temperature=prm["temperature"], top_p=prm["top_p"], seed=prm["seed"])
            for p in PROMPTS]
    streams, _ = _drain(eng)
    assert [streams[r] for r in rids] == _plain(mode)
    st = eng.spec_stats
    assert set(st) == {"verify_steps", "drafted", "accepted", "emitted"} and st["accepted"] <= st["drafted"]
    if name == "oracle":
        assert st["verify_steps"] == math.ceil((N_NEW - 1) / (K + 1)) and st["accepted"] == st["drafted"] > 0
    if name == "always_wrong":
        assert st["accepted"] == 0 and st["emitted"] == len(PROMPTS) * (N_NEW - 2) == len(PROMPTS) * st["verify_steps"]
    assert eng.cache.num_free_blocks == 64


def test_int_speculative_is_prompt_lookup():
    got, _ = _spec_generate("greedy", K)
    assert got == _plain("greedy")
    eng = _engine(K)
    assert isinstance(eng._proposer, NgramProposer) and eng.num_draft == K and eng.fused_sampling
    for bad in (0, -1, "ngram", object()):
        with pytest.raises(ValueError):
            _engine(bad)
        with pytest.raises(ValueError):
            _model().generate([[1, 2]], 4, speculative=bad)


# ---------------------------------------------------------------------------------------- engine
def test_engine_mixed_batch_tight_cache(monkeypatch):
    """Greedy and sampled requests, one behind a registered prefix, all through chunked prefill,
    in a cache of exactly the blocks admission demands; the stream of each equals its plain one."""
    page = 16
    prefix, suffix = list(PROMPTS[1][:24]), list(PROMPTS[1][24:])
    reqs = [dict(prompt=list(PROMPTS[0]), **MODES["greedy"]), dict(prompt=list(PROMPTS[2]), **MODES["sampled"]),
            dict(prompt=suffix, prefix=True, **MODES["greedy"]), dict(prompt=list(PROMPTS[0]), **MODES["sampled"])]
    blocks = -(-len(prefix) // page)
    for r in reqs:
        total = len(r["prompt"]) + N_NEW + (len(prefix) if r.get("prefix") else 0)
        blocks += -(-total // page) - (len(prefix) // page if r.get("prefix") else 0)
    plain = {"greedy": _plain("greedy"), "sampled": _plain("sampled")}
    want = [plain["greedy"][0], plain["sampled"][2], plain["greedy"][1], plain["sampled"][0]]

    class Both:  # the oracle of whichever mode the history follows
        num_draft = K

        def __init__(self):
            self.by_mode = [Scripted(plain[m]) for m in ("greedy", "sampled")]

        def propose(self, history, k):
            for s in self.by_mode:
                try:
                    return s.propose(history, k)
                except AssertionError:
                    pass
            raise AssertionError("the speculative stream left both plain ones")

    rows = []
    m = _model()
    eng = GenerationEngine(m, max_slots=4, num_blocks=blocks, page_size=page, prefill_chunk=16, speculative=Both())
    real = type(m).extend

    def spy(self, tokens, cache, seq_ids, all_logits=False, num_splits=1):
        if all_logits:
            rows.append(len(tokens))
        return real(self, tokens, cache, seq_ids, all_logits=all_logits, num_splits=num_splits)

    monkeypatch.setattr(type(m), "extend", spy)
    handle = eng.register_prefix(prefix)
    rids = [eng.add_request(r["prompt"], N_NEW, temperature=r["temperature"], top_p=r["top_p"], seed=r["seed"],
                            prefix=handle if r.get("prefix") else None) for r in reqs]
    streams, _ = _drain(eng)  # must not raise KVCacheFull
    assert [streams[r] for r in rids] == want
    eng.release_prefix(handle)
    assert eng.cache.num_free_blocks == blocks
    st = eng.spec_stats
    assert st["verify_steps"] == len(rows) > 0
    assert st["emitted"] == st["accepted"] + sum(rows) and st["accepted"] <= st["drafted"]


def test_engine_eos_inside_accepted_run_and_exact_length():
    plain = _plain("greedy")[1]
    e = next(i for i in range(2, K + 1) if plain[i] not in plain[:i])  # inside the first verify step's draft
    eng = _engine(Scripted(_plain("greedy")))
    a = eng.add_request(list(PROMPTS[1]), N_NEW, eos_token_id=plain[e])
    b = eng.add_request(list(PROMPTS[0]), N_NEW - 1)  # 22 after the first = 4 * 5 + 2: a full draft would overshoot
    streams, steps = _drain(eng)
    assert streams[a] == plain[: e + 1]
    assert streams[b] == _plain("greedy")[0][: N_NEW - 1]
    last = [ev for ev in steps if any(r == a for r, _, _ in ev)][-1]
    assert [fin for r, _, fin in last if r == a][-1] is True
    assert eng.cache.num_free_blocks == 64 and not eng.has_work()


def test_engine_cancel_between_steps():
    eng = _engine(Scripted(_plain("greedy")))
    a = eng.add_request(list(PROMPTS[1]), N_NEW)
    b = eng.add_request(list(PROMPTS[0]), N_NEW)
    got = {a: [], b: []}
    for _ in range(2):
        for rid, tok, _ in eng.step():
            got[rid].append(tok)
    assert eng.cancel(a) and not eng.cancel(a)
    while eng.has_work():
        for rid, tok, _ in eng.step():
            assert rid == b
            got[rid].append(tok)
    assert got[a] == _plain("greedy")[1][: len(got[a])] and 0 < len(got[a]) < N_NEW
    assert got[b] == _plain("greedy")[0]
    assert eng.cache.num_free_blocks == 64


# -------------------------------------------------------------------------------------- defaults
def test_defaults_never_extend_in_the_decode_phase(monkeypatch):
    m = _model()
    calls = []
    real = type(m).extend
    monkeypatch.setattr(type(m), "extend", lambda self, *a, **kw: calls.append(1) or real(self, *a, **kw))
    assert m.generate([list(p) for p in PROMPTS], N_NEW, fused_sampling=True) == _plain("greedy")
    eng = _engine(None)
    for p in PROMPTS:
        eng.add_request(list(p), 6)
    _drain(eng)
    assert calls == [] and eng.spec_stats == {"verify_steps": 0, "drafted": 0, "accepted": 0, "emitted": 0}
    m.generate([list(PROMPTS[2])], 6, speculative=K)
    assert calls  # the spy does see a verify step
