"""The decode round that ``Llama.generate`` and ``GenerationEngine`` share (``models/decoding.py``),
on the CPU reference path with the model, prompts and plain streams of ``test_speculative_cpu``:
both callers make the same model and sampler calls, the ``sample_tokens`` path of ``generate`` still
draws every step's whole logits tensor at once, and ``Sampling`` is where values are refused."""
import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, PagedKVCache, build_llama, decoding
from ray_community_amd.models.decoding import Sampling
from test_speculative_cpu import MODES, PROMPTS, V, Scripted, _model, _plain

N_NEW = 12


# --------------------------------------------------------------------------------- call traces
def _traced(monkeypatch, run):
    """What ``run()`` returns, and the model and sampler calls it made: method, token lists,
    which sequences are inactive (``None``), keyword arguments; for the sampler the row count and
    every per-row parameter list."""
    m, trace, real_sample = _model(), [], ops.sample_logits

    def spy(name, real, ntok):
        def wrapper(self, *a, **kw):
            tokens = a[0].tolist() if torch.is_tensor(a[0]) else [list(t) if isinstance(t, (list, tuple)) else int(t)
                                                                   for t in a[0]]
            trace.append((name, tokens, [s is None for s in a[-1]], a[1:ntok], kw))
            return real(self, *a, **kw)
        return wrapper

    def sample(logits, *a, **kw):
        trace.append(("sample_logits", logits.shape[0], a, kw))
        return real_sample(logits, *a, **kw)

    with monkeypatch.context() as patch:
        for name, ntok in (("prefill", 2), ("decode_step", 1), ("extend", 1)):  # prefill: tokens, lengths
            patch.setattr(type(m), name, spy(name, getattr(type(m), name), ntok))
        patch.setattr(ops, "sample_logits", sample)
        return run(), trace


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("speculative", [False, True])
def test_generate_and_engine_make_the_same_calls(monkeypatch, mode, speculative):
    prm, plain = MODES[mode], _plain(mode)
    prompts = [list(p) for p in PROMPTS]
    eos = None
    if speculative:  # an EOS inside the shortest prompt's stream: the last token new to it before its end
        e = max(i for i in range(N_NEW - 1) if plain[0][i] not in plain[0][:i])
        eos = plain[0][e]

    def proposer():
        if not speculative:
            return None
        return Scripted(plain, wrong=lambda call, j, k: j == (0, 1, k - 1)[call % 3])  # wrong_in_turn

    def by_generate():
        m = _model()
        out = m.generate(prompts, N_NEW, eos_token_id=eos, speculative=proposer(), fused_sampling=True, **prm)
        return out, dict(m.spec_stats) if speculative else None

    def by_engine():
        eng = GenerationEngine(_model(), max_slots=3, num_blocks=64, fused_sampling=True, speculative=proposer())
        rids = [eng.add_request(p, N_NEW, eos_token_id=eos, **prm) for p in prompts]
        out = {}
        while eng.has_work():
            for rid, tok, _ in eng.step():
                out.setdefault(rid, []).append(tok)
        assert eng.cache.num_free_blocks == 64
        return [out[r] for r in rids], dict(eng.spec_stats) if speculative else None

    (got_g, stats_g), trace_g = _traced(monkeypatch, by_generate)
    (got_e, stats_e), trace_e = _traced(monkeypatch, by_engine)
    want = [s[:N_NEW] for s in plain]
    if speculative:
        want = [s[: s.index(eos) + 1] if eos in s else s for s in want]
        assert len(want[0]) == e + 1 < N_NEW
    assert got_g == want and got_e == want
    assert trace_g[0][0] == "prefill" and len(trace_g[0][1]) == 3    # all admitted in the first step
    assert len(trace_g) == len(trace_e)
    for n, (a, b) in enumerate(zip(trace_g, trace_e)):
        assert a == b, (n, a, b)
    verifies = [t for t in trace_g if t[0] == "extend"]
    if speculative:
        assert stats_g == stats_e and 0 < stats_g["accepted"] < stats_g["drafted"]
        assert len(verifies) == stats_g["verify_steps"] > 0
        assert all(t[4] == dict(all_logits=True, num_splits=None) for t in verifies)
        # the rounds after the EOS run without the shortest stream
        assert any(any(t[2]) for t in trace_g if t[0] == "decode_step") or any(len(t[1]) < 3 for t in verifies)
    else:
        assert not verifies and [t[0] for t in trace_g[:3]] == ["prefill", "sample_logits", "decode_step"]


# ------------------------------------------------------------------------------ legacy sampling
def test_generate_legacy_sampling_draws_the_whole_tensor(monkeypatch):
    torch.manual_seed(0)
    m = build_llama("llama3-tiny", dtype=torch.float32).eval()
    prompts, n, T, K, seed = [[5, 9, 2, 7], [11, 3, 8, 1, 4, 6]], 8, 0.8, 20, 3
    real = decoding.sample_tokens

    def by_hand(eos):
        """The loop ``generate`` has always run on this path: one ``sample_tokens`` over all rows
        of each step's logits, finished rows included, on one generator."""
        cache = PagedKVCache(m.cfg, 8, 16, dtype=torch.float32)
        gen = torch.Generator().manual_seed(seed)
        ids, out = ["a", "b"], [[], []]
        logits = m.prefill(prompts, None, cache, ids)
        for step in range(n):
            nxt = real(logits, T, K, gen).tolist()
            for b in range(2):
                if ids[b] is not None:
                    out[b].append(nxt[b])
                    if nxt[b] == eos:
                        cache.free(ids[b])
                        ids[b] = None
            if step + 1 == n or ids == [None, None]:
                break
            logits = m.decode_step([t if s is not None else 0 for t, s in zip(nxt, ids)], cache, ids)
        return out

    base = by_hand(None)
    e = next(i for i in range(2, n - 2) if base[0][i] not in base[0][:i] and base[0][i] not in base[1])
    eos = base[0][e]
    want = by_hand(eos)
    assert want[0] == base[0][: e + 1] and len(want[1]) == n

    shapes, fused = [], []
    monkeypatch.setattr(decoding, "sample_tokens", lambda logits, *a, **kw: shapes.append(tuple(logits.shape))
                        or real(logits, *a, **kw))
    monkeypatch.setattr(ops, "sample_logits", lambda *a, **kw: fused.append(1))
    assert m.generate(prompts, n, temperature=T, top_k=K, seed=seed, eos_token_id=eos) == want
    assert shapes == [(2, V)] * n and fused == []   # one draw per step, never a [1, V] one, never the op


# ----------------------------------------------------------------------------------- validation
REFUSED = [("top_p", dict(top_p=0.0), False), ("min_p", dict(min_p=1.5), False), ("top_k", dict(top_k=-1), True)]


@pytest.mark.parametrize("name,kw,fused", REFUSED)
def test_sampling_refuses_what_generate_and_add_request_refuse(name, kw, fused):
    m = _model()
    with pytest.raises(ValueError, match=name):
        Sampling(temperature=1.0, fused=fused, **kw)
    with pytest.raises(ValueError, match=name):
        m.generate([[1, 2, 3]], 2, temperature=1.0, fused_sampling=fused, **kw)
    eng = GenerationEngine(m, max_slots=2, num_blocks=8, fused_sampling=fused)
    with pytest.raises(ValueError, match=name):
        eng.add_request([1, 2, 3], 2, temperature=1.0, **kw)
    assert not eng.has_work()


def test_sampling_normalises():
    s = Sampling(0.5, 3, 0.9, 0.0, None)
    assert (s.temperature, s.top_k, s.top_p, s.min_p, s.seed, s.fused) == (0.5, 3, 0.9, 0.0, 0, True)
    assert not Sampling(0.5, 3, seed=7).fused and Sampling(0.5, 3, seed=7, fused=True).fused
    assert Sampling(min_p=0.1).fused
    Sampling(temperature=1.0, top_k=-1)   # as ever: top_k and temperature are the batched sampler's to check
    with pytest.raises(ValueError, match="temperature"):
        Sampling(temperature=-1.0, fused=True)
    with pytest.raises(Exception):
        s.seed = 1                        # frozen
