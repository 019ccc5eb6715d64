"""The batched sampler without a GPU: Philox known answers, ``ops.reference.sample_logits_ref``
against a brute-force float64 oracle (a sort and a Python loop, written here), argument checks,
and the engine's use of ``ops.sample_logits`` (one call per logits tensor, untouched default
streams, independence from batching, greedy equivalence)."""
import functools
import types

import numpy as np
import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, PagedKVCache, build_llama
from ray_community_amd.models.llama import Llama, _seeded_generator, sample_tokens
from ray_community_amd.ops import reference as ref

# counter, key -> output words of Philox4x32-10
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# --------------------------------------------------------------------------------------- Philox
def _uniform_of(word0):
    return ((word0 >> 8) + 0.5) * 2.0 ** -24


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        got = ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter],
                                [np.array([k], dtype=np.uint64) for k in key])
        assert tuple(int(w[0]) for w in got) == want
    # philox_uniforms runs the same rounds at counter (step lo, step hi, 0, 0), key (seed lo, seed hi)
    assert float(ref.philox_uniforms([0], [0])[0]) == _uniform_of(KNOWN[0][2][0])
    seed, step = 0x299f31d0a4093822, 0x85a308d3243f6a88
    word0 = int(ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in (0x243f6a88, 0x85a308d3, 0, 0)],
                                  [np.array([k], dtype=np.uint64) for k in (0xa4093822, 0x299f31d0)])[0][0])
    assert float(ref.philox_uniforms([seed], [step])[0]) == _uniform_of(word0)


def test_philox_uniforms_are_inside_the_unit_interval():
    edge = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1]
    seeds = [s for s in edge for _ in edge] + list(range(1000))
    steps = [s for _ in edge for s in edge] + [7] * 1000
    u = ref.philox_uniforms(seeds, steps)
    assert u.dtype == torch.float64 and u.shape == (len(seeds),)  # 25 significant bits: exact in float64 only
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert float(u.min()) >= 2.0 ** -25 and float(u.max()) <= 1 - 2.0 ** -25
    again = ref.philox_uniforms(torch.tensor(seeds[::-1]), torch.tensor(steps[::-1]))
    assert torch.equal(again.flip(0), u)  # a function of (seed, step) alone
    assert len(set(u[25:].tolist())) > 990


# ------------------------------------------------------------------- reference vs brute force
def _brute(x, t, k, p, mp, u):
    """(token, kept set) of one row by the definition: float64, a sort and loops. ``x``: fp32 logits."""
    xs = [float(v) for v in x]
    V = len(xs)
    if t == 0:
        return xs.index(max(xs)), None
    t32, p32, mp32 = (float(np.float32(v)) for v in (t, p, mp))
    w32 = torch.exp((x.float() - x.float().max()) / torch.tensor(t32))  # the one fp32 step, as specified
    w = [float(v) for v in w32.double()]
    order = sorted(range(V), key=lambda i: -xs[i])
    keep = set(range(V))
    if 0 < k < V:
        keep = {i for i in keep if xs[i] >= xs[order[k - 1]]}
    if p32 < 1:
        surv = [i for i in order if i in keep]
        total = sum(w[i] for i in surv)
        keep &= {i for i in surv if sum(w[j] for j in surv if xs[j] > xs[i]) < p32 * total}
    if mp32 > 0:
        keep = {i for i in keep if float(w32[i]) >= mp32}
    kept = sorted(keep)
    total, run = sum(w[i] for i in kept), 0.0
    for i in kept:
        run += w[i]
        if run > u * total:
            return i, keep
    return kept[-1], keep


def _rows():
    g = torch.Generator().manual_seed(0)
    rnd = torch.randn(64, generator=g) * 3
    inf = float("-inf")
    return {
        "random64": rnd,
        "random63": rnd[:63].clone(),
        "ties": torch.tensor([1.0, 3.0, 2.0, 3.0, 2.0, 2.0, 0.5, 2.0, 1.0, 3.0]),
        "one": torch.tensor([0.7]),
        "minus_inf": torch.tensor([inf, 1.0, 0.0, inf, 2.0, 2.0, inf, -1.0]),
        "zeros": torch.tensor([0.0, -0.0, 0.0, -0.0, -1.0]),
    }


CASES = [  # (row, temperature, top_k, top_p, min_p)
    ("random64", 0.8, 10, 1.0, 0.0), ("random64", 0.8, 0, 0.7, 0.0), ("random64", 0.8, 0, 1.0, 0.1),
    ("random64", 1.3, 20, 0.8, 0.02), ("random63", 0.5, 63, 0.999, 0.0), ("random63", 2.0, 100, 1.0, 0.0),
    ("random64", 1.0, 1, 1.0, 0.0), ("random64", 1.0, 0, 1e-6, 0.0), ("random64", 0.8, 0, 1.0, 0.0),
    # top_k ties: the 2nd..4th largest are all 3.0, then five 2.0
    ("ties", 1.0, 2, 1.0, 0.0), ("ties", 1.0, 4, 1.0, 0.0), ("ties", 1.0, 8, 1.0, 0.0),
    # top_p ties straddling the threshold: the three 3.0 hold 0.61 of the mass, the five 2.0 0.37
    ("ties", 1.0, 0, 0.3, 0.0), ("ties", 1.0, 0, 0.7, 0.0), ("ties", 1.0, 0, 0.99, 0.0), ("ties", 1.0, 4, 0.7, 0.0),
    ("ties", 1.0, 0, 1.0, 0.0), ("ties", 1.0, 0, 1.0, 1.0), ("ties", 0.5, 0, 1.0, 0.3), ("ties", 1.0, 5, 0.9, 0.2),
    ("one", 0.8, 0, 1.0, 0.0), ("one", 0.8, 3, 0.5, 1.0), ("one", 0.0, 0, 1.0, 0.0),
    ("minus_inf", 1.0, 0, 1.0, 0.0), ("minus_inf", 1.0, 6, 0.9, 0.0), ("minus_inf", 1.0, 0, 0.5, 0.0),
    ("minus_inf", 0.7, 0, 1.0, 0.2), ("minus_inf", 0.0, 0, 1.0, 0.0),
    ("zeros", 1.0, 2, 1.0, 0.0), ("zeros", 1.0, 0, 0.5, 0.0), ("zeros", 0.0, 0, 1.0, 0.0), ("ties", 0.0, 3, 0.5, 0.5),
]
UNIFORMS = [2.0 ** -25, 0.013, 0.21, 0.37, 0.5, 0.64, 0.83, 0.97, 1 - 2.0 ** -25]


@pytest.mark.parametrize("name,t,k,p,mp", CASES)
def test_reference_matches_brute_force(name, t, k, p, mp):
    x = _rows()[name]
    n = len(UNIFORMS)
    got = ref.sample_logits_ref(x[None].expand(n, -1), [t] * n, [k] * n, [p] * n, [mp] * n, [0] * n, [0] * n,
                                torch.tensor(UNIFORMS, dtype=torch.float64))
    want = [_brute(x, t, k, p, mp, u) for u in UNIFORMS]
    assert got.tolist() == [tok for tok, _ in want]
    if t > 0:
        kept = ref.sample_kept_ref(x, t, k, p, mp)[1]
        assert set(torch.nonzero(kept).reshape(-1).tolist()) == want[0][1]


def test_reference_special_cases():
    rows = _rows()
    ties = rows["ties"]
    kept = lambda *a: torch.nonzero(ref.sample_kept_ref(ties, *a)[1]).reshape(-1).tolist()  # noqa: E731
    assert kept(1.0, 2, 1.0, 0.0) == [1, 3, 9]            # top_k inside a tie keeps the whole tie
    assert kept(1.0, 4, 1.0, 0.0) == [1, 2, 3, 4, 5, 7, 9]
    assert kept(1.0, 0, 0.3, 0.0) == [1, 3, 9]            # the threshold falls inside the tie of maxima
    assert kept(1.0, 0, 0.7, 0.0) == [1, 2, 3, 4, 5, 7, 9]
    assert kept(1.0, 0, 1.0, 1.0) == [1, 3, 9]            # min_p = 1: only the maxima
    assert kept(1.0, 0, 1.0, 0.0) == list(range(10))
    greedy = ref.sample_logits_ref(ties[None], [0.0], [5], [0.1], [0.9], [1], [2])
    assert greedy.tolist() == [1]                          # lowest index of the maximum
    one = ref.sample_logits_ref(rows["one"][None].expand(3, 1), [0.0, 1.0, 5.0], [0, 1, 0], [1.0, 0.2, 1.0],
                                [0.0, 1.0, 0.0], [0, 1, 2], [0, 1, 2])
    assert one.tolist() == [0, 0, 0]
    # Philox-driven: what the uniforms argument would give
    x = rows["random64"][None].expand(8, -1)
    seeds, steps = list(range(8)), [3] * 8
    a = ref.sample_logits_ref(x, [3.0] * 8, [0] * 8, [0.95] * 8, [0.0] * 8, seeds, steps)
    b = ref.sample_logits_ref(x, [3.0] * 8, [0] * 8, [0.95] * 8, [0.0] * 8, None, None,
                              ref.philox_uniforms(seeds, steps))
    assert torch.equal(a, b) and len(set(a.tolist())) > 1


def test_op_on_cpu_runs_the_reference_and_broadcasts_parameters():
    x = _rows()["random64"][None].expand(4, -1).contiguous()
    assert not ops.sample_logits_supported(x)
    got = ops.sample_logits(x, 0.8, top_k=torch.tensor([0, 5, 0, 5]), top_p=[0.9, 1.0, 0.5, 0.7], min_p=0.01, seeds=7,
                            steps=torch.arange(4))
    want = ref.sample_logits_ref(x, [0.8] * 4, [0, 5, 0, 5], [0.9, 1.0, 0.5, 0.7], [0.01] * 4, [7] * 4, [0, 1, 2, 3])
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert ops.sample_logits(x[:0], 0.8).shape == (0,)


# ------------------------------------------------------------------------------------ validation
@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    return build_llama("llama3-tiny", dtype=torch.float32).eval()


BAD = [("temperature", dict(temperature=-0.1)), ("temperature", dict(temperature=float("nan"))),
       ("temperature", dict(temperature=float("inf"))), ("top_k", dict(temperature=1.0, top_k=-1)),
       ("top_p", dict(temperature=1.0, top_p=0.0)), ("top_p", dict(temperature=1.0, top_p=1.5)),
       ("top_p", dict(temperature=1.0, top_p=float("nan"))), ("min_p", dict(temperature=1.0, min_p=-0.1)),
       ("min_p", dict(temperature=1.0, min_p=1.01))]


@pytest.mark.parametrize("name,kw", BAD)
def test_op_validation(name, kw):
    x = torch.zeros(2, 8)
    with pytest.raises(ValueError, match=name):
        ops.sample_logits(x, **kw)


def test_op_validation_of_shapes():
    x = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="logits"):
        ops.sample_logits(torch.zeros(8), 1.0)
    with pytest.raises(ValueError, match="logits"):
        ops.sample_logits(torch.zeros(2, 2, 8), 1.0)
    for name in ("temperature", "top_k", "top_p", "min_p", "seeds", "steps"):
        kw = {"temperature": 1.0, name: [1, 1, 1]}
        with pytest.raises(ValueError, match=name):
            ops.sample_logits(x, **kw)
    with pytest.raises(ValueError, match="uniforms"):
        ops.sample_logits(x, 1.0, uniforms=torch.zeros(3))


@pytest.mark.parametrize("name,kw", [b for b in BAD if b[0] in ("top_p", "min_p")])
def test_generate_and_add_request_validation(name, kw):
    m = _model()
    with pytest.raises(ValueError, match=name):
        m.generate([[1, 2, 3]], 2, **kw)
    eng = GenerationEngine(m, max_slots=2, num_blocks=8)
    with pytest.raises(ValueError, match=name):
        eng.add_request([1, 2, 3], 2, **kw)
    assert not eng.has_work() and not eng.waiting  # refused before anything is queued


def test_fused_requests_validate_temperature_and_top_k():
    eng = GenerationEngine(_model(), max_slots=2, num_blocks=8, fused_sampling=True)
    with pytest.raises(ValueError, match="temperature"):
        eng.add_request([1, 2, 3], 2, temperature=-1.0)
    with pytest.raises(ValueError, match="top_k"):
        eng.add_request([1, 2, 3], 2, temperature=1.0, top_k=-2)
    with pytest.raises(ValueError, match="top_k"):
        _model().generate([[1, 2, 3]], 2, temperature=1.0, top_k=-2, fused_sampling=True)
    assert not eng.has_work()


# ---------------------------------------------------------------------------------------- engine
def _drain(eng):
    out = {}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            out.setdefault(rid, []).append(tok)
    return out


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (n,), generator=g).tolist()


class _Counted:
    """``ops.sample_logits`` behind a counter (the engine and ``generate`` call it through ``ops``)."""

    def __init__(self, monkeypatch):
        self.rows, real = [], ops.sample_logits

        def wrapper(logits, *a, **kw):
            self.rows.append(logits.shape[0])
            return real(logits, *a, **kw)

        monkeypatch.setattr(ops, "sample_logits", wrapper)


def test_engine_samples_once_per_logits_tensor(monkeypatch):
    calls = _Counted(monkeypatch)
    m = _model()
    eng = GenerationEngine(m, max_slots=3, num_blocks=32, fused_sampling=True)
    for i in range(3):
        eng.add_request(_prompt(4 + i, 20 + i), 5, temperature=0.8, top_k=20, seed=i)
    assert len(eng.step()) == 6 and calls.rows == [3, 3]     # one prefill tensor, one decode tensor
    assert len(eng.step()) == 3 and calls.rows == [3, 3, 3]
    _drain(eng)
    assert calls.rows == [3] * 5
    # generate: one call per step over all rows
    calls.rows.clear()
    out = m.generate([_prompt(4, 1), _prompt(6, 2)], 4, temperature=0.8, top_p=0.9, seed=5)
    assert calls.rows == [2] * 4 and [len(o) for o in out] == [4, 4]
    # a mixed engine: only the fused rows go through the op
    calls.rows.clear()
    eng = GenerationEngine(m, max_slots=3, num_blocks=32)
    eng.add_request(_prompt(4, 1), 3, temperature=0.8, top_k=20, seed=1)
    eng.add_request(_prompt(5, 2), 3, temperature=0.8, top_p=0.9, seed=1)
    eng.add_request(_prompt(6, 3), 3, temperature=0.8, min_p=0.05, seed=1)
    _drain(eng)
    assert calls.rows == [2] * 3


def test_default_streams_are_those_of_sample_tokens(monkeypatch):
    calls = _Counted(monkeypatch)
    m = _model()
    prompts, n = [_prompt(5, 31), _prompt(9, 32)], 8

    def direct(prompt):
        """The parent's sampler driven by hand: ``sample_tokens`` on each step's logits row."""
        cache = PagedKVCache(m.cfg, 8, 16, dtype=torch.float32)
        gen = _seeded_generator(torch.device("cpu"), 0.8, 3)
        logits, toks = m.prefill([prompt], None, cache, ["s"]), []
        for _ in range(n):
            toks.append(int(sample_tokens(logits[0][None], 0.8, 20, gen)[0]))
            logits = m.decode_step([toks[-1]], cache, ["s"])
        return toks

    want = [direct(p) for p in prompts]
    eng = GenerationEngine(m, max_slots=1, num_blocks=8)
    rids = [eng.add_request(p, n, temperature=0.8, top_k=20, seed=3) for p in prompts]
    out = _drain(eng)
    assert [out[r] for r in rids] == want
    assert [m.generate([p], n, temperature=0.8, top_k=20, seed=3)[0] for p in prompts] == want
    assert calls.rows == []


class _TableModel:
    """Stand-in model: the logits row after a sequence is a fixed function (a table row) of its
    last token. It allocates cache slots the way the ``Llama`` methods do."""
    V = 48

    def __init__(self):
        self.cfg = types.SimpleNamespace(vocab_size=self.V, max_seq_len=256, num_kv_heads=1, head_dim=8, num_layers=1)
        g = torch.Generator().manual_seed(4)
        self.table = torch.randn(self.V, self.V, generator=g) * 1.5
        self.table[:, 7] = self.table[:, 11]  # an exact tie in every row
        self.embed = types.SimpleNamespace(weight=self.table)

    def prefill(self, tokens, lengths, cache, seq_ids):
        Llama._allocate(cache, [(s, len(t)) for s, t in zip(seq_ids, tokens)])
        return self.table[[t[-1] for t in tokens]]

    def extend(self, tokens, cache, seq_ids):
        return self.prefill(tokens, None, cache, seq_ids)

    def decode_step(self, tokens, cache, seq_ids):
        Llama._allocate(cache, [(s, 1) for s in seq_ids])
        return self.table[list(tokens)]


MIXED = [  # prompt, sampling arguments: greedy, top_p, min_p, top_k; one seed on two prompts
    ([3, 5], dict(temperature=0.0)),
    ([8, 1, 2], dict(temperature=0.9, top_p=0.8, seed=5)),
    ([9], dict(temperature=1.2, min_p=0.05, seed=6)),
    ([4, 4, 4, 4], dict(temperature=0.7, top_k=6, seed=7)),
    ([30, 21], dict(temperature=0.9, top_p=0.8, seed=5)),
]


@pytest.mark.parametrize("prefill_chunk", [None, 2])
def test_fused_streams_do_not_depend_on_batching(prefill_chunk):
    m, n = _TableModel(), 9

    def run(requests, slots):
        eng = GenerationEngine(m, max_slots=slots, num_blocks=16, prefill_chunk=prefill_chunk, fused_sampling=True)
        rids = [eng.add_request(p, n, **kw) for p, kw in requests]
        out = _drain(eng)
        assert eng.cache.num_free_blocks == 16
        return [out[r] for r in rids]

    together = run(MIXED, 3)
    assert together == [run([r], 1)[0] for r in MIXED]
    for (prompt, kw), stream in zip(MIXED, together):  # the op by hand, steps 0, 1, 2, ...
        last, want = prompt[-1], []
        for step in range(n):
            last = int(ops.sample_logits(m.table[last][None], kw["temperature"], kw.get("top_k", 0),
                                         kw.get("top_p", 1.0), kw.get("min_p", 0.0), kw.get("seed", 0), step)[0])
            want.append(last)
        assert stream == want
    assert together[1] != together[4] and len({tuple(s) for s in together}) == 5


def test_tiny_top_p_is_greedy():
    m = _model()
    prompt, n = _prompt(6, 77), 8
    # no step's maximum logit is tied (else top_p would keep the whole tie)
    cache = PagedKVCache(m.cfg, 8, 16, dtype=torch.float32)
    logits, greedy = m.prefill([prompt], None, cache, ["s"]), []
    for _ in range(n):
        assert int((logits[0] == logits[0].max()).sum()) == 1
        greedy.append(int(logits[0].argmax()))
        logits = m.decode_step([greedy[-1]], cache, ["s"])
    eng = GenerationEngine(m, max_slots=2, num_blocks=16)
    a = eng.add_request(prompt, n, temperature=1.0, top_p=1e-6, seed=9)
    b = eng.add_request(prompt, n, temperature=0.0)
    out = _drain(eng)
    assert out[a] == out[b]


def test_serve_deployment_passes_the_sampling_arguments():
    import asyncio

    from ray_community_amd.serve.llm import _LlamaDeployment

    async def main():
        dep = _LlamaDeployment(dtype="float32", max_slots=2, num_blocks=16, fused_sampling=True)
        assert (await dep.status())["fused_sampling"] is True
        toks = [t async for t in dep.generate([1, 2, 3], 5, temperature=0.9, top_p=0.8, min_p=0.01, seed=4)]
        with pytest.raises(ValueError, match="top_p"):
            async for _ in dep.generate([1, 2, 3], 5, temperature=0.9, top_p=2.0):
                pass
        plain = _LlamaDeployment(dtype="float32", max_slots=2, num_blocks=16)
        assert "fused_sampling" not in await plain.status()
        again = [t async for t in plain.generate([1, 2, 3], 5, temperature=0.9, top_p=0.8, min_p=0.01, seed=4)]
        return toks, again

    toks, again = asyncio.run(main())
    assert len(toks) == 5 and toks == again
