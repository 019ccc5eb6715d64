"""The gfx950 kernels of ops/csrc/sampling_penalties.hip behind ``ops.penalize_logits`` and
``ops.token_logprobs`` against their references (``ops.reference``, themselves checked against
brute-force float64 loops in test_sampling_penalties_cpu.py).

``penalize_logits`` is compared bitwise: kernel and reference perform the same IEEE fp32
operations in the same order, and the inputs (``randn * 4`` logits, penalties of order 1) keep
every intermediate in the normal range, so denormal handling cannot differ. That is a condition
on the inputs, not a tolerance. Rows sit in a NaN-padded buffer (``PAD`` columns, so rows are not
16-byte aligned): a read outside a row poisons the result.

``token_logprobs``: ``top_ids`` compare stored values and indices only and must equal the
reference exactly. ``lp`` / ``top_lp`` stay within ``2**-19 + 2**-21 * |lp64|`` of the float64
oracle ``log_softmax(x.double())``: 4x the sum of (a) the roundings of ``x - m`` and of the result,
``<= 2**-23 * |lp|``, and (b) a relative error of ``S`` of ``2**-22`` from ``expf`` plus
``V * 2**-40`` from the fixed point, ``<= 2**-21`` in the logarithm. (b) allows ``expf`` 2 ulp; the
HIP math API documents 1 ulp for ``expf``. That table is not among the ROCm files installed next to
the compiler used here (no document under the ROCm tree gives ulp figures for the device math
functions), so the 1 ulp is quoted from the public HIP documentation, not confirmed locally; the
bound is the one derived above and is not fitted to any measured error.
"""
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.ops import reference as ref

gpu = pytest.mark.gpu

MARGIN = 1e-3
PAD = 3
VS = (1, 2, 63, 65, 1000, 4097, 128256)
DTYPES = [torch.bfloat16, torch.float32]
DTYPE_IDS = ["bf16", "fp32"]
NKINDS = 9
# (repetition, presence, frequency) per history kind; kind 8 is neutral
PENALTIES = [(1.3, 0.4, 0.25), (0.7, -0.5, 0.1), (1.0, 1.5, -0.3), (2.5, 0.0, 0.9), (1.3, 0.4, 0.25), (1.7, 0.2, 0.05),
             (1.2, 0.3, 0.15), (1.2, 0.3, 0.15), (1.0, 0.0, 0.0)]


def _histories(V, kinds, seed):
    """Flat tokens, ranges and penalties for one row per entry of ``kinds``:
    0 empty; 1 prompt only; 2 output only; 3 ids 0 and V - 1; 4 one id 300 times (same-address
    contention); 5 length 2500 (more than one id per thread); 6 / 7 one shared region, rows that
    differ only in ``end``; 8 neutral parameters over a non-empty history."""
    g = torch.Generator().manual_seed(seed)

    def rnd(n):
        return torch.randint(0, V, (n,), generator=g).tolist()

    flat, ranges, shared = [], [], None
    for kind in kinds:
        s = len(flat)
        if kind == 0:
            ranges.append((s, s, s))
        elif kind == 1:
            flat += rnd(17)
            ranges.append((s, s + 17, s + 17))
        elif kind == 2:
            flat += rnd(23)
            ranges.append((s, s, s + 23))
        elif kind == 3:
            flat += [0, V - 1, V - 1, 0, V - 1]
            ranges.append((s, s + 2, s + 5))
        elif kind == 4:
            one = rnd(1)
            flat += one + rnd(5) + one * 300
            ranges.append((s, s + 3, s + 306))
        elif kind == 5:
            flat += rnd(2500)
            ranges.append((s, s + 1000, s + 2500))
        elif kind in (6, 7):
            if shared is None:
                shared = s
                flat += rnd(40)
            ranges.append((shared, shared + 30, shared + (36 if kind == 6 else 39)))
        else:
            flat += rnd(50)
            ranges.append((s, s + 20, s + 50))
    cols = [[PENALTIES[k][i] for k in kinds] for i in range(3)]
    return flat, ranges, cols


@functools.lru_cache(maxsize=None)
def _logits(V, B, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * V + B + seed + (7 if dtype == torch.float32 else 0))
    full = torch.full((B, V + PAD), float("nan"), dtype=dtype)
    full[:, :V] = (torch.randn(B, V, generator=g) * 4).to(dtype)
    return full


@functools.lru_cache(maxsize=None)
def _penalty_case(V, kinds, dtype, seed):
    full = _logits(V, len(kinds), dtype)
    flat, ranges, (rep, pres, freq) = _histories(V, kinds, seed)
    want = ref.penalize_logits_ref(full[:, :V], flat, ranges, rep, pres, freq)
    assert not want.isnan().any()
    return full, flat, ranges, rep, pres, freq, want


def _run(case, V):
    full, flat, ranges, rep, pres, freq, want = case
    x = full.cuda()[:, :V]
    assert x.stride(0) == V + PAD and ops.sample_logits_supported(x)
    got = ops.penalize_logits(x, flat, ranges, rep, pres, freq)
    assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous() and got.shape == want.shape
    return got


def _same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_penalties_equal_the_reference(V, B, dtype):
    """Over the shapes, every history kind turns up (kinds cycle with V); the second call, with
    other histories, equals *its* reference, which it would not had the counters been left dirty."""
    first = tuple((VS.index(V) * B + b) % NKINDS for b in range(B))
    for kinds, seed in ((first, 1), (tuple((k + 4) % NKINDS for k in first), 2)):
        case = _penalty_case(V, kinds, dtype, seed)
        got = _run(case, V)
        assert torch.equal(got.cpu(), case[-1])
        assert _same_bits(got, case[-1])
    ws = ops._WS[(str(got.device), "penalty_counts")]
    assert int(ws.count_nonzero()) == 0


@gpu
@pytest.mark.parametrize("V", [1000, 128256])
def test_every_history_kind_in_one_batch(V):
    kinds = tuple(range(NKINDS))
    for dtype in DTYPES:
        case = _penalty_case(V, kinds, dtype, 3)
        got = _run(case, V)
        assert _same_bits(got, case[-1])
        assert torch.equal(got[8].cpu(), case[0][8, :V].float())          # neutral: the copy
        assert not torch.equal(got[6], got[7])                            # the two ends differ


@gpu
def test_a_row_does_not_depend_on_its_batch():
    V, kinds = 4097, (0, 1, 2, 3, 4, 6, 7, 8, 5)   # the long history last: it owns the end of the buffer
    full, flat, ranges, rep, pres, freq, want = _penalty_case(V, kinds, torch.bfloat16, 4)
    x = full.cuda()[:, :V]
    whole = ops.penalize_logits(x, flat, ranges, rep, pres, freq)
    assert _same_bits(whole, want)
    perm = [5, 8, 0, 7, 2, 6, 1, 4, 3]
    moved = ops.penalize_logits(x[torch.tensor(perm).cuda()], flat, [ranges[i] for i in perm], [rep[i] for i in perm],
                                [pres[i] for i in perm], [freq[i] for i in perm])
    assert torch.equal(moved, whole[torch.tensor(perm).cuda()])
    for b in (0, 4, 5, 7):
        alone = ops.penalize_logits(x[b:b + 1], flat, [ranges[b]], rep[b], pres[b], freq[b])
        assert torch.equal(alone[0], whole[b])
    # device tensors for tokens and ranges, with ids outside [0, V) that the kernel must skip
    dirty = torch.tensor(flat + [-5, V, 1 << 30], dtype=torch.int32).cuda()
    rng = torch.tensor(ranges, dtype=torch.int32)
    assert ranges[8][2] == len(flat)
    rng[8, 2] = len(flat) + 3      # the last row now also covers the bad ids
    got = ops.penalize_logits(x, dirty, rng.cuda(), rep, pres, freq)
    assert torch.equal(got, whole)


# ----------------------------------------------------------------------- composition with the sampler
def _breakpoints(x, temperature, top_k):
    w, keep = ref.sample_kept_ref(x, temperature, top_k, 1.0, 0.0)
    vals, inv = torch.unique(x.float()[keep], return_inverse=True)
    mass = torch.zeros(vals.shape[0], dtype=torch.float64).index_add_(0, inv, w[keep])
    return (mass.flip(0).cumsum(0) - mass.flip(0)) / mass.sum()


def _clear_top_p(x, temperature, top_k, top_p):
    """``top_p`` moved (deterministically) until it keeps ``MARGIN`` from every breakpoint."""
    if temperature > 0 and top_p < 1:
        bp = _breakpoints(x, temperature, top_k)
        if float((bp - ref._f32(top_p)).abs().min()) < MARGIN:
            edges = torch.cat([bp, torch.ones(1, dtype=torch.float64)])
            mids, gaps = (edges[1:] + edges[:-1]) / 2, edges[1:] - edges[:-1]
            mids = mids[gaps >= 2.5 * MARGIN]
            top_p = float(mids[(mids - top_p).abs().argmin()])
        assert 0 < top_p < 1 and float((bp - ref._f32(top_p)).abs().min()) >= MARGIN
    return top_p


def _wide_interval(x, prm, pick):
    """(u, token): the centre of an oracle CDF interval of half-width >= MARGIN."""
    w, keep = ref.sample_kept_ref(x, *prm)
    cdf = (w * keep).cumsum(0) / (w * keep).sum()
    width = torch.diff(cdf, prepend=torch.zeros(1, dtype=torch.float64))
    wide = torch.nonzero(keep & (width >= 2 * MARGIN)).reshape(-1)
    assert wide.numel()
    tok = int(wide[pick % wide.numel()])
    return float(cdf[tok] - width[tok] / 2), tok


@gpu
def test_the_sampler_takes_the_penalized_logits():
    """``sample_logits`` on the kernel's own output: greedy rows, and sampled rows whose uniform sits
    at the centre of an oracle CDF interval of half-width >= MARGIN (the condition of
    test_sampling_gpu.py, under which the fp32 sums of the two sides cannot decide differently)."""
    V, kinds = 4097, tuple(range(NKINDS))
    case = _penalty_case(V, kinds, torch.bfloat16, 5)
    P = _run(case, V)
    rows = P.cpu()
    assert _same_bits(P, case[-1])
    mix = [(0.0, 0, 1.0), (0.8, 0, 1.0), (0.8, 50, 1.0), (1.0, 0, 0.9), (0.0, 7, 0.3), (1.3, 5, 0.5), (2.0, 3, 1.0),
           (0.5, 0, 0.3), (1.0, 200, 0.95)]
    params, uniforms, want = [], [], []
    for b, (t, k, p) in enumerate(mix):
        if t == 0:
            u, tok = 0.5, int(rows[b].argmax())
        else:
            p = _clear_top_p(rows[b], t, k, p)
            u, tok = _wide_interval(rows[b], (t, k, p, 0.0), 7 * b + 1)
        params.append((t, k, p, 0.0))
        uniforms.append(u)
        want.append(tok)
    cols = [[prm[i] for prm in params] for i in range(4)]
    u = torch.tensor(uniforms, dtype=torch.float32)
    assert ref.sample_logits_ref(rows, *cols, [0] * 9, [0] * 9, u).tolist() == want
    got = ops.sample_logits(P, *cols, seeds=0, steps=0, uniforms=u.cuda())
    assert got.cpu().tolist() == want


# ------------------------------------------------------------------------------------ logprobs
@functools.lru_cache(maxsize=None)
def _logprob_case(V, B, dtype, top_n):
    full = _logits(V, B, dtype, seed=50)
    g = torch.Generator().manual_seed(V + B)
    tokens = torch.randint(0, V, (B,), generator=g)
    x = full[:, :V]
    return full, tokens, ref.token_logprobs_ref(x, tokens, top_n), torch.log_softmax(x.double(), dim=1)


def _check_logprobs(full, V, tokens, want, oracle, top_n):
    x = full.cuda()[:, :V]
    assert ops.sample_logits_supported(x)
    lp, ids, tlp = ops.token_logprobs(x, tokens.cuda(), top_n)
    B, n = x.shape[0], min(top_n, V)
    assert lp.is_cuda and lp.dtype == torch.float32 and lp.shape == (B,)
    assert ids.dtype == torch.int64 and ids.shape == (B, top_n) and tlp.dtype == torch.float32 and tlp.shape == (B, top_n)
    lp, ids, tlp = lp.cpu(), ids.cpu(), tlp.cpu()
    assert torch.equal(ids, want[1]), (ids, want[1])
    assert ids[:, n:].eq(-1).all() and tlp[:, n:].eq(float("-inf")).all()

    def close(got, w64):
        err, bound = (got.double() - w64).abs(), 2.0 ** -19 + 2.0 ** -21 * w64.abs()
        print(f"V={V} top_n={top_n}: max err {float(err.max()):.3e}, min bound {float(bound.min()):.3e}")
        return bool((err <= bound).all())

    assert close(lp, oracle.gather(1, tokens[:, None])[:, 0])
    if n:
        assert close(tlp[:, :n], oracle.gather(1, ids[:, :n]))
    again = ops.token_logprobs(x, tokens.cuda(), top_n)
    assert _same_bits(again[0], lp) and torch.equal(again[1].cpu(), ids) and _same_bits(again[2], tlp)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_logprobs_against_the_oracle(V, B, dtype):
    """bf16 rows of 1000 and more ``randn * 4`` values are full of equal logits, so most thresholds
    here are ties that straddle the ``top_n``-th place; V < top_n gives the -1 / -inf tail."""
    for top_n in (20, 5) if V > 2 else (5,):
        full, tokens, want, oracle = _logprob_case(V, B, dtype, top_n)
        _check_logprobs(full, V, tokens, want, oracle, top_n)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_logprobs_ties(dtype):
    """An all-equal row (ids 0..n-1), a tie that straddles the n-th place across tiles (equal values
    at scattered indices, more than one 16-byte tile apart), -0 / +0, and a tie that ends exactly at n."""
    V, n = 20000, 20
    x = _logits(V, 5, dtype, seed=60).clone()
    x[0, :V] = 1.5
    top = torch.tensor([11, 12, 5000, 9000, 9001, 13000, 13001, 19990, 19999, 3, 16384, 16383, 8192, 8191, 4096, 4095,
                        1024, 1023, 7, 19000, 19001, 19002, 19003, 19004, 19005, 19006])
    x[1, top] = 30.0                      # 26 equal maxima: the 20 lowest indices
    x[1, 77] = 31.0                       # and one above them: 19 ties needed
    x[2, :V] = x[2, :V].clamp(max=0.0)    # many maxima equal to 0 ...
    x[2, 1::2] = -x[2, 1::2].abs() - 0.0  # ... and -0 among them
    x[2, 5] = -0.0
    x[3, top[:20]] = 40.0                 # exactly n ties at the top
    tokens = torch.tensor([V - 1, 77, 5, 11, 0])
    want = ref.token_logprobs_ref(x[:, :V], tokens, n)
    assert want[1][0].tolist() == list(range(n)) and want[1][1].tolist() == [77] + sorted(top.tolist())[:19]
    assert want[1][3].tolist() == sorted(top[:20].tolist())
    _check_logprobs(x, V, tokens, want, torch.log_softmax(x[:, :V].double(), dim=1), n)


# ------------------------------------------------------------------------- fallbacks, end to end
@gpu
def test_fallbacks():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 300, generator=g) * 4
    flat, ranges, (rep, pres, freq) = _histories(150, (1, 2, 4, 8), 6)
    tokens = torch.tensor([3, 299, 0, 7])
    for make, src in ((lambda t: t, x), (lambda t: t.half().cuda(), x.half()), (lambda t: t.cuda()[:, ::2], x[:, ::2])):
        dev = make(x)
        assert not ops.sample_logits_supported(dev)
        got = ops.penalize_logits(dev, flat, ranges, rep, pres, freq)
        assert got.device == dev.device and got.dtype == torch.float32
        assert torch.equal(got.cpu(), ref.penalize_logits_ref(src, flat, ranges, rep, pres, freq))
        toks = (tokens % src.shape[1]).to(dev.device)
        lp, ids, tlp = ops.token_logprobs(dev, toks, 4)
        want = ref.token_logprobs_ref(src, toks.cpu(), 4)
        assert lp.device == dev.device and torch.equal(lp.cpu(), want[0]) and torch.equal(ids.cpu(), want[1])
        assert torch.equal(tlp.cpu(), want[2])
    on = x.bfloat16().cuda()
    lp, ids, tlp = ops.token_logprobs(on, tokens.cuda(), 0)   # top_n = 0: the chosen token's lp alone
    assert ids.shape == (4, 0) and ids.dtype == torch.int64 and tlp.shape == (4, 0) and lp.shape == (4,)
    assert _same_bits(lp, ops.token_logprobs(on, tokens.cuda(), 3)[0].cpu())
    empty = torch.empty(0, 300, device="cuda", dtype=torch.bfloat16)
    assert ops.penalize_logits(empty, [], []).shape == (0, 300)
    lp, ids, tlp = ops.token_logprobs(empty, torch.empty(0, dtype=torch.long, device="cuda"), 2)
    assert lp.shape == (0,) and ids.shape == (0, 2) and tlp.shape == (0, 2) and lp.is_cuda


@gpu
def test_llama_end_to_end():
    from ray_community_amd.models import GenerationEngine, build_llama

    torch.manual_seed(0)
    model = build_llama("llama3-tiny", device="cuda", dtype=torch.bfloat16).eval()
    V = model.cfg.vocab_size
    prompts = [[5, 9, 200, 31, 5, 9, 200, 31], [77, 3], [400, 401, 402, 403, 404]]
    pen = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.25)
    mode = dict(temperature=0.9, top_p=0.9, seed=11)

    def run(requests, **engine_kw):
        eng = GenerationEngine(model, max_slots=4, num_blocks=32, **engine_kw)
        rids = [eng.add_request(p, 12, **kw) for p, kw in zip(prompts, requests)]
        out, lps = {r: [] for r in rids}, {r: [] for r in rids}
        while eng.has_work():
            for rid, tok, _ in eng.step():
                out[rid].append(tok)
            for rid in rids:
                lps[rid].extend(eng.pop_logprobs(rid))
        return [out[r] for r in rids], [lps[r] for r in rids]

    a = model.generate(prompts, 12, logprobs=5, **mode, **pen)
    assert a == model.generate(prompts, 12, logprobs=5, **mode, **pen)
    toks, lps = a
    for stream, entries in zip(toks, lps):
        assert len(stream) == 12 and all(0 <= t < V for t in stream) and [e[0] for e in entries] == stream
        for tok, lp, top in entries:
            assert lp <= 0 and len(top) == 5 and all(top[i][1] >= top[i + 1][1] for i in range(4))
            assert all(lp == v for i, v in top if i == tok)
    plain = model.generate(prompts, 12, fused_sampling=True, **mode)
    assert toks != plain
    # a neutral row rides through penalize_logits next to penalized ones and keeps the plain stream
    mixed, mixed_lp = run([dict(mode), dict(mode, logprobs=5, **pen), dict(mode)], fused_sampling=True)
    base, _ = run([dict(mode)] * 3, fused_sampling=True)
    assert mixed[0] == base[0] and mixed[2] == base[2]
    assert [e[0] for e in mixed_lp[1]] == mixed[1] and mixed_lp[0] == []
    greedy = model.generate(prompts, 40, presence_penalty=1e6)
    assert all(len(set(s)) == 40 for s in greedy)
