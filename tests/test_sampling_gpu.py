"""The gfx950 batched sampler (ops/csrc/sampling.hip behind ``ops.sample_logits``) against the
float64 reference (``ops.reference.sample_kept_ref`` / ``sample_logits_ref``, themselves checked
against a brute-force oracle in test_sampling_cpu.py).

Exact agreement needs no tolerance because the cases keep clear of every decision the two sides
could round differently: each row's ``top_p`` is at least ``MARGIN`` = 1e-3 (in units of the
survivors' mass) from every cumulative-mass breakpoint of the oracle, each ``min_p`` at least 1e-3
(relative) from every weight, and each uniform sits at the centre of an oracle CDF interval of
half-width >= 1e-3. The margin is a condition, not a measurement: fp32 accumulation over V <= 2**17
positive terms is below 2e-5 relative even summed naively in blocks (the kernel sums 2**-40
fixed-point integers, far tighter), so 1e-3 is 50 times the worst honest error. Rows without such
an interval would be regenerated from another seed; with ``randn * 4`` logits the top token alone
is wider (``test_cases_keep_their_margins``, CPU only, checks all of this).
"""
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.ops import reference as ref

gpu = pytest.mark.gpu

MARGIN = 1e-3
PAD = 3  # extra columns per row (NaN): rows are not 16-byte aligned and any read past a row poisons it
VS = (1, 2, 63, 64, 65, 1000, 4097, 128256)
SHAPES = [(V, B) for V in VS for B in (1, 3, 33) if B < 33 or V <= 4097]
# (temperature, top_k, top_p, min_p) per row, cycled; row 0 of the cycle is greedy
MIX = [(0.0, 0, 1.0, 0.0), (0.8, 0, 1.0, 0.0), (0.8, 50, 1.0, 0.0), (1.0, 0, 0.9, 0.0), (0.7, 0, 1.0, 0.05),
       (0.8, 50, 0.9, 0.02), (1.3, 5, 0.5, 0.0), (0.0, 7, 0.3, 0.5), (2.0, 3, 1.0, 0.0), (0.5, 0, 0.3, 0.0),
       (1.0, 200, 0.95, 0.001)]


def _breakpoints(x, temperature, top_k):
    """Cumulative mass fractions S / W of the oracle at which ``top_p`` changes the kept set."""
    w, keep = ref.sample_kept_ref(x, temperature, top_k, 1.0, 0.0)
    vals, inv = torch.unique(x.float()[keep], return_inverse=True)
    mass = torch.zeros(vals.shape[0], dtype=torch.float64).index_add_(0, inv, w[keep])
    return (mass.flip(0).cumsum(0) - mass.flip(0)) / mass.sum()


def _clear_params(x, temperature, top_k, top_p, min_p):
    """``top_p`` and ``min_p`` moved (deterministically) until they keep the margins."""
    if temperature > 0 and top_p < 1:
        bp = _breakpoints(x, temperature, top_k)
        if float((bp - ref._f32(top_p)).abs().min()) < MARGIN:
            # the middle of the nearest gap between breakpoints that is wide enough (the first gap,
            # the top token's mass, always is)
            edges = torch.cat([bp, torch.ones(1, dtype=torch.float64)])
            mids, gaps = (edges[1:] + edges[:-1]) / 2, edges[1:] - edges[:-1]
            mids = mids[gaps >= 2.5 * MARGIN]
            top_p = float(mids[(mids - top_p).abs().argmin()])
        assert 0 < top_p < 1 and float((bp - ref._f32(top_p)).abs().min()) >= MARGIN
    if temperature > 0 and min_p > 0:
        w, _ = ref.sample_kept_ref(x, temperature, 0, 1.0, 0.0)
        while float((w / ref._f32(min_p) - 1).abs().min()) < MARGIN:
            min_p *= 1 + 3 * MARGIN
        assert min_p <= 1
    return top_p, min_p


def _wide_interval(x, prm, pick):
    """(u, token): the centre of an oracle CDF interval of half-width >= MARGIN, or None."""
    w, keep = ref.sample_kept_ref(x, *prm)
    cdf = (w * keep).cumsum(0) / (w * keep).sum()
    width = torch.diff(cdf, prepend=torch.zeros(1, dtype=torch.float64))
    wide = torch.nonzero(keep & (width >= 2 * MARGIN)).reshape(-1)
    if not wide.numel():
        return None
    tok = int(wide[pick % wide.numel()])
    return float(cdf[tok] - width[tok] / 2), tok


@functools.lru_cache(maxsize=None)
def _case(V, B, dtype):
    """CPU side of one exact-agreement case: padded logits, per-row parameters, uniforms, tokens."""
    g = torch.Generator().manual_seed(1000 * V + B + (7 if dtype == torch.float32 else 0))
    full = torch.full((B, V + PAD), float("nan"), dtype=dtype)
    params, uniforms, want, regenerated = [], [], [], 0
    for b in range(B):
        t, k, p, mp = MIX[(b + V) % len(MIX)]
        while True:
            x = (torch.randn(V, generator=g) * 4).to(dtype)
            if t == 0:
                u, tok = 0.5, int(torch.nonzero(x.float() == x.float().max())[0])
                break
            p2, mp2 = _clear_params(x, t, k, p, mp)
            got = _wide_interval(x, (t, k, p2, mp2), int(torch.randint(1 << 30, (1,), generator=g)))
            if got is not None:
                (u, tok), p, mp = got, p2, mp2
                break
            regenerated += 1
        full[b, :V] = x
        params.append((t, k, p, mp))
        uniforms.append(u)
        want.append(tok)
    return {"full": full, "params": params, "uniforms": torch.tensor(uniforms, dtype=torch.float32),
            "want": torch.tensor(want), "regenerated": regenerated}


def _columns(c):
    return [[prm[i] for prm in c["params"]] for i in range(4)]


def test_cases_keep_their_margins():
    """CPU: the reference returns the chosen token of every row at the chosen uniform, the margins
    hold, and no row had to be regenerated."""
    for V, B in [(1, 3), (2, 33), (65, 33), (1000, 33), (4097, 3), (128256, 3)]:
        for dtype in (torch.bfloat16, torch.float32):
            c = _case(V, B, dtype)
            assert c["regenerated"] == 0
            x = c["full"][:, :V]
            got = ref.sample_logits_ref(x, *_columns(c), [0] * B, [0] * B, c["uniforms"])
            assert torch.equal(got, c["want"])
            for b, (t, k, p, mp) in enumerate(c["params"]):
                if t > 0 and p < 1:
                    assert float((_breakpoints(x[b], t, k) - ref._f32(p)).abs().min()) >= MARGIN


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_tokens_equal_the_oracle(V, B, dtype):
    c = _case(V, B, dtype)
    logits = c["full"].cuda()[:, :V]
    assert logits.stride(0) == V + PAD and ops.sample_logits_supported(logits)
    got = ops.sample_logits(logits, *_columns(c), seeds=0, steps=0, uniforms=c["uniforms"].cuda())
    assert got.dtype == torch.int64 and got.shape == (B,)
    assert torch.equal(got.cpu(), c["want"])


@gpu
def test_philox_tokens_stay_in_the_kept_set():
    V, N, R = 1000, 4096, 16
    g = torch.Generator().manual_seed(11)
    base = (torch.randn(R, V, generator=g) * 4).bfloat16()
    prms = []
    for r in range(R):
        t, k, p, mp = MIX[1 + r % (len(MIX) - 1)]
        t = t if t > 0 else 0.9
        prms.append((t, k) + _clear_params(base[r], t, k, p, mp))
    kept = torch.stack([ref.sample_kept_ref(base[r], *prms[r])[1] for r in range(R)])
    rows = torch.arange(N) % R
    seeds = [(i * 2654435761) % (1 << 64) for i in range(N)]
    steps = [(i // R) * 97 + (i % 5) * (1 << 32) for i in range(N)]
    cols = [[prms[r][i] for r in rows.tolist()] for i in range(4)]
    got = ops.sample_logits(base.cuda()[rows.cuda()], *cols, seeds=seeds, steps=steps).cpu()
    assert int(got.min()) >= 0 and int(got.max()) < V
    assert bool(kept[rows, got].all())
    assert all(len(set(got[rows == r].tolist())) > 1 for r in range(R) if int(kept[r].sum()) > 1)


@gpu
def test_device_philox_matches_the_reference():
    V, N = 1 << 16, 256
    edge = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, (1 << 64) - 1]
    g = torch.Generator().manual_seed(5)
    rnd = [int(a) * (1 << 32) + int(b) for a, b in torch.randint(1 << 32, (2 * N, 2), generator=g).tolist()]
    seeds = ([s for s in edge for _ in edge] + rnd)[:N]
    steps = ([s for _ in edge for s in edge] + rnd[N:])[:N]
    u = ref.philox_uniforms(seeds, steps).double()
    logits = torch.zeros(1, V, device="cuda").expand(N, V)  # equal weights: the inverse CDF is exact
    got = ops.sample_logits(logits, 1.0, seeds=seeds, steps=steps).cpu()
    assert torch.equal(got, torch.floor(u * V).long())


@gpu
def test_distribution():
    V, N = 16, 65535
    x = torch.linspace(-3.0, 1.5, V)
    p = torch.softmax(x.double(), 0)
    got = ops.sample_logits(x.cuda()[None].expand(N, V), 1.0, seeds=2024, steps=list(range(N))).cpu()
    counts = torch.bincount(got, minlength=V).double()
    assert counts.shape[0] == V
    bound = 6 * torch.sqrt(N * p * (1 - p)) + 1
    assert bool(((counts - N * p).abs() <= bound).all()), (counts - N * p, bound)


@gpu
def test_determinism_and_row_independence():
    V, B = 4097, 33
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(B, V, generator=g) * 4).bfloat16().cuda()
    cols = [[MIX[b % len(MIX)][i] for b in range(B)] for i in range(4)]
    seeds, steps = [b * 31 + 1 for b in range(B)], [b % 4 for b in range(B)]
    first = ops.sample_logits(logits, *cols, seeds=seeds, steps=steps)
    assert torch.equal(first, ops.sample_logits(logits, *cols, seeds=seeds, steps=steps))
    perm = torch.randperm(B, generator=g)
    pl = perm.tolist()
    moved = ops.sample_logits(logits[perm.cuda()], *[[c[i] for i in pl] for c in cols], seeds=[seeds[i] for i in pl],
                              steps=[steps[i] for i in pl])
    assert torch.equal(moved, first[perm.cuda()])
    for b in (0, 5, 17, 32):
        alone = ops.sample_logits(logits[b:b + 1], *[c[b] for c in cols], seeds=seeds[b], steps=steps[b])
        assert int(alone[0]) == int(first[b])


@gpu
def test_fallbacks():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 300, generator=g) * 4
    args = ([0.0, 0.8, 1.0, 0.7, 1.2], [0, 20, 0, 0, 4], [1.0, 0.9, 0.8, 1.0, 0.6], [0.0, 0.0, 0.0, 0.1, 0.0])
    seeds, steps = [1, 2, 3, 4, 5], [0, 1, 2, 3, 4]
    half = x.half().cuda()
    assert not ops.sample_logits_supported(half)
    got = ops.sample_logits(half, *args, seeds=seeds, steps=steps)
    assert got.is_cuda and torch.equal(got.cpu(), ref.sample_logits_ref(x.half(), *args, seeds, steps))
    strided = x.cuda()[:, ::2]
    assert not ops.sample_logits_supported(strided)
    got = ops.sample_logits(strided, *args, seeds=seeds, steps=steps)
    assert torch.equal(got.cpu(), ref.sample_logits_ref(x[:, ::2], *args, seeds, steps))
    empty = ops.sample_logits(torch.empty(0, 300, device="cuda", dtype=torch.bfloat16), 0.8)
    assert empty.shape == (0,) and empty.dtype == torch.int64 and empty.is_cuda


@gpu
def test_engine_end_to_end():
    from ray_community_amd.models import GenerationEngine, build_llama

    torch.manual_seed(0)
    model = build_llama("llama3-tiny", device="cuda", dtype=torch.bfloat16).eval()
    V = model.cfg.vocab_size
    prompts = [[5, 9, 200, 31], [5, 9, 200, 31], [77, 3], [400, 401, 402, 403, 404]]
    seeds = [11, 11, 12, 13]

    def run():
        eng = GenerationEngine(model, max_slots=4, num_blocks=32, fused_sampling=True)
        rids = [eng.add_request(p, 12, temperature=0.9, top_p=0.9, seed=s) for p, s in zip(prompts, seeds)]
        out = {r: [] for r in rids}
        while eng.has_work():
            for rid, tok, _ in eng.step():
                out[rid].append(tok)
        return [out[r] for r in rids]

    a = run()
    assert all(len(s) == 12 and all(0 <= t < V for t in s) for s in a)
    assert a == run()
    assert a[0] == a[1]
    assert len({tuple(s) for s in a}) > 1
