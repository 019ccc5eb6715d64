"""The hand-written bf16 GEMM (ops/csrc/gemm.hip, gemm4.hip, gemm_common.h) and its two fused epilogues
-- EPI 1, SwiGLU backward (``rca_gemm_swiglu_bwd``) and EPI 2, affine + residual + ReLU
(``rca_gemm_affine_act``) -- checked per element against float64 oracles written here, independent of
ops/reference.py and of torch.matmul in low precision, on strided, NaN-padded operand views and an
output view surrounded by guard bands.

Oracle. S = A64 @ B64^T and P = |A64| @ |B64|^T in float64 on the CPU from the bf16 operand values (exact
in fp64), cached per case.

Bounds: per element, derived, none taken from a kernel.
    plain         |got - S| <= 2**-8 |S| + K 2**-24 P + TINY
    accumulating  the same with S + base for S, plus 2**-24 |S + base| (the fp32 add); base is the bf16 C
    EPI 2         pre = S + shift[n] (+ res[m][n]); the plain bound on pre plus 2**-23 |pre| (two fp32
                  adds); with ReLU got >= 0 everywhere and got == 0 where pre < -bound
    EPI 1         want = dh * factor, dh = S; 2**-8 |want| + |factor| H 2**-24 P + REL_F |want| + TINY
2**-8 |S| is half a bf16 ulp under round-to-nearest-even (its worst case, a result just above a power of
two, is exact), K 2**-24 P the standard fp32 accumulation bound, TINY = 2**-126 (the smallest normal
bf16) times max(1, case magnitude): a flushed denormal may come back as zero and nothing else is
excused. The case magnitude is the largest operand or base magnitude of a GEMM case; for EPI 1 it is
max |dh| * max (1 + |g|) max(1, |u|), because below g = -87.3 the fp32 sigmoid is itself a denormal
(or, past the overflow of exp at 88.7, zero) and the factor's absolute error there is at most 2**-126
(1 + |g|) |u| (``test_bounds_are_twice_the_measured_floors`` checks that figure).

EPI 1 factors (gemm4.hip, swiglu_bwd_epilogue): dg = dh * u * s * (1 + g (1 - s)) and du = dh * bf16(g s),
the one documented rounding (``const bf16_t dub = f2bf(d * bf2f(f2bf(si)))``, gemm4.hip:626). REL_F covers
the fp32 evaluation of the factor with __expf: the ``emulate`` mode of ``_epi1_factors`` evaluates the
factor in fp32 with exp(-g) = exp2(fp32(-g * log2 e)) rounded to fp32 and moved by -1, 0 and +1 fp32 steps
(the fast exponential's documented error); REL_F is twice its worst relative deviation from the fp64
factor over every gate of this file whose sigmoid is a normal fp32 number, rounded up to a power of two.
For du the quantity is the fp32 g s BEFORE its one bf16 rounding: after it the emulated factor equals the
exact one everywhere except where the exact g s lies within REL_F of the midpoint of two bf16 values
(g = -2**-8 is such a gate: 1462 of 393 216 gate elements), and there, and nowhere else, the checker
accepts either neighbour (``_silu_ties``). The dg floor is set by gates near g = -1.278, where 1 + g (1 -
s) crosses zero and the factor cancels.

    factor   floor      REL_F
    dg       3.47e-05   2**-13 = 1.22e-04
    du       1.26e-06   2**-18 = 3.81e-06

Data. Every case is built on the CPU from a seeded generator. ``coded``: randn plus terms that differ per
row of A, per row of B and along k. ``exact``: entries of {-1, 0, 1}, rows of A scaled by 2**(m % 7 - 3),
K <= 256, base = small non-zero integers times the row scale: every partial sum and the result are exact
in fp32 and bf16 and the output must equal the oracle bit for bit. ``binades``: rows of A scaled by 2**e,
e cycling over -20..20, rows of B ([N][K]: the columns of the product) over -6..6. ``nonfinite``: one
+inf in A, one NaN in B, no zeros anywhere: row m* of C is +-inf with the sign of B[n][k*] except
C[m*][n*] = NaN, column n* is NaN, everything else is inside its bound. EPI 1 gates: two rows of 4 *
randn, then one row of {0, -0, +-2**-20, +-1, +-8, +-30, +-88, +-90, +-120} walked over the columns with
a shift that advances per row, so each value meets every lane group and register slot of a wave tile.

Views. A, B and C are ``buf[2 : 2 + rows, c0 : c0 + cols]`` of larger allocations with (row stride -
cols, c0) from (8, 0), (72, 8), (264, 64), a different pair for each of the three in one call, k-major
operands included. Operand padding is NaN; the C allocation holds a sentinel bit pattern (a function of
the flat index) that must be bit-identical outside the view after plain and accumulating calls.

The tests without a ``gpu`` mark run anywhere: they recompute REL_F, run an fp32 emulation of the GEMM
(fp32 accumulation over K in 32-deep chunks, one bf16 rounding) through every case the GPU tests run
(worst share of the bound 0.99; ``exact`` bit for bit), and show that the checkers reject every slip
listed in ``test_checker_rejects_*``.

Host contract. ``rca_gemm_swiglu_bwd`` and ``rca_gemm_affine_act`` did not check their base pointers (a
view starting 8 bytes off a 16-byte boundary went to the LDS-DMA as it was); they now return -2 for it
before any launch, as ``rca_gemm_bf16`` does. Found by reading, before any device run.

Measured on one MI355X (the whole file, CPU tests included, takes 9 s on the device, 127 tests; the
slowest GPU test, test_gemm_rows_coded[0-(False, False)], 0.35 s), worst share of the bound per GPU test:
    test_gemm_rows_coded                         0.99 for every variant and layout
    test_gemm_rows_exact_binades_nonfinite       exact: bit for bit; binades 0.99; nonfinite 0.99
    test_gemm_schedule_variants_accumulate_...   71-78 accumulating equal 7 bit for bit
    test_gemm_swiglu_bwd_rows                    dg 0.96  du 0.99, dgu_t = dgu^T bit for bit
    test_conv1x1_affine_act_rows                 0.98
The share is set by the rounding term in every test: an element just above a power of two whose rounding
error is nearly half a bf16 ulp (the fp32 emulation reaches the same 0.99 on the CPU). Nothing failed on
the device: every variant, layout and epilogue passed at the first run, guard bands and NaN padding
included.
"""
import functools
import math

import pytest
import torch

from ray_community_amd import ops

gpu = pytest.mark.gpu

TINY = 2.0 ** -126
NAN = float("nan")
PADS = [(8, 0), (72, 8), (264, 64)]  # (row stride - cols, c0)
SLACK = 2                            # rows of the allocation before and after a view
REL_F = {"dg": 2.0 ** -13, "du": 2.0 ** -18}
LAYOUTS = [(False, False), (False, True), (True, True), (True, False)]  # (a_kmaj, b_kmaj)
VARIANTS = [0, 2, 3, 5, 6, 7, 71, 72, 73, 74, 75, 76, 77, 78]
ROWROW_ONLY = [v for v in VARIANTS if v >= 6]  # mixed layouts are their documented fallback to 3
GRIDS = [(256, 256), (256, 768), (768, 256), (768, 768), (1280, 768), (2304, 512), (2560, 256)]
KS = [64, 128, 192, 256, 448, 1152]
SHAPES = sorted({(M, N, K) for M, N in [(256, 256), (768, 768)] for K in KS}
                | {(M, N, K) for M, N in GRIDS for K in (128, 192)})
MIXED = [(768, 768, 128), (256, 256, 192), (2304, 512, 128)]      # fallback of the row/row-only variants
EXTRA = {
    "exact": [(256, 256, 64), (768, 768, 256), (2304, 512, 192), (1280, 768, 128)],
    "binades": [(768, 768, 128), (256, 256, 1152), (2560, 256, 192), (768, 768, 448)],
    "nonfinite": [(768, 768, 128), (256, 768, 192)],
}
KINDS = ["coded", "exact", "binades", "nonfinite"]


def _bf(x):
    """Round to bf16 (RNE), keep the dtype."""
    return x.bfloat16().to(x.dtype)


def _gen(*ints):
    seed = 0
    for v in ints:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def _operands(kind, M, N, K):
    """Logical A [M][K], B [N][K] and the accumulating base [M][N], bf16, on the CPU."""
    g = _gen(KINDS.index(kind), M, N, K)
    m = torch.arange(M, dtype=torch.float64)[:, None]
    n = torch.arange(N, dtype=torch.float64)[:, None]
    k = torch.arange(K, dtype=torch.float64)[None, :]
    sa, sb = torch.ones(M, 1, dtype=torch.float64), torch.ones(N, 1, dtype=torch.float64)
    sign = torch.where(torch.rand(M, N, generator=g) < 0.5, -1.0, 1.0).double()
    if kind == "exact":
        assert K <= 256
        sa = 2.0 ** (m % 7 - 3)
        A = torch.randint(-1, 2, (M, K), generator=g).double() * sa
        B = torch.randint(-1, 2, (N, K), generator=g).double()
        base = sign * torch.randint(1, 9, (M, N), generator=g).double() * sa
    else:
        if kind == "binades":
            sa, sb = 2.0 ** (m % 41 - 20), 2.0 ** (n % 13 - 6)
        A = torch.randn(M, K, generator=g).double()
        B = torch.randn(N, K, generator=g).double()
        if kind != "binades":
            A = A + 0.5 * torch.sin(0.37 * m + 0.11 * k)
            B = B - 0.4 * torch.cos(0.23 * n + 0.05 * k)
        A, B = A * sa, B * sb
        base = sign * (0.5 + torch.rand(M, N, generator=g).double()) * math.sqrt(K) * sa * sb.t()
    c = dict(A=A.bfloat16(), B=B.bfloat16(), base=base.bfloat16(), kind=kind, M=M, N=N, K=K)
    if kind == "exact":
        for t, name in ((A, "A"), (B, "B"), (base, "base")):
            assert torch.equal(c[name].double(), t), name
    if kind == "nonfinite":
        for name in ("A", "B"):
            c[name][c[name] == 0] = 1.0
        c.update(ms=M - 37, ks=K - 5, ns=70, kn=3)
        c["bsign"] = torch.sign(c["B"][:, c["ks"]].double())
        c["A"][c["ms"], c["ks"]] = float("inf")
        c["B"][c["ns"], c["kn"]] = NAN
        assert (c["A"] != 0).all() and (c["B"] != 0).all()
        assert int(torch.isinf(c["A"]).sum()) == 1 and int(torch.isnan(c["B"]).sum()) == 1
        assert not torch.isnan(c["A"]).any() and not torch.isinf(c["B"]).any()
    else:
        assert torch.isfinite(c["A"]).all() and torch.isfinite(c["B"]).all()
    fin = [t[torch.isfinite(t)].abs().max().item() for t in (c["A"].double(), c["B"].double(), c["base"].double())]
    c["mag"] = max(fin)
    return c


@functools.lru_cache(maxsize=None)
def _oracle(kind, M, N, K):
    """S, P in fp64. ``nonfinite``: with the inf and the NaN replaced by 1, which no element outside
    row m* and column n* can see."""
    c = _operands(kind, M, N, K)
    A, B = c["A"].double().clone(), c["B"].double().clone()
    if kind == "nonfinite":
        A[c["ms"], c["ks"]] = 1.0
        B[c["ns"], c["kn"]] = 1.0
    S, P = A @ B.t(), A.abs() @ B.abs().t()
    if kind == "exact":
        assert torch.equal(_bf(S), S) and torch.equal(_bf(S + c["base"].double()), S + c["base"].double())
    return S, P


def _want_bound(kind, M, N, K, accumulate):
    c = _operands(kind, M, N, K)
    S, P = _oracle(kind, M, N, K)
    want = S + c["base"].double() if accumulate else S
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -24 * P + TINY * max(1.0, c["mag"])
    if accumulate:
        bound = bound + 2.0 ** -24 * want.abs()
    return want, bound


def _fails(kind, M, N, K, got, accumulate):
    """[M][N] bool, True where ``got`` (bf16, CPU) is rejected, and the largest share of the bound used
    by the elements the bound applies to. NaN where a number is due is a failure."""
    c = _operands(kind, M, N, K)
    want, bound = _want_bound(kind, M, N, K, accumulate)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    g64 = got.double()
    if kind == "exact":
        fail = got.contiguous().view(torch.int16) != want.bfloat16().view(torch.int16)
        return fail, float(fail.any())
    diff = (g64 - want).abs()
    fail = ~(diff <= bound)
    ratio = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff / bound)
    if kind == "nonfinite":
        ms, ns = c["ms"], c["ns"]
        fail[ms, :] = ~(torch.isinf(g64[ms]) & (torch.sign(g64[ms]) == c["bsign"]))
        fail[:, ns] = ~torch.isnan(g64[:, ns])
        ratio[ms, :] = 0.0
        ratio[:, ns] = 0.0
    return fail, float(ratio.max())


# ----------------------------------------------------------------------------------------- views
def _embed(x, pad, c0):
    """x [rows][cols] -> (NaN-filled allocation, the view of it that holds x)."""
    rows, cols = x.shape
    buf = torch.full((rows + 2 * SLACK, cols + pad), NAN, dtype=torch.bfloat16)
    buf[SLACK:SLACK + rows, c0:c0 + cols] = x
    return buf, _view(buf, rows, cols, c0)


def _view(buf, rows, cols, c0):
    v = buf[SLACK:SLACK + rows, c0:c0 + cols]
    assert v.data_ptr() % 16 == 0 and v.stride(0) != cols and v.stride(0) % 8 == 0 and v.stride(1) == 1
    return v


def _sentinel(rows, width):
    idx = torch.arange(rows * width, dtype=torch.int64)
    bits = (idx * 40503 + 0x1234) & 0xFFFF
    return (bits - ((bits >> 15) << 16)).to(torch.int16).view(rows, width)


def _guard_intact(after, M, N, c0):
    """``after``: the whole C allocation (bf16, CPU) after a call; every element outside the view is
    bit-identical to the sentinel."""
    keep = torch.ones(after.shape, dtype=torch.bool)
    keep[SLACK:SLACK + M, c0:c0 + N] = False
    return torch.equal(after.view(torch.int16)[keep], _sentinel(*after.shape)[keep])


def _run_case(run, kind, M, N, K, layout, sel, accumulate):
    """One call of ``run(abuf, bbuf, cbuf, geometry)`` on the case's strided views; asserts the guard
    bands and the per-element bound, returns the share of the bound."""
    a_kmaj, b_kmaj = layout
    c = _operands(kind, M, N, K)
    A = c["A"].t().contiguous() if a_kmaj else c["A"]
    B = c["B"].t().contiguous() if b_kmaj else c["B"]
    (pa, ca), (pb, cb), (pc, cc) = PADS[sel % 3], PADS[(sel + 1) % 3], PADS[(sel + 2) % 3]
    abuf, _ = _embed(A, pa, ca)
    bbuf, _ = _embed(B, pb, cb)
    cbuf = _sentinel(M + 2 * SLACK, N + pc).view(torch.bfloat16).clone()
    if accumulate:
        cbuf[SLACK:SLACK + M, cc:cc + N] = c["base"]
    geo = dict(a=(A.shape[0], A.shape[1], ca), b=(B.shape[0], B.shape[1], cb), c=(M, N, cc),
               a_kmaj=a_kmaj, b_kmaj=b_kmaj, accumulate=accumulate)
    after = run(abuf, bbuf, cbuf, geo)
    label = (kind, M, N, K, layout, sel, accumulate)
    assert _guard_intact(after, M, N, cc), (label, "guard band written")
    fail, share = _fails(kind, M, N, K, after[SLACK:SLACK + M, cc:cc + N], accumulate)
    assert not fail.any(), (label, int(fail.sum()), int(fail.flatten().int().argmax()), share)
    return share


def _emulate(abuf, bbuf, cbuf, geo):
    """A correct kernel on the CPU: fp32 accumulation over K in 32-deep chunks, one bf16 rounding."""
    a, b, cv = _view(abuf, *geo["a"]), _view(bbuf, *geo["b"]), _view(cbuf, *geo["c"])
    A = (a.t() if geo["a_kmaj"] else a).float()
    B = (b.t() if geo["b_kmaj"] else b).float()
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    for k0 in range(0, A.shape[1], 32):
        acc += A[:, k0:k0 + 32] @ B[:, k0:k0 + 32].t()
    if geo["accumulate"]:
        acc += cv.float()
    cv.copy_(acc.bfloat16())
    return cbuf


def _gpu_gemm(abuf, bbuf, cbuf, geo):
    abuf, bbuf, cbuf = abuf.cuda(), bbuf.cuda(), cbuf.cuda()
    a, b, cv = _view(abuf, *geo["a"]), _view(bbuf, *geo["b"]), _view(cbuf, *geo["c"])
    assert len({a.stride(0) - a.shape[1], b.stride(0) - b.shape[1], cv.stride(0) - cv.shape[1]}) == 3
    out = ops.gemm(a, b, geo["a_kmaj"], geo["b_kmaj"], out=cv, accumulate=geo["accumulate"])
    assert out.data_ptr() == cv.data_ptr()
    return cbuf.cpu()


def _sel(M, N, K, layout):
    return SHAPES.index((M, N, K)) + LAYOUTS.index(layout)


def _coded_shapes(variant, layout):
    if variant in ROWROW_ONLY and layout != LAYOUTS[0]:
        return MIXED
    return SHAPES


def _mixed_layout(variant):
    return LAYOUTS[1 + ROWROW_ONLY.index(variant) % 3]


CODED_RUNS = [(v, lay) for v in VARIANTS for lay in (LAYOUTS if v < 6 else [LAYOUTS[0], _mixed_layout(v)])]


def _extra_layouts(variant):
    return LAYOUTS if variant < 6 else LAYOUTS[:1]


def _all_gpu_cases():
    """Every (kind, M, N, K, layout) the GPU tests run, each plain and accumulating."""
    seen = []
    for v, lay in CODED_RUNS:
        seen += [("coded",) + s + (lay,) for s in _coded_shapes(v, lay)]
    for v in VARIANTS:
        for kind, shapes in EXTRA.items():
            seen += [(kind,) + s + (lay,) for s in shapes for lay in _extra_layouts(v)]
    return sorted(set(seen))


# ============================================================================ EPI 1: SwiGLU backward
EPI1 = [(256, 128, 256), (512, 384, 256), (256, 256, 768)]  # T, H, F
SPECIAL = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, 8.0, -8.0, 30.0, -30.0, 88.0, -88.0, 90.0, -90.0, 120.0, -120.0]
LOG2E = 1.4426950408889634


@functools.lru_cache(maxsize=None)
def _epi1_case(T, H, F):
    g = _gen(11, T, H, F)
    dy = torch.randn(T, H, generator=g).bfloat16()
    w_t = torch.randn(F, H, generator=g).bfloat16()
    gate = 4.0 * torch.randn(T, F, generator=g)
    r, col = torch.arange(T)[:, None], torch.arange(F)[None, :]
    special = torch.tensor(SPECIAL)[(col + r // 3) % len(SPECIAL)]
    gate = torch.where((r % 3 == 2).expand(T, F), special, gate)
    up = torch.randn(T, F, generator=g)
    gu = torch.cat([gate, up], dim=1).bfloat16()
    assert (gu[2, :16].view(torch.int16) == torch.tensor(SPECIAL).bfloat16().view(torch.int16)).all()  # -0.0 kept
    return dy, w_t, gu


def _epi1_factors(gu, emulate=False, unrounded=False, ulp=0):
    """(factor of dg, factor of du), fp64 values. emulate: every operation in fp32, exp(-g) as
    exp2(fp32(-g * log2 e)) (the fast exponential) moved ``ulp`` fp32 steps (its documented error is one),
    g s rounded to bf16 from fp32; a third value, the fp32 g s before that rounding, is returned too."""
    F = gu.shape[1] // 2
    if emulate:
        g, u = gu[:, :F].float(), gu[:, F:].float()
        e = torch.exp2((-g * torch.tensor(LOG2E, dtype=torch.float32)).double()).float()
        for _ in range(abs(ulp)):
            e = torch.nextafter(e, torch.full_like(e, float("inf") if ulp > 0 else 0.0))
        sg = 1.0 / (1.0 + e)
        return ((u * sg) * (1.0 + g * (1.0 - sg))).double(), _bf(g * sg).double(), (g * sg).double()
    g, u = gu[:, :F].double(), gu[:, F:].double()
    sg = torch.sigmoid(g)
    si = g * sg
    return u * sg * (1.0 + g * (1.0 - sg)), si if unrounded else _bf(si)


def _silu_ties(gu):
    """Where the exact g s lies within REL_F["du"] (relative) of the midpoint of two bf16 values, the fp32
    evaluation may round to either: (mask, the other neighbour). Nowhere else is a second value accepted."""
    F = gu.shape[1] // 2
    g = gu[:, :F].double()
    si = g * torch.sigmoid(g)
    near = _bf(si)
    step = 2.0 ** (torch.floor(torch.log2(si.abs().clamp_min(TINY))) - 7)  # bf16 spacing in si's binade
    other = torch.where(si.abs() >= near.abs(), near + torch.sign(si) * step, near - torch.sign(si) * step)
    mid = (near + other) / 2
    return (si != 0) & ((si - mid).abs() <= REL_F["du"] * si.abs()), other


@functools.lru_cache(maxsize=None)
def _epi1_want(T, H, F):
    """{name: [(want, bound), ...]}, fp64: dg has one admissible value per element, du a second one at
    the elements of ``_silu_ties``."""
    dy, w_t, gu = _epi1_case(T, H, F)
    S, P = dy.double() @ w_t.double().t(), dy.double().abs() @ w_t.double().abs().t()
    g, u = gu[:, :F].double(), gu[:, F:].double()
    tiny = TINY * max(1.0, float(S.abs().max()) * float(((1 + g.abs()) * u.abs().clamp_min(1.0)).max()))

    def wb(name, f):
        want = S * f
        return want, 2.0 ** -8 * want.abs() + f.abs() * H * 2.0 ** -24 * P + REL_F[name] * want.abs() + tiny

    fg, fu = _epi1_factors(gu)
    tie, other = _silu_ties(gu)
    alt_w, alt_b = wb("du", other)
    return {"dg": [wb("dg", fg)], "du": [wb("du", fu), (alt_w, torch.where(tie, alt_b, torch.full_like(alt_b, -1.0)))]}


def _epi1_fails(T, H, F, dgu):
    """dgu [T][2F] bf16 CPU -> {name: (fail mask, share)}."""
    w = _epi1_want(T, H, F)
    res = {}
    for name, got in (("dg", dgu[:, :F]), ("du", dgu[:, F:])):
        ratio = None
        for want, bound in w[name]:
            diff = (got.double() - want).abs()
            r = torch.where(torch.isnan(diff) | (bound < 0), torch.full_like(diff, float("inf")), diff / bound)
            ratio = r if ratio is None else torch.minimum(ratio, r)
        res[name] = (~(ratio <= 1.0), float(ratio.max()))
    return res


def _epi1_floors():
    worst = {"dg": 0.0, "du": 0.0}
    sub = 0.0  # largest |emulated - exact| / (2**-126 (1 + |g|) max(1, |u|)) where the sigmoid is below fp32 normal
    ties = 0
    for T, H, F in EPI1:
        gu = _epi1_case(T, H, F)[2]
        g, u = gu[:, :F].double(), gu[:, F:].double()
        normal = torch.sigmoid(g) >= TINY
        xg, xu = _epi1_factors(gu)
        xs = _epi1_factors(gu, unrounded=True)[1]
        tie, other = _silu_ties(gu)
        ties += int(tie.sum())
        for ulp in (-1, 0, 1):
            mg, mu, ms = _epi1_factors(gu, emulate=True, ulp=ulp)
            # dg: the factor; du: the fp32 g s before its one bf16 rounding
            for name, x, m in (("dg", xg, mg), ("du", xs, ms)):
                live = normal & (x != 0)
                worst[name] = max(worst[name], float(((m - x).abs() / x.abs())[live].max()))
                assert bool((m[normal & (x == 0)] == 0).all())
                sub = max(sub, float(((m - x).abs() / (TINY * (1 + g.abs()) * u.abs().clamp_min(1.0)))[~normal].max()))
            # the rounded factor is the exact one, or at a tie its other neighbour
            assert bool(((mu == xu) | (tie & (mu == other)))[normal].all()), (T, H, F, ulp)
    return worst, sub, ties


# ============================================================================ EPI 2: affine + act
EPI2 = [(1, 128, 256, 16), (4, 384, 512, 8), (16, 256, 768, 4)]  # N, Cin, Cout, HW


@functools.lru_cache(maxsize=None)
def _epi2_case(Nb, Cin, Cout, HW):
    g = _gen(12, Nb, Cin, Cout, HW)
    x = torch.randn(Nb, Cin, HW, HW, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    w = torch.randn(Cout, Cin, 1, 1, generator=g).bfloat16()
    shift = (3.0 * torch.randn(Cout, generator=g) + 0.01 * torch.arange(Cout)).float()
    res = (5.0 * torch.randn(Nb, Cout, HW, HW, generator=g)).bfloat16().contiguous(memory_format=torch.channels_last)
    return x, w, shift, res


@functools.lru_cache(maxsize=None)
def _epi2_sp(Nb, Cin, Cout, HW):
    x, w, _, _ = _epi2_case(Nb, Cin, Cout, HW)
    A, B = x.permute(0, 2, 3, 1).reshape(-1, Cin).double(), w.reshape(Cout, Cin).double()
    return A @ B.t(), A.abs() @ B.abs().t()


def _epi2_pre(case, with_res, shift_by_m=False):
    _, _, shift, res = _epi2_case(*case)
    S, P = _epi2_sp(*case)
    M, Cout = S.shape
    sh = shift.double()
    pre = S + (sh[torch.arange(M) % Cout][:, None] if shift_by_m else sh[None, :])
    if with_res:
        pre = pre + res.permute(0, 2, 3, 1).reshape(M, Cout).double()
    mag = max(1.0, float(sh.abs().max()), float(res.double().abs().max()))
    return pre, 2.0 ** -8 * pre.abs() + case[1] * 2.0 ** -24 * P + 2.0 ** -23 * pre.abs() + TINY * mag


def _epi2_fails(case, got, with_res, relu):
    """got [M][Cout] bf16 CPU -> (fail mask, share)."""
    pre, bound = _epi2_pre(case, with_res)
    g64 = got.double()
    want = pre.clamp_min(0) if relu else pre
    diff = (g64 - want).abs()
    fail = ~(diff <= bound)
    if relu:
        fail |= ~(g64 >= 0) | ((pre < -bound) & (g64 != 0))
    return fail, float(torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff / bound).max())


# ================================================================================ CPU tests: the bounds
def test_bounds_are_twice_the_measured_floors():
    worst, sub, ties = _epi1_floors()
    for name in REL_F:
        print(f"    {name}       {worst[name]:.2e}   2**{math.log2(REL_F[name]):.0f} = {REL_F[name]:.2e}")
    print(f"    denormal-sigmoid gates: {sub:.2f} of 2**-126 (1 + |g|) max(1, |u|); elements at a bf16 tie: {ties}")
    for name in REL_F:
        assert 0 < worst[name] <= REL_F[name] / 2, (name, worst[name])
        assert REL_F[name] == 2.0 ** math.ceil(math.log2(2 * worst[name])), (name, worst[name])
    assert sub <= 1.0, sub


def test_shape_matrix_reaches_every_path():
    assert len(SHAPES) == 22 and all(M % 256 == 0 and N % 256 == 0 and K % 64 == 0 for M, N, K in SHAPES)
    for K in KS:
        assert (256, 256, K) in SHAPES and (768, 768, K) in SHAPES
    for M, N in GRIDS:
        assert (M, N, 128) in SHAPES and (M, N, 192) in SHAPES
    assert all((768, 768, K) in _coded_shapes(v, LAYOUTS[0]) for v in VARIANTS for K in KS)
    assert {_mixed_layout(v) for v in ROWROW_ONLY} == set(LAYOUTS[1:])
    for case in EPI2:
        assert case[0] * case[3] ** 2 % 256 == 0


@pytest.mark.parametrize("kind", KINDS)
def test_fp32_emulation_passes_every_gpu_case(kind):
    """The bound is reachable by a correct kernel: the fp32 emulation, run through the same strided
    views, guard bands and checks as the GPU calls, passes every case of the GPU tests."""
    worst = 0.0
    for case in (c for c in _all_gpu_cases() if c[0] == kind):
        k, M, N, K, lay = case
        for accumulate in (False, True):
            worst = max(worst, _run_case(_emulate, k, M, N, K, lay, _sel(M, N, K, lay), accumulate))
    print(f"emulation, {kind}: worst share of the bound {worst:.2f}")


# ======================================================================= CPU tests: the checkers' teeth
TEETH = (1280, 768, 192)  # 5 x 3 tiles, three 64-deep K-tiles


def _tile(tm, tn):
    return slice(tm * 256, tm * 256 + 256), slice(tn * 256, tn * 256 + 256)


def _only_in(fail, rows, cols):
    other = fail.clone()
    other[rows, cols] = False
    return bool(fail[rows, cols].any()) and not bool(other.any())


@pytest.mark.parametrize("kind", ["coded", "binades", "exact"])
def test_checker_rejects_kslice_chunk_block_tile_and_base_slips(kind):
    M, N, K = TEETH
    c = _operands(kind, M, N, K)
    A, B, base = c["A"].double(), c["B"].double(), c["base"].double()
    S = _oracle(kind, M, N, K)[0]
    good = S.bfloat16()
    assert not _fails(kind, M, N, K, good, False)[0].any()
    assert not _fails(kind, M, N, K, (S + base).bfloat16(), True)[0].any()

    # one 32-deep K-slice dropped / counted twice for one 128 x 128 wave tile
    rows, cols, ks = slice(640, 768), slice(384, 512), slice(96, 128)
    part = A[rows, ks] @ B[cols, ks].t()
    for sgn in (-1.0, 1.0):
        bad = S.clone()
        bad[rows, cols] += sgn * part
        fail = _fails(kind, M, N, K, bad.bfloat16(), False)[0]
        assert _only_in(fail, rows, cols), (kind, "k-slice", sgn)
        if kind != "exact":
            assert float(fail[rows, cols].double().mean()) > 0.9, (kind, "k-slice", sgn)

    # two adjacent 8-element k-chunks swapped in A only, one 256-row tile, one 64-deep K-tile
    A2 = A.clone()
    A2[512:768, 64:72], A2[512:768, 72:80] = A[512:768, 72:80], A[512:768, 64:72]
    fail = _fails(kind, M, N, K, (A2 @ B.t()).bfloat16(), False)[0]
    assert not fail[:512].any() and not fail[768:].any()
    for tn in range(N // 256):
        assert fail[_tile(2, tn)].any(), (kind, "k-chunks", tn)

    # two 16-row blocks of one output tile exchanged
    bad = good.clone()
    bad[256 + 32:256 + 48, 512:768], bad[256 + 160:256 + 176, 512:768] = \
        good[256 + 160:256 + 176, 512:768], good[256 + 32:256 + 48, 512:768]
    fail = _fails(kind, M, N, K, bad, False)[0]
    assert _only_in(fail, slice(256, 512), slice(512, 768))
    assert fail[256 + 32:256 + 48, 512:768].any(1).all() and fail[256 + 160:256 + 176, 512:768].any(1).all()

    # one output tile written at the transposed tile coordinates (5 x 3 grid): tiles (1, 2) and (2, 1)
    bad = good.clone()
    bad[_tile(2, 1)], bad[_tile(1, 2)] = good[_tile(1, 2)], good[_tile(2, 1)]
    fail = _fails(kind, M, N, K, bad, False)[0]
    assert fail[_tile(2, 1)].any() and fail[_tile(1, 2)].any()
    fail[_tile(2, 1)] = False
    fail[_tile(1, 2)] = False
    assert not fail.any()

    # base added twice / not at all in one 4-element store: every one of the 4 elements
    for mult in (2.0, 0.0):
        bad = S + base
        bad[777, 300:304] = S[777, 300:304] + mult * base[777, 300:304]
        fail = _fails(kind, M, N, K, bad.bfloat16(), True)[0]
        assert fail[777, 300:304].all() and int(fail.sum()) == 4, (kind, "base", mult)


@pytest.mark.parametrize("kind", ["coded", "binades", "exact"])
@pytest.mark.parametrize("sel", [0, 1, 2])
def test_checker_rejects_a_row_stride_of_k_and_a_store_past_the_view(kind, sel):
    M, N, K = TEETH
    c = _operands(kind, M, N, K)
    pad, c0 = PADS[sel]
    abuf, a = _embed(c["A"], pad, c0)
    # row stride K in place of lda: rows 1.. read the padding (NaN) or their neighbours' data
    wrong = torch.as_strided(abuf, (M, K), (K, 1), a.storage_offset())
    assert torch.equal(wrong[0], a[0])
    fail = _fails(kind, M, N, K, (wrong.double() @ c["B"].double().t()).bfloat16(), False)[0]
    assert not fail[0].any() and fail[1:].any(1).all(), (kind, sel, int(fail[1:].any(1).sum()))
    # one 8-byte store landing 4 elements right of the view's last column
    good = _oracle(kind, M, N, K)[0].bfloat16()
    cbuf = _sentinel(M + 2 * SLACK, N + pad).view(torch.bfloat16).clone()
    cbuf[SLACK:SLACK + M, c0:c0 + N] = good
    assert _guard_intact(cbuf, M, N, c0)
    r = SLACK + M - 1
    cbuf[r, c0 + N:c0 + N + 4] = good[M - 1, N - 4:]
    if (cbuf[r, c0 + N:c0 + N + 4].view(torch.int16) == _sentinel(*cbuf.shape)[r, c0 + N:c0 + N + 4]).all():
        cbuf[r, c0 + N] = 1.0  # the stored values happen to be the sentinel's: any other value
    assert not _guard_intact(cbuf, M, N, c0)
    assert not _fails(kind, M, N, K, cbuf[SLACK:SLACK + M, c0:c0 + N], False)[0].any()


def test_nonfinite_checker_wants_the_exact_pattern():
    kind, (M, N, K) = "nonfinite", EXTRA["nonfinite"][0]
    c = _operands(kind, M, N, K)
    good = (c["A"].double() @ c["B"].double().t()).bfloat16()
    assert not _fails(kind, M, N, K, good, False)[0].any()
    ms, ns = c["ms"], c["ns"]
    assert torch.isnan(good[ms, ns]) and int(torch.isnan(good).sum()) == M and int(torch.isinf(good).sum()) == N - 1
    for bad_at, value in (((ms, 5), 1.0), ((ms, 5), -good[ms, 5].item()), ((9, ns), 0.0), ((ms, ns), float("inf")),
                          ((ms - 1, 5), float("inf")), ((9, ns + 1), NAN)):
        bad = good.clone()
        bad[bad_at] = value
        fail = _fails(kind, M, N, K, bad, False)[0]
        assert fail[bad_at] and int(fail.sum()) == 1, (bad_at, value)


@pytest.mark.parametrize("case", EPI1, ids=str)
def test_epi1_checker_rejects_the_unrounded_silu_and_swapped_outputs(case):
    T, H, F = case
    dy, w_t, gu = _epi1_case(*case)
    S = dy.double() @ w_t.double().t()
    fg, fu = _epi1_factors(gu)
    good = torch.cat([S * fg, S * fu], 1).bfloat16()
    assert not any(f.any() for f, _ in _epi1_fails(T, H, F, good).values())
    # the emulated (fp32, fast-exp) factors pass as well
    eg, eu, _ = _epi1_factors(gu, emulate=True)
    res = _epi1_fails(T, H, F, torch.cat([(S.float() * eg.float()), (S.float() * eu.float())], 1).bfloat16())
    assert not any(f.any() for f, _ in res.values()), {k: v[1] for k, v in res.items()}
    print(f"EPI 1 emulation {case}: share dg {res['dg'][1]:.2f} du {res['du'][1]:.2f}")
    # bf16(g s) replaced by the unrounded g s
    raw = _epi1_factors(gu, unrounded=True)[1]
    res = _epi1_fails(T, H, F, torch.cat([S * fg, S * raw], 1).bfloat16())
    assert not res["dg"][0].any() and res["du"][0].any(), int(res["du"][0].sum())
    # gate and up gradients the other way round
    res = _epi1_fails(T, H, F, torch.cat([S * fu, S * fg], 1).bfloat16())
    assert res["dg"][0].any(1).all() and res["du"][0].any(1).all()


@pytest.mark.parametrize("case", EPI2, ids=str)
def test_epi2_checker_rejects_shift_by_row_and_relu_before_the_residual(case):
    M, Cout = _epi2_sp(*case)[0].shape
    res = _epi2_case(*case)[3].permute(0, 2, 3, 1).reshape(M, Cout).double()
    for with_res in (False, True):
        pre = _epi2_pre(case, with_res)[0]
        for relu in (False, True):
            good = (pre.clamp_min(0) if relu else pre).bfloat16()
            assert not _epi2_fails(case, good, with_res, relu)[0].any()
            wrong = _epi2_pre(case, with_res, shift_by_m=True)[0]
            fail = _epi2_fails(case, (wrong.clamp_min(0) if relu else wrong).bfloat16(), with_res, relu)[0]
            assert fail.any(1).all(), (case, with_res, relu, "shift[m]")
        # ReLU before the residual
        early = (_epi2_pre(case, False)[0].clamp_min(0) + res).bfloat16() if with_res else None
        if early is not None:
            assert _epi2_fails(case, early, True, True)[0].any(1).all()
            neg = early.clone()
            neg[3, 7] = -1.0  # a negative output under ReLU, whatever its bound
            assert _epi2_fails(case, neg, True, True)[0][3, 7]


# ========================================================================================= GPU tests
def _with_variant(variant, fn):
    lib = ops.lib()
    prev = lib.rca_gemm_set_variant(variant)
    try:
        return fn()
    finally:
        lib.rca_gemm_set_variant(prev)


@gpu
@pytest.mark.parametrize("variant,layout", CODED_RUNS, ids=str)
def test_gemm_rows_coded(variant, layout):
    def go():
        worst = 0.0
        for M, N, K in _coded_shapes(variant, layout):
            for accumulate in (False, True):
                worst = max(worst, _run_case(_gpu_gemm, "coded", M, N, K, layout, _sel(M, N, K, layout), accumulate))
        return worst

    print(f"variant {variant} {layout}: coded, worst share of the bound {_with_variant(variant, go):.2f}")


@gpu
@pytest.mark.parametrize("kind", list(EXTRA))
@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_rows_exact_binades_nonfinite(variant, kind):
    def go():
        worst = 0.0
        for M, N, K in EXTRA[kind]:
            for layout in _extra_layouts(variant):
                for accumulate in (False, True):
                    worst = max(worst, _run_case(_gpu_gemm, kind, M, N, K, layout, _sel(M, N, K, layout), accumulate))
        return worst

    print(f"variant {variant}: {kind}, worst share of the bound {_with_variant(variant, go):.2f}")


@gpu
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v > 70])
def test_gemm_schedule_variants_accumulate_as_variant_7(variant):
    """71-78 do not accumulate: with ``accumulate`` they run as 7, bit for bit on the same inputs."""
    for M, N, K in [(768, 768, 128), (768, 768, 256), (2304, 512, 128)]:
        outs = []
        for v in (7, variant):
            keep = []

            def run(abuf, bbuf, cbuf, geo):
                keep.append(_gpu_gemm(abuf, bbuf, cbuf, geo))
                return keep[0]

            _with_variant(v, lambda: _run_case(run, "coded", M, N, K, LAYOUTS[0], _sel(M, N, K, LAYOUTS[0]), True))
            outs.append(keep[0].view(torch.int16))
        assert torch.equal(outs[0], outs[1]), (variant, M, N, K)


@gpu
@pytest.mark.parametrize("case", EPI1, ids=str)
def test_gemm_swiglu_bwd_rows(case):
    T, H, F = case
    dy, w_t, gu = _epi1_case(*case)
    sel = EPI1.index(case)
    dbuf, _ = _embed(dy, *PADS[sel % 3])
    wbuf, _ = _embed(w_t, *PADS[(sel + 1) % 3])
    dbuf, wbuf = dbuf.cuda(), wbuf.cuda()
    dv, wv = _view(dbuf, T, H, PADS[sel % 3][1]), _view(wbuf, F, H, PADS[(sel + 1) % 3][1])
    gud = gu.cuda()
    assert ops.gemm_swiglu_bwd_supported(dv, wv, gud)
    dgu, dgu_t = ops.gemm_swiglu_bwd(dv, wv, gud)
    torch.cuda.synchronize()
    assert dgu.dtype == torch.bfloat16 and tuple(dgu.shape) == (T, 2 * F) and tuple(dgu_t.shape) == (2 * F, T)
    dgu, dgu_t = dgu.cpu(), dgu_t.cpu()
    assert torch.equal(dgu_t.view(torch.int16), dgu.t().contiguous().view(torch.int16)), "dgu_t != dgu.t()"
    res = _epi1_fails(T, H, F, dgu)
    print(f"EPI 1 {case}: share of the bound dg {res['dg'][1]:.2f} du {res['du'][1]:.2f}")
    for name, (fail, share) in res.items():
        assert not fail.any(), (case, name, int(fail.sum()), int(fail.flatten().int().argmax()), share)


@gpu
@pytest.mark.parametrize("case", EPI2, ids=str)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_conv1x1_affine_act_rows(case, with_res, relu):
    x, w, shift, res = (t.cuda() for t in _epi2_case(*case))
    assert ops.conv1x1_affine_act_supported(x, w)
    out = ops.conv1x1_affine_act(x, w, shift, res if with_res else None, relu)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (case[0], case[2], case[3], case[3])
    got = out.permute(0, 2, 3, 1).reshape(-1, case[2]).cpu()
    fail, share = _epi2_fails(case, got, with_res, relu)
    print(f"EPI 2 {case} res={with_res} relu={relu}: share of the bound {share:.2f}")
    assert not fail.any(), (case, with_res, relu, int(fail.sum()), int(fail.flatten().int().argmax()), share)


@gpu
def test_gemm_wrapper_and_entry_points_refuse_bad_operands_before_any_launch():
    from ray_community_amd.ops._lib import stream_ptr

    dev = torch.device("cuda")
    lib, st = ops.lib(), stream_ptr(dev)
    big = torch.zeros(600, 600, device=dev, dtype=torch.bfloat16)
    a, b = big[:256, :128], big[256:512, :128]
    sent = _sentinel(260, 520).view(torch.bfloat16).cuda()
    out = sent.clone()
    c = out[:256, :256]
    bad_calls = [
        lambda: ops.gemm(big[:255, :128], b),                 # M % 256
        lambda: ops.gemm(a, big[:257, :128]),                 # N % 256
        lambda: ops.gemm(big[:256, :96], big[256:512, :96]),  # K % 64
        lambda: ops.gemm(torch.zeros(256, 132, device=dev, dtype=torch.bfloat16)[:, :128], b),  # stride % 8
        lambda: ops.gemm(big[:256, 4:132], b),                # base 8 bytes off
        lambda: ops.gemm(a, b, out=out[:256, 4:260]),         # misaligned output
        lambda: ops.gemm(a, b, out=out[:256, :512]),          # out of the wrong shape
        lambda: ops.gemm(a, b, accumulate=True),              # accumulate without out
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    p = lambda t: t.data_ptr()  # noqa: E731
    ok = (256, 256, 128, 600, 600, 520)
    codes = [
        lib.rca_gemm_bf16(p(a), p(b), p(c), 255, 256, 128, 600, 600, 520, 0, 0, 0, st),
        lib.rca_gemm_bf16(p(a), p(b), p(c), 256, 257, 128, 600, 600, 520, 0, 0, 0, st),
        lib.rca_gemm_bf16(p(a), p(b), p(c), 256, 256, 96, 600, 600, 520, 0, 0, 0, st),
        lib.rca_gemm_bf16(p(a), p(b), p(c), 256, 256, 128, 604, 600, 520, 0, 0, 0, st),
        lib.rca_gemm_bf16(p(a), p(b), p(c), 256, 256, 128, 600, 600, 524, 0, 0, 1, st),
        lib.rca_gemm_bf16(p(a) + 8, p(b), p(c), *ok, 0, 0, 0, st),
        lib.rca_gemm_bf16(p(a), p(b), p(c) + 8, *ok, 0, 0, 1, st),
    ]
    # EPI 1: dy [T][H], w_t [F][H], gu / dgu [T][2F], dgu_t [2F][T]
    gu = torch.zeros(256, 512, device=dev, dtype=torch.bfloat16)
    dgu, dgu_t = out.view(-1)[:256 * 512].view(256, 512), torch.zeros(512, 256, device=dev, dtype=torch.bfloat16)
    e1 = lambda dy=p(a), w=p(b), T=256, F=256, H=128, ld=600, ldw=600: lib.rca_gemm_swiglu_bwd(  # noqa: E731
        dy, w, p(gu), p(dgu), p(dgu_t), T, F, H, ld, ldw, st)
    codes += [e1(T=255), e1(F=257), e1(H=64), e1(ld=604), e1(ldw=596), e1(dy=p(a) + 8), e1(w=p(b) + 8)]
    # EPI 2: x [M][K], w [N][K], out [M][N]
    shift = torch.zeros(256, device=dev, dtype=torch.float32)
    e2 = lambda x=p(a), w=p(b), o=p(c), M=256, N=256, K=128, ldx=600, ldw=600, ldo=520: lib.rca_gemm_affine_act(  # noqa: E731
        x, w, p(shift), None, o, M, N, K, ldx, ldw, ldo, 0, 1, st)
    codes += [e2(M=255), e2(N=257), e2(K=64), e2(ldx=604), e2(ldw=596), e2(ldo=522), e2(x=p(a) + 8), e2(w=p(b) + 8),
              e2(o=p(c) + 4)]
    torch.cuda.synchronize()
    assert all(code < 0 for code in codes), codes
    assert torch.equal(out.view(torch.int16), sent.view(torch.int16)), "a refused call wrote its output"
    assert not dgu_t.any()
