"""The memory-bound kernels of the Llama training step -- RMSNorm (ops/csrc/rmsnorm.hip), SwiGLU and
RoPE (ops/csrc/elementwise.hip) and cross-entropy (ops/csrc/loss_optim.hip) -- checked per row, per
column or per element against float64 oracles written here, independent of ops/reference.py and of
autograd.

Metric. Elementwise outputs (RMSNorm y, s, dx, dres; SwiGLU out, dgate, dup; RoPE output and
gradient) are scored per row by ``_row_err`` = max_j |got - want| / max(rowmax |want|, floor_abs),
floor_abs = 2**-126 (the smallest normal bf16) times max(1, the row's input magnitude); an element
whose ``want`` lies under floor_abs may come back as zero (a flushed denormal) and nothing else is
excused. A row is a token of RMSNorm and SwiGLU and one (token, head) of RoPE. rstd is relative, lse
and loss are absolute differences, per row, in fp32. RMSNorm dw is scored per column in the GEMM style:
|got - S| <= 2**-8 |S| + rows * 2**-24 * sum|terms| + 1e-30, S the fp64 sum of the terms dy * bf16(s *
rstd) the backward kernel forms from ITS inputs (s, dy and the rstd the forward kernel wrote, which is
scored on its own). CE dlogits are scored per element: |got - want| <= REL |want| + A |g_row| [j ==
label]. The absolute term exists for the one place the kernels cancel, p - 1 at the label column (p is
fp32 and comes from the fp32 lse); giving it to the label column alone is stricter than giving it to
the row, leaves every other entry with a purely relative bound (REL < 1: an entry written as zero
cannot pass, whatever the median of its row, which ``test_ce_data_cannot_hide_a_zeroed_entry`` checks
to be non-zero) and no kind of row needs the row metric.

Bounds: none is taken from a kernel. Each oracle has an ``emulate`` mode that rounds where the kernel
rounds (the ``_*_oracle`` functions cite the lines); the floor of a quantity is the worst error of that
mode against the exact one over every case of this file, computed on the CPU, and the bound is twice
the floor rounded up to a power of two (``test_bounds_are_twice_the_measured_floors``):

    quantity      floor      bound
    rms.y         9.97e-03   2**-5  = 3.12e-02
    rms.s         3.89e-03   2**-7  = 7.81e-03
    rms.rstd      3.03e-03   2**-7  = 7.81e-03   (relative)
    rms.dx        4.03e-03   2**-6  = 1.56e-02   (dres is the same tensor)
    swiglu.out    6.39e-03   2**-6  = 1.56e-02
    swiglu.dgate  3.79e-03   2**-7  = 7.81e-03
    swiglu.dup    6.48e-03   2**-6  = 1.56e-02
    rope.out      3.89e-03   2**-7  = 7.81e-03
    rope.grad     3.87e-03   2**-7  = 7.81e-03
    ce.lse        7.61e-06   2**-16 = 1.53e-05   (absolute; half an fp32 ulp of the shifted rows' lse = 216)
    ce.loss       7.61e-06   2**-16 = 1.53e-05   (absolute)
    ce.dl_rel     3.89e-03   2**-7  = 7.81e-03   (REL; every entry but the label's)
    ce.dl_a       5.73e-06   2**-16 = 1.53e-05   (A; the label's fp32 probability and what REL leaves over there)

The RMSNorm floors are set by the residual cases at H = 8, where the bf16 rounding of s = x + r moves the
mean of 8 squares (rstd by 3e-3, and y and dx with it); without a residual rstd is exact in this model.

Data. RMSNorm: ``random``; ``spiked`` (row i holds most of its energy in one 8-column vector that walks
over the 64 lanes and the register slots with i; the register-resident widths also have a case of H / 8
rows in which every vector is the heavy one once); ``mixed`` (rows scaled 2**-10, 1, 2**6 in turn, so eps
decides the small rows); the weight is 1 + a non-symmetric function of the column + noise. SwiGLU: gates
4 * randn, and ``exhaustive``: every bf16 bit pattern once as a gate (NaN and inf patterns replaced by
0), in pattern order, so a row spans 8 binades and small gates are not scored against large ones. CE:
the rows of a case cycle through random (3 * randn), peaked with the label on and off the peak, flat,
shifted +200 and -200, and, where the case masks columns, masked rows (-inf over the last columns).
``masked-head`` rows (-inf over the FIRST 8 columns) are this file's own addition: see below.

The tests without a ``gpu`` mark run anywhere. They recompute the floors, check the CE data, and show
that the checkers reject every slipped oracle listed in ``test_*_rejects_*`` at each row, column or
element the slip affects (for a dropped 8-column vector: the rows whose heavy vector it is).

-inf logits. A lane of ce_fwd_kernel / ce_fused_kernel whose first 16-byte vector is all -inf computes
exp(-inf - -inf) = NaN into its running sum. When that is the lane's ONLY vector (-inf over the last 16
columns of V = 1024 or 4096: the ``masked`` rows) its max stays -inf and the wave merge discards the
sum, so those rows were always right. When a finite vector follows (-inf over the first 8 columns of V
= 4104 or 8200: thread 0 holds vectors 0 and 512 / 1024) the NaN survives: lse, loss and the whole
gradient row were NaN. The per-lane loops now skip a vector (and the scalar tail an element) whose
running max is still -inf.

Measured on one MI355X, worst value per GPU test (the whole file, CPU tests included, takes 16 s on the
device, 137 tests; the slowest GPU test 1.2 s):
    test_rmsnorm_rows                      y 8.48e-3  s 3.89e-3  rstd 3.03e-3  dx 3.99e-3, dw within its formula
    test_rmsnorm_rows_over_the_..._cap     y 9.98e-3  s 3.89e-3  rstd 5.62e-4  dx 4.03e-3
    test_swiglu_rows                       out 6.39e-3  dgate 3.79e-3  dup 6.48e-3 (plain and transposing alike)
    test_rope_rows                         out 3.89e-3  grad 3.86e-3
    test_rope_rows_backward_with_...       out 3.86e-3  grad 3.87e-3 (rca_rope_bwd_tr the same)
    test_cross_entropy_rows                lse 7.84e-6  loss 7.61e-6  dlogits 0.50 of an element's bound
    test_cross_entropy_fused_rows          lse 7.52e-6  loss 7.29e-6  dlogits 0.49 of an element's bound
    test_linear_cross_entropy_v1003_...    |loss - want| 4.2e-5 against 1.34e-2
Every kernel sits on its oracle's rounding floor; the largest share of a bound any row used is 0.51 (lse,
V = 1024, a shifted row). Before the -inf guard the ``masked-head`` rows of V = 4104 (both ignore_index
values) and of the fused V = 8200 came back NaN in lse, loss and dlogits; everything else passed as it does
now.
"""
import functools
import math

import pytest
import torch

from ray_community_amd import ops

gpu = pytest.mark.gpu

TINY = 2.0 ** -126  # the smallest normal bf16
EPS = 1e-5
BOUND = {
    "rms.y": 2.0 ** -5, "rms.s": 2.0 ** -7, "rms.rstd": 2.0 ** -7, "rms.dx": 2.0 ** -6,
    "swiglu.out": 2.0 ** -6, "swiglu.dgate": 2.0 ** -7, "swiglu.dup": 2.0 ** -6,
    "rope.out": 2.0 ** -7, "rope.grad": 2.0 ** -7,
    "ce.lse": 2.0 ** -16, "ce.loss": 2.0 ** -16, "ce.dl_rel": 2.0 ** -7, "ce.dl_a": 2.0 ** -16,
}


def _bf(x):
    """Round to bf16 (RNE), keep the dtype."""
    return x.bfloat16().to(x.dtype)


def _gen(*ints):
    seed = 0
    for v in ints:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------ the metrics
def _row_err(got, want, scale=None):
    """[..., n] -> [...]: see the module docstring. ``scale``: the row's input magnitude, [...]."""
    a, b = got.detach().cpu().double(), want.double()
    fa = torch.full(b.shape[:-1], TINY, dtype=torch.float64)
    if scale is not None:
        fa = fa * scale.double().clamp_min(1.0)
    diff = (a - b).abs()
    diff = torch.where((b.abs() < fa[..., None]) & (a == 0), torch.zeros_like(diff), diff)
    return diff.amax(-1) / torch.maximum(b.abs().amax(-1), fa)


def _note(kind, err, label):
    w = float(err.max()) if err.numel() else 0.0
    print(f"{label}: {kind} worst {w:.3e} ({w / BOUND[kind]:.2f} x bound)")


def _check_rows(kind, got, want, label, scale=None, dtype=torch.bfloat16):
    """dtype, shape, finiteness where the oracle is finite, and every row within BOUND[kind]."""
    assert got.dtype == dtype, (label, kind, got.dtype)
    assert tuple(got.shape) == tuple(want.shape), (label, kind, tuple(got.shape))
    assert torch.isfinite(got).all(), (label, kind, "not finite")
    err = _row_err(got, want, scale)
    _note(kind, err, label)
    assert bool((err < BOUND[kind]).all()), (label, kind, float(err.max()), int(err.flatten().argmax()))


def _rel_err(got, want):
    a, b = got.detach().cpu().double(), want.double()
    return (a - b).abs() / b.abs()


def _check_scalar_rows(kind, got, want, label, relative):
    """rstd (relative), lse and loss (absolute): fp32, one value per row."""
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), (label, kind)
    err = _rel_err(got, want) if relative else (got.detach().cpu().double() - want.double()).abs()
    _note(kind, err, label)
    assert bool((err < BOUND[kind]).all()), (label, kind, float(err.max()), int(err.flatten().argmax()))


def _dw_excess(got, terms):
    """Per column: |got - S| - (2**-8 |S| + rows * 2**-24 * sum|terms| + 1e-30); <= 0 passes."""
    rows = terms.shape[0]
    S = terms.sum(0)
    tol = 2.0 ** -8 * S.abs() + rows * 2.0 ** -24 * terms.abs().sum(0) + 1e-30
    return (got.detach().cpu().double() - S).abs() - tol


def _dl_excess(got, want, g_row, labels):
    """Per element: |got - want| - (REL |want| + A |g_row| [j == label]); <= 0 passes. NaN stays NaN."""
    a, b = got.detach().cpu().double(), want.double()
    tol = BOUND["ce.dl_rel"] * b.abs()
    rows = torch.arange(b.shape[0])
    ok = (labels >= 0) & (labels < b.shape[1])
    tol[rows[ok], labels[ok]] += BOUND["ce.dl_a"] * g_row.double().abs()[ok]
    return (a - b).abs() - tol


def _check_dlogits(got, want, g_row, labels, label):
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == tuple(want.shape), label
    assert torch.isfinite(got).all(), (label, "dlogits not finite")
    ex = _dl_excess(got, want, g_row, labels)
    diff = (got.cpu().double() - want).abs()
    used = float((diff / (diff - ex).clamp_min(1e-300)).max())  # diff - ex is the element's bound
    print(f"{label}: dlogits largest share of an element's bound {used:.2f}")
    assert bool((ex <= 0).all()), (label, "dlogits", float(ex.max()), int(ex.flatten().argmax()))


# ================================================================================ RMSNorm
def _rms_oracle(c, emulate=False, drop=None, eps=EPS, norm_of_x=False):
    """x, r (or None), w, dy, ds (or None) -> s, rstd, y, dx (= dres) in fp64, and the dw terms.
    emulate rounds where the kernels do:
      * s = bf16(x + r)                      rmsnorm.hip:35 (pack8) and :86
      * y = bf16(bf16(s * rstd) * w)         rmsnorm.hip:61-62 and :107-108
      * dw terms dy * bf16(s * rstd)         rmsnorm.hip:158, :256 and :332
      * dx = bf16(rstd w dy - c s + ds)      rmsnorm.hip:175-182, :286-293 and :348-355
    The slips: ``drop`` [rows] = index of the 8-column vector each row leaves out of its sum of
    squares; ``eps``; ``norm_of_x`` takes the norm of x where it should be x + r."""
    x, w, dy = c["x"].double(), c["w"].double(), c["dy"].double()
    H = x.shape[1]
    s = x if c["r"] is None else x + c["r"].double()
    if emulate:
        s = _bf(s)
    sq = (x if norm_of_x else s) ** 2
    ss = sq.sum(1)
    if drop is not None:
        ss = ss - sq.view(-1, H // 8, 8).sum(-1).gather(1, drop[:, None])[:, 0]
    rstd = (ss / H + eps) ** -0.5
    n = s * rstd[:, None]
    if emulate:
        n = _bf(n)
    y = n * w
    terms = dy * n
    dot = (s * w * dy).sum(1)
    dx = rstd[:, None] * w * dy - (dot * rstd ** 3 / H)[:, None] * s
    if c["ds"] is not None:
        dx = dx + c["ds"].double()
    if emulate:
        y, dx = _bf(y), _bf(dx)
    return dict(s=s, rstd=rstd, y=y, dx=dx, terms=terms)


def _heavy_vector(rows, H):
    """The vector that carries row i of a spiked case: vector i where the case has a row for every vector,
    else lane i % 64 in slot i % slots while that exists."""
    nvec = H // 8
    i = torch.arange(rows)
    if rows >= nvec:
        return i % nvec
    v = i % 64 + 64 * (i % ((nvec + 63) // 64))
    return torch.where(v < nvec, v, i % nvec)


@functools.lru_cache(maxsize=None)
def _rms_case(kind, rows, H, res):
    g = _gen(1, rows, H, res, len(kind))
    x = torch.randn(rows, H, generator=g)
    r = torch.randn(rows, H, generator=g) if res else None
    if kind == "spiked":
        hv = _heavy_vector(rows, H)
        cols = hv[:, None] * 8 + torch.arange(8)[None, :]
        x.scatter_(1, cols, 64.0 * (1.0 + torch.rand(rows, 8, generator=g)) * (1 - 2 * (cols % 2)))
    elif kind == "mixed":
        sc = torch.tensor([2.0 ** -10, 1.0, 2.0 ** 6])[torch.arange(rows) % 3][:, None]
        x = x * sc
        r = r * sc if res else None
    else:
        assert kind == "random"
    col = torch.arange(H, dtype=torch.float32)
    w = 1.0 + 0.5 * torch.sin(0.37 * col) + 0.25 * col / H + 0.05 * torch.randn(H, generator=g)
    dy = torch.randn(rows, H, generator=g)
    ds = torch.randn(rows, H, generator=g) if res else None
    b = lambda t: None if t is None else t.bfloat16()
    return dict(x=b(x), r=b(r), w=b(w), dy=b(dy), ds=b(ds))


RMS_H = (8, 520, 640, 512, 1024, 2048, 4096, 8192)
RMS_ROWS = (1, 3, 5, 67)
RMS_CASES = [(kind, rows, H, res) for H in RMS_H for rows in RMS_ROWS for kind in ("random", "spiked", "mixed")
             for res in (False, True)]
# a row for every vector of the register-resident widths: each (lane, slot) pair is the heavy one once
RMS_CASES += [("spiked", H // 8, H, res) for H in RMS_H if H % 512 == 0 for res in (False, True)]
# over the backward grid caps: 512 blocks x 16 rows of the LDS-slice kernels, 1024 x 8 of the split ones
RMS_BIG = [("random", 8195, 512, True), ("random", 8203, 2048, True)]


@functools.lru_cache(maxsize=None)
def _rms_want(case):
    return _rms_oracle(_rms_case(*case))


def _rms_scale(c):
    m = c["x"].abs().amax(1).double()
    return m if c["r"] is None else torch.maximum(m, c["r"].abs().amax(1).double())


def _rms_check(got, c, want, label):
    """got: y, s (or None), rstd, dx, dres (or None), dw from the kernels, on any device."""
    scale = _rms_scale(c)
    _check_scalar_rows("rms.rstd", got["rstd"], want["rstd"], label, relative=True)
    _check_rows("rms.y", got["y"], want["y"], label)
    if c["r"] is not None:
        _check_rows("rms.s", got["s"], want["s"], label, scale)
    if "dx" in got:
        dscale = c["dy"].abs().amax(1).double()
        _check_rows("rms.dx", got["dx"], want["dx"], label, dscale)
        if c["r"] is not None:
            assert torch.equal(got["dres"], got["dx"]), (label, "dres")
        # the backward kernel's own inputs: s as stored, dy, and the rstd the forward wrote (fp32 product)
        s = (c["x"].float() + c["r"].float()).bfloat16() if c["r"] is not None else c["x"]
        terms = c["dy"].double() * (s.float() * got["rstd"].cpu()[:, None]).bfloat16().double()
        assert got["dw"].dtype == torch.bfloat16 and torch.isfinite(got["dw"]).all(), (label, "dw")
        ex = _dw_excess(got["dw"], terms)
        assert bool((ex <= 0).all()), (label, "dw", float(ex.max()), int(ex.argmax()))


def _rounded(want, c):
    """An oracle's outputs stored as the kernels store them."""
    out = dict(y=want["y"].bfloat16(), s=want["s"].bfloat16(), rstd=want["rstd"].float(), dx=want["dx"].bfloat16(),
               dres=want["dx"].bfloat16())
    s = (c["x"].float() + c["r"].float()).bfloat16() if c["r"] is not None else c["x"]
    out["dw"] = (c["dy"].double() * (s.float() * out["rstd"][:, None]).bfloat16().double()).sum(0).bfloat16()
    return out


# ================================================================================ SwiGLU
def _swiglu_oracle(gu, d, emulate=False, swap=False, no_gterm=False):
    """gu [T, 2F] = gate | up, d [T, F] -> out, dgate, dup in fp64. emulate rounds where the kernels do:
      * out = bf16(bf16(silu(g)) * u)        elementwise.hip:32-33 and :109-110
      * dup = bf16(d * bf16(silu(g)))        elementwise.hip:55, 60 and :137, 142
      * dgate = bf16(d u s (1 + g (1 - s)))  elementwise.hip:56, 59 and :138, 141
    The slips: ``swap`` takes the halves the other way round, ``no_gterm`` leaves g (1 - s) out."""
    F = gu.shape[1] // 2
    g, u = gu[:, :F].double(), gu[:, F:].double()
    if swap:
        g, u = u, g
    d = d.double()
    sg = torch.sigmoid(g)
    si = g * sg
    if emulate:
        si = _bf(si)
    out, dup = si * u, d * si
    dgate = d * u * sg * (1.0 if no_gterm else 1.0 + g * (1.0 - sg))
    if emulate:
        out, dup, dgate = _bf(out), _bf(dup), _bf(dgate)
    return dict(out=out, dgate=dgate, dup=dup)


SWIGLU_SHAPES = [(1, 8), (3, 520), (257, 1024), (1031, 4104)]  # the last: 528 903 vectors > 2048 x 256
EXHAUSTIVE = (64, 1024)


@functools.lru_cache(maxsize=None)
def _swiglu_case(T, F, exhaustive=False):
    g = _gen(2, T, F, exhaustive)
    if exhaustive:
        assert T * F == 65536
        bits = torch.arange(65536, dtype=torch.int32)
        bits = torch.where((bits & 0x7F80) == 0x7F80, torch.zeros_like(bits), bits)  # NaN, inf -> 0
        gate = (bits - ((bits >> 15) << 16)).to(torch.int16).view(torch.bfloat16).view(T, F).float()
        col, row = torch.arange(F, dtype=torch.float32)[None, :], torch.arange(T, dtype=torch.float32)[:, None]
        up = 0.25 + 0.75 * torch.sin(0.37 * col + 0.5 * row)
        d = 0.3 - 0.7 * torch.cos(0.23 * col + 0.9 * row)
    else:
        gate = 4.0 * torch.randn(T, F, generator=g)
        up = torch.randn(T, F, generator=g)
        d = torch.randn(T, F, generator=g)
    return torch.cat([gate, up], dim=1).bfloat16(), d.bfloat16()


SWIGLU_CASES = [(T, F, False) for T, F in SWIGLU_SHAPES] + [EXHAUSTIVE + (True,)]


@functools.lru_cache(maxsize=None)
def _swiglu_want(case):
    return _swiglu_oracle(*_swiglu_case(*case))


def _swiglu_check(got, case, want, label):
    gu, d = _swiglu_case(*case)
    F = gu.shape[1] // 2
    scale = torch.maximum(gu[:, F:].abs().amax(1), d.abs().amax(1)).double()
    for name in ("out", "dgate", "dup"):
        if name in got:
            _check_rows(f"swiglu.{name}", got[name], want[name], label, scale)


# ================================================================================ RoPE
MAX_POS = 300


@functools.lru_cache(maxsize=None)
def _cs_table(D):
    """[MAX_POS, D/2, 2] fp32 (cos, sin), theta = 500000: the kernels' table operand."""
    inv = 500000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    f = torch.outer(torch.arange(MAX_POS, dtype=torch.float64), inv)
    return torch.stack([f.cos(), f.sin()], dim=-1).float()


def _rope_oracle(x, pos, Hq, Hk, D, backward=False, emulate=False, slip=None):
    """x [T, (Hq + 2 Hk) D], pos [T] -> the q and k heads rotated by +theta (by -theta: the gradient),
    v heads as they are; fp64. emulate rounds once, on the store (elementwise.hip:184-185, :333).
    slip: "sign", "pos+1", "adjacent" (pairs (2i, 2i+1)) or "v" (the first v head rotated too)."""
    T = x.shape[0]
    cs = _cs_table(D).double()
    p = pos + 1 if slip == "pos+1" else pos
    c, s = cs[p, :, 0][:, None, :], cs[p, :, 1][:, None, :]
    if backward != (slip == "sign"):
        s = -s
    nrot = Hq + Hk + (1 if slip == "v" else 0)
    h = x.double().view(T, Hq + 2 * Hk, D).clone()
    r = h[:, :nrot]
    if slip == "adjacent":
        a, b = r[..., 0::2], r[..., 1::2]
        h[:, :nrot] = torch.stack([a * c - b * s, b * c + a * s], dim=-1).flatten(-2)
    else:
        a, b = r[..., : D // 2], r[..., D // 2:]
        h[:, :nrot] = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    if emulate:
        h = _bf(h)
    return h.view(T, -1)


def _rope_pos(T, S, explicit):
    if not explicit:
        return torch.arange(T) % S
    p = torch.randint(0, MAX_POS, (T,), generator=_gen(3, T, S))
    p[0] = 0
    p[-1] = MAX_POS - 1
    if T == 1:
        p[0] = MAX_POS - 1
    return p


@functools.lru_cache(maxsize=None)
def _rope_case(T, Hq, Hk, D):
    g = _gen(4, T, Hq, Hk, D)
    W = (Hq + 2 * Hk) * D
    return torch.randn(T, W, generator=g).bfloat16(), torch.randn(T, W, generator=g).bfloat16()


ROPE_S = {1: 4, 5: 3, 130: 7, 128: 48, 2048: 130}  # seq_len for each T; none divides its T but T = 1
ROPE_CASES = [(T, Hq, Hk, D) for D in (16, 64, 128) for Hq, Hk in ((1, 1), (4, 2)) for T in (1, 5, 130)]
ROPE_BIG = (2048, 32, 8, 128)  # 655 360 work items > 2048 x 256
ROPE_TR = [(128, 1, 1, 128), ROPE_BIG]  # rca_rope_bwd_tr: D = 128, T % 128 == 0


def _rope_check(kind, got, want, x, Hq, Hk, D, label):
    T = x.shape[0]
    nrot = (Hq + Hk) * D
    rows = lambda t: t[:, :nrot].reshape(T, Hq + Hk, D)
    _check_rows(kind, rows(got), rows(want), label, rows(x).abs().amax(-1).double())
    assert torch.equal(got[:, nrot:].cpu(), x[:, nrot:]), (label, "v heads changed")


# ================================================================================ cross-entropy
def _ce_oracle(x, labels, g_row, ignore_index=-100, emulate=False, slip=None):
    """x [T, V] bf16, labels [T], g_row [T] (the upstream gradient of each row's loss) -> lse, loss
    [T] and dlogits [T, V] = g (softmax - onehot), fp64; an ignored row has loss 0 and a zero gradient.
    emulate rounds where the kernels do -- once, on the store: lse and loss as fp32 (loss_optim.hip:
    64-66 and :179-180; the label logit is subtracted from the fp32 lse), p = exp(x - lse) from that
    fp32 lse, p - 1 at the label and the product with g in fp32, and dlogits as bf16 (loss_optim.hip:
    90-94, :97-99 and :192-196).
    slip: "vector" (the lse leaves out columns 8..15), "tail" (the V % 8 tail), "label+1", "no-1",
    "zeros" (non-label entries zero), "ignored" (an ignored row treated as a live one)."""
    T, V = x.shape
    xd = x.double()
    lab = labels.clone()
    ign = (lab == ignore_index) | (lab < 0) | (lab >= V)
    live = ~ign
    if slip == "ignored":
        live = torch.ones_like(live)
    lab_c = torch.where(ign, torch.zeros_like(lab), lab)
    xs = xd
    if slip == "vector":
        xs = xd.clone()
        xs[:, 8:16] = -math.inf
    elif slip == "tail":
        xs = xd[:, : V - V % 8]
    lse = torch.logsumexp(xs, dim=1)
    col = (lab_c + 1) % V if slip == "label+1" else lab_c
    xl = xd.gather(1, col[:, None])[:, 0]
    if emulate:
        lse = lse.float()
        loss = (lse - xl.float()).double()
        lse = lse.double()
        p = torch.exp((x.float() - lse.float()[:, None]).double()).float()
    else:
        loss = lse - xl
        p = torch.exp(xd - lse[:, None])
    loss = torch.where(live, loss, torch.zeros_like(loss))
    hot = torch.zeros(T, V, dtype=p.dtype)
    if slip != "no-1":
        hot[torch.arange(T), col] = 1.0
    if slip == "zeros":
        p = p * hot
    gl = torch.where(live, g_row.double(), torch.zeros(T, dtype=torch.float64))
    if emulate:
        dl = (gl.float()[:, None] * (p - hot)).bfloat16().double()
    else:
        dl = gl[:, None] * (p - hot)
    dl[~live] = 0.0
    return dict(lse=lse, loss=loss, dlogits=dl)


CE_KINDS = ("random", "peak-on", "peak-off", "flat", "shift+", "shift-")
CE_MASK = {1024: 16, 4096: 16, 1003: 5}   # V -> columns masked at the end of a ``masked`` row
CE_MASK_HEAD = (4104, 8200)               # V whose ``masked-head`` rows mask the first 8 columns
CE_UNFUSED = [(8, 67), (1000, 67), (1003, 67), (1024, 23), (4096, 67), (4104, 31), (128256, 19)]
CE_FUSED = [(8, 5), (1024, 9), (8200, 9), (32000, 6), (40000, 7), (128256, 8), (131072, 9)]


def _ce_kinds(V):
    return CE_KINDS + (("masked",) if V in CE_MASK else ()) + (("masked-head",) if V in CE_MASK_HEAD else ())


@functools.lru_cache(maxsize=None)
def _ce_case(V, T, ignore_index=-100):
    """logits [T, V] bf16, labels [T] (first at 0, 7, 8, V - 1; some ignored), the row kinds."""
    g = _gen(5, V, T, ignore_index)
    kinds = _ce_kinds(V)
    off = V % len(kinds)
    kind = [kinds[(i + off) % len(kinds)] for i in range(T)]
    x = 3.0 * torch.randn(T, V, generator=g)
    lab = torch.randint(0, V, (T,), generator=g)
    fixed = [0, 7, 8, V - 1]
    for i in range(min(T, 4)):
        lab[i] = min(fixed[i], V - 1)
    for i, k in enumerate(kind):
        if k in ("peak-on", "peak-off"):
            top = int(torch.randint(0, V, (1,), generator=g))
            x[i] = x[i].clamp_max(3.0)
            x[i, top] = x[i].max() + 30.0
            if k == "peak-on" and i >= 4:
                lab[i] = top
            elif k == "peak-off" and lab[i] == top:
                lab[i] = (top + 1) % V
        elif k == "flat":
            x[i] = float(torch.randn(1, generator=g)) * 2.0
        elif k == "shift+":
            x[i] += 200.0
        elif k == "shift-":
            x[i] -= 200.0
        elif k == "masked":
            x[i, V - CE_MASK[V]:] = -math.inf
            lab[i] = lab[i] % (V - CE_MASK[V])
        elif k == "masked-head":
            x[i, :8] = -math.inf
            lab[i] = 8 + lab[i] % (V - 8)
    if ignore_index == -100:
        lab[4::6] = -100
    else:
        lab[4::6] = ignore_index  # a valid class id: rows labelled with it are ignored
    return x.bfloat16(), lab, kind


def _ce_grow(T, seed):
    """Per-row upstream gradients with zeros and negative values among them."""
    g = torch.randn(T, generator=_gen(6, T, seed)) * 0.5
    g[1::5] = 0.0
    g[2::5] = -g[2::5].abs() - 0.1
    return g


def _ce_runs():
    """(V, T, ignore_index, g_row) of every CE run of the file: the unfused reductions and the fused scale."""
    runs = []
    for V, T in CE_UNFUSED:
        for ii in (-100, 5):
            _, lab, _ = _ce_case(V, T, ii)
            n = max(1, int((lab != ii).sum()))
            runs += [(V, T, ii, _ce_grow(T, V)), (V, T, ii, torch.ones(T)), (V, T, ii, torch.full((T,), 1.0 / n))]
    for V, T in CE_FUSED:
        runs += [(V, T, -100, torch.full((T,), 1.0 / T)), (V, T, -100, torch.zeros(T))]
    return runs


def _ce_check(got, x, lab, g_row, want, label):
    _check_scalar_rows("ce.lse", got["lse"], want["lse"], label, relative=False)
    _check_scalar_rows("ce.loss", got["loss"], want["loss"], label, relative=False)
    if "dlogits" in got:
        _check_dlogits(got["dlogits"], want["dlogits"], g_row, lab, label)


# ======================================================================== CPU tests: the bounds
def _floors():
    f = dict.fromkeys(BOUND, 0.0)

    def up(kind, err):
        f[kind] = max(f[kind], float(err.max()))

    for case in RMS_CASES + RMS_BIG:
        c = _rms_case(*case)
        ex, em = _rms_want(case), _rms_oracle(c, emulate=True)
        up("rms.rstd", _rel_err(em["rstd"], ex["rstd"]))
        up("rms.y", _row_err(em["y"], ex["y"]))
        up("rms.s", _row_err(em["s"], ex["s"], _rms_scale(c)))
        up("rms.dx", _row_err(em["dx"], ex["dx"], c["dy"].abs().amax(1).double()))
    for case in SWIGLU_CASES:
        gu, d = _swiglu_case(*case)
        F = gu.shape[1] // 2
        scale = torch.maximum(gu[:, F:].abs().amax(1), d.abs().amax(1)).double()
        ex, em = _swiglu_want(case), _swiglu_oracle(gu, d, emulate=True)
        for name in ("out", "dgate", "dup"):
            up(f"swiglu.{name}", _row_err(em[name], ex[name], scale))
    for T, Hq, Hk, D in ROPE_CASES + ROPE_TR:
        x, gr = _rope_case(T, Hq, Hk, D)
        nrot = Hq + Hk
        for explicit in (False, True):
            pos = _rope_pos(T, ROPE_S[T], explicit)
            for kind, t, bw in (("rope.out", x, False), ("rope.grad", gr, True)):
                ex = _rope_oracle(t, pos, Hq, Hk, D, bw).view(T, -1, D)[:, :nrot]
                em = _rope_oracle(t, pos, Hq, Hk, D, bw, emulate=True).view(T, -1, D)[:, :nrot]
                up(kind, _row_err(em, ex, t.view(T, -1, D)[:, :nrot].abs().amax(-1).double()))
    for V, T, ii, g_row in _ce_runs():
        x, lab, _ = _ce_case(V, T, ii)
        ex, em = _ce_oracle(x, lab, g_row, ii), _ce_oracle(x, lab, g_row, ii, emulate=True)
        up("ce.lse", (em["lse"] - ex["lse"]).abs())
        up("ce.loss", (em["loss"] - ex["loss"]).abs())
        diff = (em["dlogits"] - ex["dlogits"]).abs()
        live = (lab != ii) & (lab >= 0) & (g_row != 0)
        hot = torch.zeros_like(diff, dtype=torch.bool)
        hot[torch.arange(T)[live], lab[live]] = True
        rel = diff / ex["dlogits"].abs()
        rel = torch.where(hot | (ex["dlogits"] == 0), torch.zeros_like(rel), rel)
        up("ce.dl_rel", rel)
        # at the label: what the relative part (at its floor: half a bf16 ulp, 2**-8) leaves over
        over = (diff - 2.0 ** -8 * ex["dlogits"].abs()).clamp_min(0) / g_row.double().abs().clamp_min(1e-300)[:, None]
        up("ce.dl_a", torch.where(hot, over, torch.zeros_like(over)))
        if live.any():
            # the fp32 label probability against the exact one: the cancelling term itself
            pl = torch.exp((x.float() - ex["lse"].float()[:, None]).double()).float().double()
            pe = torch.exp(x.double() - ex["lse"][:, None])
            up("ce.dl_a", (pl - pe).abs()[hot])
    return f


def test_bounds_are_twice_the_measured_floors():
    """The reference for BOUND. dw has no floor: its bound is the column-sum formula of ``_dw_excess``."""
    f = _floors()
    for kind in BOUND:
        print(f"    {kind:<13} {f[kind]:.2e}   2**{math.log2(BOUND[kind]):.0f} = {BOUND[kind]:.2e}")
    for kind in BOUND:
        assert 0 < f[kind] <= BOUND[kind] / 2, (kind, f[kind])
        assert BOUND[kind] == 2.0 ** math.ceil(math.log2(2 * f[kind])), (kind, f[kind])


def test_ce_data_cannot_hide_a_zeroed_entry():
    """Every entry of a live row with g != 0 that is not masked has a non-zero exact gradient (its
    bound is relative, so zero there fails), the median |want| of such a row is far above the label
    column's absolute allowance A |g| except in rows whose label sits ON the peak (where every other
    entry is 1e-13 and still has its relative bound), and labels avoid the masked columns."""
    for V, T, ii, g_row in _ce_runs():
        x, lab, kind = _ce_case(V, T, ii)
        want = _ce_oracle(x, lab, g_row, ii)
        live = (lab != ii) & (g_row != 0)
        assert live.any() or not g_row.any()
        assert bool(((want["dlogits"] != 0) | torch.isinf(x.float()))[live].all()), (V, T, ii)
        assert bool((want["dlogits"][~live] == 0).all())
        assert torch.isfinite(x.float().gather(1, lab.clamp_min(0)[:, None])[:, 0][lab != ii]).all()
        assert torch.isfinite(want["lse"]).all() and torch.isfinite(want["loss"]).all()
        for i in torch.nonzero(live)[:, 0].tolist():
            assert want["dlogits"][i].abs().median().item() > 0, (V, i, kind[i])


def test_ce_fused_supported_shapes():
    assert not ops.ce_fused_supported(1003) and not ops.ce_fused_supported(131080)
    assert all(ops.ce_fused_supported(V) for V, _ in CE_FUSED)


# ================================================================ CPU tests: the checkers reject slips
def _rows_rejected(kind, got, want, scale=None):
    return ~(_row_err(got, want, scale) < BOUND[kind])


@pytest.mark.parametrize("H", [H for H in RMS_H if H % 512 == 0])
@pytest.mark.parametrize("res", [False, True])
def test_rmsnorm_checker_rejects_a_dropped_vector(H, res):
    """The sum of squares without one 8-column vector: every row of a spiked case leaves out ITS heavy
    vector. In the 67-row case that is lane i % 64 of slot i % VPL (every lane and every slot of
    rmsnorm_fwd_reg / rmsnorm_bwd_reg<VPL> in turn), in the H / 8-row case vector i (every pair of
    them). Each row is rejected through rstd, y and dx."""
    for rows in (67, H // 8):
        case = ("spiked", rows, H, res)
        c, want = _rms_case(*case), _rms_want(case)
        hv = _heavy_vector(rows, H)
        assert set((hv % 64).tolist()) == set(range(64)) and set((hv // 64).tolist()) == set(range(H // 512))
        assert rows == 67 or set(hv.tolist()) == set(range(H // 8))
        bad = _rounded(_rms_oracle(c, drop=hv), c)
        assert bool(~(_rel_err(bad["rstd"], want["rstd"]) < BOUND["rms.rstd"]).all())
        assert bool(_rows_rejected("rms.y", bad["y"], want["y"]).all())
        assert bool(_rows_rejected("rms.dx", bad["dx"], want["dx"], c["dy"].abs().amax(1).double()).all())
        with pytest.raises(AssertionError):
            _rms_check(bad, c, want, "dropped vector")
        _rms_check(_rounded(want, c), c, want, "intact")


@pytest.mark.parametrize("H", RMS_H)
def test_rmsnorm_checker_rejects_eps_norm_of_x_and_a_missing_dw_row(H):
    # eps = 1e-6: the 2**-10 rows of the mixed case (rows 0, 3, ..) move by a factor of 2
    case = ("mixed", 67, H, True)
    c, want = _rms_case(*case), _rms_want(case)
    bad = _rounded(_rms_oracle(c, eps=1e-6), c)
    small = torch.arange(67) % 3 == 0
    assert bool(~(_rel_err(bad["rstd"], want["rstd"]) < BOUND["rms.rstd"])[small].all())
    assert bool(_rows_rejected("rms.y", bad["y"], want["y"])[small].all())
    # the norm of x in place of x + r: every row
    for kind in ("random", "spiked", "mixed"):
        case = (kind, 67, H, True)
        c, want = _rms_case(*case), _rms_want(case)
        bad = _rounded(_rms_oracle(c, norm_of_x=True), c)
        assert bool(~(_rel_err(bad["rstd"], want["rstd"]) < BOUND["rms.rstd"]).all()), kind
    # dw without the last row: every column whose last term is not negligible
    for rows in RMS_ROWS:
        case = ("random", rows, H, False)
        c, want = _rms_case(*case), _rms_want(case)
        good = _rounded(want, c)
        terms = c["dy"].double() * (c["x"].float() * good["rstd"][:, None]).bfloat16().double()
        assert bool((_dw_excess(good["dw"], terms) <= 0).all())
        short = terms[:-1].sum(0).bfloat16()
        ex = _dw_excess(short, terms)
        matters = terms[-1].abs() > 2.0 ** -6 * terms.abs().sum(0)
        assert matters.any() and bool((ex > 0)[matters].all()), (H, rows)


@pytest.mark.parametrize("case", SWIGLU_CASES, ids=str)
def test_swiglu_checker_rejects_swapped_halves_and_a_missing_term(case):
    gu, d = _swiglu_case(*case)
    F = gu.shape[1] // 2
    scale = torch.maximum(gu[:, F:].abs().amax(1), d.abs().amax(1)).double()
    want = _swiglu_want(case)
    ok = {k: v.bfloat16() for k, v in _swiglu_oracle(gu, d, emulate=True).items()}
    _swiglu_check(ok, case, want, "intact")
    bad = {k: v.bfloat16() for k, v in _swiglu_oracle(gu, d, swap=True).items()}
    for name in ("out", "dgate", "dup"):
        assert bool(_rows_rejected(f"swiglu.{name}", bad[name], want[name], scale).all()), name
    bad = _swiglu_oracle(gu, d, no_gterm=True)["dgate"].bfloat16()
    rej = _rows_rejected("swiglu.dgate", bad, want["dgate"], scale)
    # the term g (1 - s) vanishes with g, and the whole of dgate with -g and 1 - s with g: the slip is
    # felt by the rows that hold a gate of ordinary size (all but some of the exhaustive case)
    g = gu[:, :F].float().abs()
    felt = ((g >= 0.25) & (g <= 8.0)).any(1)
    assert felt.any() and bool(rej[felt].all())


@pytest.mark.parametrize("T,Hq,Hk,D", ROPE_CASES + ROPE_TR[:1])
@pytest.mark.parametrize("explicit", [False, True])
def test_rope_checker_rejects_sign_position_pairing_and_a_rotated_v(T, Hq, Hk, D, explicit):
    x, gr = _rope_case(T, Hq, Hk, D)
    pos = _rope_pos(T, ROPE_S[T], explicit).clamp_max(MAX_POS - 2)
    nrot = Hq + Hk
    heads = lambda t: t.view(T, -1, D)
    for kind, t, bw in (("rope.out", x, False), ("rope.grad", gr, True)):
        want = _rope_oracle(t, pos, Hq, Hk, D, bw)
        scale = heads(t)[:, :nrot].abs().amax(-1).double()
        _rope_check(kind, _rope_oracle(t, pos, Hq, Hk, D, bw, emulate=True).bfloat16(), want, t, Hq, Hk, D, "intact")
        moved = pos != 0  # position 0 is the identity rotation
        for slip in ("sign", "adjacent"):
            bad = _rope_oracle(t, pos, Hq, Hk, D, bw, slip=slip).bfloat16()
            rej = _rows_rejected(kind, heads(bad)[:, :nrot], heads(want)[:, :nrot], scale)
            assert bool(rej[moved].all()), (kind, slip)
        # one position late: seen on the two highest-frequency pairs alone (columns 0, 1, D/2, D/2 + 1)
        bad = _rope_oracle(t, pos, Hq, Hk, D, bw, slip="pos+1").bfloat16()
        hf = [0, 1, D // 2, D // 2 + 1]
        rej = _rows_rejected(kind, heads(bad)[:, :nrot][..., hf], heads(want)[:, :nrot][..., hf],
                             heads(t)[:, :nrot][..., hf].abs().amax(-1).double())
        assert bool(rej.all()), (kind, "pos+1")
        bad = _rope_oracle(t, pos, Hq, Hk, D, bw, slip="v").bfloat16()
        if moved.any():
            with pytest.raises(AssertionError):
                _rope_check(kind, bad, want, t, Hq, Hk, D, "v rotated")
            assert not torch.equal(bad[moved][:, nrot * D: (nrot + 1) * D], t[moved][:, nrot * D: (nrot + 1) * D])


@pytest.mark.parametrize("V,T", CE_UNFUSED + CE_FUSED, ids=str)
def test_ce_checker_rejects_every_slip(V, T):
    ii = -100
    x, lab, kind = _ce_case(V, T, ii)
    g_row = _ce_grow(T, V) if (V, T) in CE_UNFUSED else torch.full((T,), 1.0 / T)
    want = _ce_oracle(x, lab, g_row, ii)
    em = _ce_oracle(x, lab, g_row, ii, emulate=True)
    _ce_check(dict(lse=em["lse"].float(), loss=em["loss"].float(), dlogits=em["dlogits"].bfloat16()), x, lab, g_row, want,
              "intact")
    live = (lab != ii)
    moving = live & (g_row != 0)

    def stored(w):
        return dict(lse=w["lse"].float(), loss=w["loss"].float(), dlogits=w["dlogits"].bfloat16())

    def lse_rejected(bad):
        return ~((bad["lse"].float().double() - want["lse"]).abs() < BOUND["ce.lse"])

    # lse without columns 8..15 (one 16-byte vector); without the V % 8 tail
    slips = (["vector"] if V >= 16 else []) + (["tail"] if V % 8 else [])
    for slip in slips:
        bad = _ce_oracle(x, lab, g_row, ii, slip=slip)
        gone = torch.logsumexp(x.double()[:, 8:16] if slip == "vector" else x.double()[:, V - V % 8:], 1)
        felt = (gone - want["lse"]) > math.log(4 * BOUND["ce.lse"])  # the dropped columns' share of exp(lse)
        assert (felt.sum() >= T // 3 or V > 4104) and bool(lse_rejected(bad)[felt].all()), slip
        if felt.any():
            with pytest.raises(AssertionError):
                _ce_check(stored(bad), x, lab, g_row, want, slip)
    for slip in ("label+1", "no-1", "zeros"):
        bad = stored(_ce_oracle(x, lab, g_row, ii, slip=slip))
        ex = _dl_excess(bad["dlogits"], want["dlogits"], g_row, lab)
        assert moving.any() and bool((ex > 0).any(1)[moving].all()), slip
        if slip == "zeros":  # every non-label, non-masked entry of every live row
            hot = torch.zeros_like(ex, dtype=torch.bool)
            hot[torch.arange(T)[live], lab[live]] = True
            rest = moving[:, None] & ~hot & ~torch.isinf(x.float())
            assert bool((ex > 0)[rest].all())
        if slip == "label+1":
            nxt = x.double().gather(1, ((lab.clamp_min(0) + 1) % V)[:, None])[:, 0]
            felt = live & ((nxt - x.double().gather(1, lab.clamp_min(0)[:, None])[:, 0]).abs() >= 2 * BOUND["ce.loss"])
            assert felt.sum() >= live.sum() // 2
            assert bool(~((bad["loss"].double() - want["loss"]).abs() < BOUND["ce.loss"])[felt].all())
    bad = stored(_ce_oracle(x, lab, g_row, ii, slip="ignored"))
    dead = ~live & (g_row != 0)
    if (~live).any():
        assert bool(~((bad["loss"].double() - want["loss"]).abs() < BOUND["ce.loss"])[~live].all())
    if dead.any():
        assert bool((_dl_excess(bad["dlogits"], want["dlogits"], g_row, lab) > 0).any(1)[dead].all())


# ========================================================================================= GPU tests
def _lib_call(name, *args):
    from ray_community_amd.ops._lib import check, stream_ptr

    check(getattr(ops.lib(), name)(*args, stream_ptr(torch.device("cuda"))), name)


def _rms_run(c):
    rows, H = c["x"].shape
    dev = {k: (None if v is None else v.cuda()) for k, v in c.items()}
    p = lambda t: 0 if t is None else t.data_ptr()
    y, rstd = torch.empty_like(dev["x"]), torch.empty(rows, device="cuda")
    s = torch.empty_like(dev["x"]) if dev["r"] is not None else None
    _lib_call("rca_rmsnorm_fwd", dev["x"].data_ptr(), p(dev["r"]), dev["w"].data_ptr(), y.data_ptr(), p(s),
              rstd.data_ptr(), rows, H, EPS)
    x, w = dev["x"].clone().requires_grad_(True), dev["w"].clone().requires_grad_(True)
    if dev["r"] is None:
        y2 = ops.rms_norm(x, w, EPS)
        y2.backward(dev["dy"])
        got = dict(dx=x.grad)
    else:
        r = dev["r"].clone().requires_grad_(True)
        y2, s2 = ops.rms_norm(x, w, EPS, residual=r)
        torch.autograd.backward([y2, s2], [dev["dy"], dev["ds"]])
        assert torch.equal(s2, s)
        got = dict(dx=x.grad, dres=r.grad, s=s.cpu())
    torch.cuda.synchronize()
    assert torch.equal(y2, y)  # the op is the kernel called above
    got.update(y=y.cpu(), rstd=rstd.cpu(), dw=w.grad.cpu())
    return {k: v.cpu() for k, v in got.items()}


@gpu
@pytest.mark.parametrize("H", RMS_H)
def test_rmsnorm_rows(H):
    for case in [c for c in RMS_CASES if c[2] == H]:
        c = _rms_case(*case)
        _rms_check(_rms_run(c), c, _rms_want(case), f"rmsnorm {case}")


@gpu
@pytest.mark.parametrize("case", RMS_BIG, ids=str)
def test_rmsnorm_rows_over_the_backward_grid_cap(case):
    rows, H = case[1], case[2]
    assert ops.lib().rca_rmsnorm_bwd_blocks(rows, H) == (1024 if H in (2048, 4096) else 512)
    assert rows > (1024 * 8 if H in (2048, 4096) else 512 * 16)
    c = _rms_case(*case)
    _rms_check(_rms_run(c), c, _rms_want(case), f"rmsnorm {case}")


def _swiglu_run(case, tr):
    gu, d = (t.cuda() for t in _swiglu_case(*case))
    F = gu.shape[1] // 2
    x = gu.clone().requires_grad_(True)
    if tr:
        assert ops._swiglu_tr_ok(gu)
        out, out_t = ops.swiglu(x, with_transposed=True)
        dgu = ops.swiglu_backward(gu, d, True)
        dgu_t = ops.pop_grad_transposed(dgu)
        torch.cuda.synchronize()
        assert torch.equal(out_t, out.t()) and torch.equal(dgu_t, dgu.t())  # bit-equal transposes
    else:
        out = ops.swiglu(x)
        out.backward(d)
        dgu = x.grad
        assert torch.equal(dgu, ops.swiglu_backward(gu, d))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), dgate=dgu[:, :F].cpu(), dup=dgu[:, F:].cpu())


@gpu
@pytest.mark.parametrize("case", SWIGLU_CASES, ids=str)
def test_swiglu_rows(case):
    """The last plain shape takes a second trip through the grid-stride loop; the exhaustive case (every
    bf16 gate) also runs the transposing kernels, whose row-major outputs are scored like the others."""
    T, F, exhaustive = case
    if not exhaustive:
        assert (T * (F // 8) > 2048 * 256) == ((T, F) == SWIGLU_SHAPES[-1])
    _swiglu_check(_swiglu_run(case, False), case, _swiglu_want(case), f"swiglu {case}")
    if exhaustive:
        _swiglu_check(_swiglu_run(case, True), case, _swiglu_want(case), f"swiglu {case} tr")


def _rope_run(T, Hq, Hk, D, variant):
    """variant: "plain" (contiguous, t % S), "pos" (explicit positions), both through apply_rope_ and
    autograd; "slice" (qkv and the gradient as column slices of wider NaN-free buffers, stride(0) >
    width): apply_rope_ without autograd and rca_rope(backward = 1) on the gradient slice."""
    x, gr = _rope_case(T, Hq, Hk, D)
    S = ROPE_S[T]
    W = x.shape[1]
    cs = _cs_table(D).cuda()
    explicit = variant == "pos"
    pos = _rope_pos(T, S, explicit)
    pos_dev = pos.cuda() if explicit else None
    if variant == "slice":
        pad = torch.randn(T, W + 32, generator=_gen(7, T, W)).bfloat16()
        bx, bg = pad.clone().cuda(), pad.clone().cuda()
        bx[:, 8: 8 + W] = x.cuda()
        bg[:, 8: 8 + W] = gr.cuda()
        vx, vg = bx[:, 8: 8 + W], bg[:, 8: 8 + W]
        assert vx.stride(0) > W and vx.data_ptr() % 16 == 0
        with torch.no_grad():
            out = ops.apply_rope_(vx, cs, S, Hq, Hk, D)
        _lib_call("rca_rope", vg.data_ptr(), cs.data_ptr(), 0, T, S, Hq + Hk, vg.stride(0), D, 1)
        torch.cuda.synchronize()
        for b in (bx, bg):  # the columns outside the slice are bit-unchanged
            assert torch.equal(b[:, :8].cpu(), pad[:, :8]) and torch.equal(b[:, 8 + W:].cpu(), pad[:, 8 + W:])
        return out.cpu(), vg.cpu(), pos
    leaf = x.cuda().requires_grad_(True)
    out = ops.apply_rope_(leaf * 1.0, cs, S, Hq, Hk, D, positions=pos_dev)
    out.backward(gr.cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), leaf.grad.cpu(), pos


@gpu
@pytest.mark.parametrize("T,Hq,Hk,D", ROPE_CASES)
def test_rope_rows(T, Hq, Hk, D):
    x, gr = _rope_case(T, Hq, Hk, D)
    for variant in ("plain", "pos", "slice"):
        out, grad, pos = _rope_run(T, Hq, Hk, D, variant)
        label = f"rope {T}x{Hq}x{Hk}x{D} {variant}"
        _rope_check("rope.out", out, _rope_oracle(x, pos, Hq, Hk, D), x, Hq, Hk, D, label)
        _rope_check("rope.grad", grad, _rope_oracle(gr, pos, Hq, Hk, D, True), gr, Hq, Hk, D, label)


@gpu
@pytest.mark.parametrize("T,Hq,Hk,D", ROPE_TR)
@pytest.mark.parametrize("explicit", [False, True])
def test_rope_rows_backward_with_transpose_and_over_the_grid_cap(T, Hq, Hk, D, explicit):
    """rca_rope_bwd_tr and the plain kernel in both directions; the large shape has more work items
    than the capped grid has threads."""
    x, gr = _rope_case(T, Hq, Hk, D)
    S, W, nrot = ROPE_S[T], x.shape[1], Hq + Hk
    assert (T * nrot * (D // 16) > 2048 * 256) == ((T, Hq, Hk, D) == ROPE_BIG)
    cs = _cs_table(D).cuda()
    pos = _rope_pos(T, S, explicit)
    pos32 = pos.to(torch.int32).cuda()
    pp = pos32.data_ptr() if explicit else 0
    fwd, bwd, g1, g1t = x.cuda(), gr.cuda(), gr.cuda(), torch.empty(W, T, dtype=torch.bfloat16, device="cuda")
    _lib_call("rca_rope", fwd.data_ptr(), cs.data_ptr(), pp, T, S, nrot, W, D, 0)
    _lib_call("rca_rope", bwd.data_ptr(), cs.data_ptr(), pp, T, S, nrot, W, D, 1)
    _lib_call("rca_rope_bwd_tr", g1.data_ptr(), cs.data_ptr(), pp, g1t.data_ptr(), T, S, W, nrot)
    torch.cuda.synchronize()
    label = f"rope {T}x{Hq}x{Hk}x{D} explicit={explicit}"
    _rope_check("rope.out", fwd, _rope_oracle(x, pos, Hq, Hk, D), x, Hq, Hk, D, label)
    want = _rope_oracle(gr, pos, Hq, Hk, D, True)
    _rope_check("rope.grad", bwd, want, gr, Hq, Hk, D, label)
    _rope_check("rope.grad", g1, want, gr, Hq, Hk, D, label + " tr")
    assert torch.equal(g1t, g1.t())


@gpu
@pytest.mark.parametrize("V,T", CE_UNFUSED, ids=str)
@pytest.mark.parametrize("ii", [-100, 5])
def test_cross_entropy_rows(V, T, ii):
    x, lab, _ = _ce_case(V, T, ii)
    n = max(1, int((lab != ii).sum()))
    label = f"ce V={V} T={T} ignore={ii}"
    # reduction="none" with per-row upstream gradients; lse is the tensor the op saved for its backward
    g_row = _ce_grow(T, V)
    want = _ce_oracle(x, lab, g_row, ii)
    leaf = x.cuda().requires_grad_(True)
    loss = ops.cross_entropy(leaf, lab.cuda(), ignore_index=ii, reduction="none")
    lse = loss.grad_fn.saved_tensors[2]
    loss.backward(g_row.cuda())
    torch.cuda.synchronize()
    _ce_check(dict(lse=lse.cpu(), loss=loss.detach().cpu(), dlogits=leaf.grad.cpu()), x, lab, g_row, want, label + " none")
    # in place: bit-equal
    leaf2 = x.cuda().requires_grad_(True)
    loss2 = ops.cross_entropy(leaf2 * 1.0, lab.cuda(), ignore_index=ii, reduction="none", inplace_backward=True)
    loss2.backward(g_row.cuda())
    torch.cuda.synchronize()
    assert torch.equal(loss2, loss) and torch.equal(leaf2.grad, leaf.grad), label + " inplace"
    # sum and mean: the scalar against the oracle's rows, the gradient with g = 1 and 1 / n
    for reduction, g in (("sum", 1.0), ("mean", 1.0 / n)):
        g_row = torch.full((T,), g)
        want = _ce_oracle(x, lab, g_row, ii)
        leaf = x.cuda().requires_grad_(True)
        out = ops.cross_entropy(leaf, lab.cuda(), ignore_index=ii, reduction=reduction)
        out.backward()
        torch.cuda.synchronize()
        live = int((want["loss"] != 0).sum())
        total = want["loss"].sum().item() * g
        # every row within BOUND["ce.loss"], summed in fp32
        assert abs(out.item() - total) <= g * live * BOUND["ce.loss"] + 2.0 ** -22 * abs(total), (label, reduction)
        _check_dlogits(leaf.grad.cpu(), want["dlogits"], g_row, lab, f"{label} {reduction}")


@gpu
@pytest.mark.parametrize("V,T", CE_FUSED, ids=str)
def test_cross_entropy_fused_rows(V, T):
    """ce_fused_kernel<NPT> for every NPT, lse read through rca_ce_fused; gscale 1 / T and 0; against the
    oracle and against the unfused kernel."""
    assert ops.ce_fused_supported(V)
    npt = (V // 8 + 1023) // 1024  # vectors per thread; the kernel is instantiated for the next power of two
    assert {8: 1, 1024: 1, 8200: 2, 32000: 4, 40000: 8, 128256: 16, 131072: 16}[V] == 1 << (npt - 1).bit_length()
    x, lab, _ = _ce_case(V, T)
    label = f"ce fused V={V} T={T}"
    dev_lab = lab.cuda()
    ref_loss = ops.cross_entropy(x.cuda().requires_grad_(True), dev_lab, reduction="none")
    ref_lse = ref_loss.grad_fn.saved_tensors[2]
    for gs in (1.0 / T, 0.0):
        g_row = torch.full((T,), gs)
        want = _ce_oracle(x, lab, g_row)
        logits = x.cuda()
        gscale = torch.tensor([gs], device="cuda")
        loss, lse = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
        _lib_call("rca_ce_fused", logits.data_ptr(), dev_lab.data_ptr(), gscale.data_ptr(), loss.data_ptr(),
                  lse.data_ptr(), T, V, -100)
        torch.cuda.synchronize()
        _ce_check(dict(lse=lse.cpu(), loss=loss.cpu(), dlogits=logits.cpu()), x, lab, g_row, want, f"{label} g={gs:.3g}")
        ign = lab == -100
        assert ign.any() and bool((logits.cpu()[ign] == 0).all()) and bool((loss.cpu()[ign] == 0).all())
        if gs == 0.0:
            assert bool((logits == 0).all())
        for a, b in ((lse, ref_lse), (loss, ref_loss.detach())):  # both sit within the bound of the oracle
            assert bool(((a - b).abs() <= 2 * BOUND["ce.lse"]).all()), label
    out = ops.ce_fused_(x.cuda(), dev_lab, torch.tensor([1.0 / T], device="cuda"))
    assert torch.equal(out, loss)


@gpu
def test_linear_cross_entropy_v1003_matches_the_oracle():
    """V = 1003 is not a fused shape: whatever path linear_cross_entropy takes, the mean loss matches the
    fp64 oracle of the bf16 operands. Its logits are at best rounded to bf16 (relative 2**-9), and a
    row's loss moves by at most twice the largest change of one of its logits: the bound is the mean over
    the rows of 2**-8 rowmax |logit|, plus the loss bound of this file."""
    from ray_community_amd.parallel.fused_linear import linear_cross_entropy

    T, H, V = 64, 64, 1003
    g = _gen(8, T, H, V)
    h = torch.randn(T, H, generator=g).bfloat16()
    w = (0.125 * torch.randn(V, H, generator=g)).bfloat16()
    lab = torch.randint(0, V, (T,), generator=g)
    lab[::7] = -100
    logits = h.double() @ w.double().T
    live = lab != -100
    rows = torch.logsumexp(logits, 1) - logits.gather(1, lab.clamp_min(0)[:, None])[:, 0]
    want = rows[live].mean().item()
    bound = (2.0 ** -8 * logits.abs().amax(1)[live]).mean().item() + BOUND["ce.loss"]
    got = linear_cross_entropy(h.cuda(), w.cuda(), lab.cuda()).item()
    print(f"linear_cross_entropy V=1003: |got - want| = {abs(got - want):.3e}, bound {bound:.3e}")
    assert abs(got - want) < bound
