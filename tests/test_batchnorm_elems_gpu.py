"""The fused NHWC BatchNorm (+ residual) (+ ReLU) kernels of ops/csrc/batchnorm.hip -- forward, backward and
the frozen apply pass -- checked per channel and per element against float64 oracles written here,
independent of ops/reference.py and of autograd. The kernels are called through ``lib()`` (rca_bn_fwd,
rca_bn_bwd, rca_bn_apply, rca_bn_workspace), so stats[4][C], coef[3][C], dgamma and dbeta are read directly
and null pointers are passed; ``ops.batch_norm_act`` (with autograd) and ``ops.affine_act_`` run once per
data kind and must return the same bits.

Metric. Every oracle starts from the bf16 inputs the kernel sees. u = 2**-24, k_c = x[0, c] (the kernel's
shift), E2 = E[(x - k_c)**2] in fp64, D = the accumulation depth of the reduction (``_depth``: the terms one
thread adds in turn + the rows it folds through LDS + its share of the block partials + the 6 + 3 levels of
the final tree). Two kinds of bound:
  * measured floors (``BOUND``): each oracle has an ``emulate`` mode that rounds where the kernel rounds
    (``_emu_sums`` and ``_fake_kernel`` cite the lines); the floor is the worst emulate-vs-exact error over
    every case of this file, on the CPU, and the bound twice the floor rounded up to a power of two
    (``test_bounds_are_twice_the_measured_floors``);
  * derived bounds, which the emulate mode only has to stay inside (same test):
      var     |1 / invstd**2 - eps - var| <= (3 D + 7) u E2 + 2**-20 (var + eps). S2 carries D + 2 roundings
              on positive terms, m1**2 = (S1 / R)**2 <= E2 carries 2 D + 3, the division and the subtraction
              2 more; the second term is rsqrtf (1 ulp, the documented accuracy of v_rsq_f32) undone.
      running momentum 1 from zero: running_mean == stats mean bit for bit, running_var against the
              unbiased variance with the var bound times R / (R - 1) plus 2**-21 of itself; momentum 0.1 from
              random starts: m times the bounds of mean and var plus 2**-21 of the two products.
      sums    dbeta = Sg, dgamma = Sgx * invstd: |got - S| <= 2**-21 |S| + (D + 2) u sum|terms|, the terms
              g = dy [out > 0] and g (x - mean) formed from the kernel's OWN out and stats (its inputs, which
              are scored on their own); coef A relative 2**-22, B and D with the bounds of Sgx and Sg
              carried through their formulas plus 2**-21 of each product.
mean is scored as |got - want| / (|k_c| + sqrt(E2)); scale and shift relative to |gamma * invstd| and to |beta| +
|mean * scale| of the kernel's own mean and invstd. out, dx: per element, |got - want| <= REL |want| + A (|x scale|
+ |shift| + |res|) (dx: |A g| + |B x| + |D|), want from the kernel's own scale / shift (coef). REL < 1: an
element written as zero fails, and nothing is excused but a flushed bf16 denormal (|want| < 2**-126 stored as
0). dres must equal the masked dy bit for bit.

    quantity   floor      bound
    mean       1.86e-07   2**-21 = 4.77e-07
    scale      5.92e-08   2**-23 = 1.19e-07   (relative)
    shift      1.12e-07   2**-22 = 2.38e-07
    out.rel    3.89e-03   2**-7  = 7.81e-03   (the bf16 store of the fp32 result)
    out.a      8.91e-08   2**-22 = 2.38e-07   (the fp32 result against the exact one, over the magnitudes)
    dx.rel     3.89e-03   2**-7  = 7.81e-03
    dx.a       1.07e-07   2**-22 = 2.38e-07
Of the derived bounds the emulate mode uses at most: var 0.29, running_mean 0.63, running_var 0.28, dbeta 0.01,
dgamma 0.12, coef A 0.25, B 0.13, D 0.09. The floors of BIG and HUGE are taken on 128 of their 2048 channels.

Shapes (R = N H W rows, C channels; nblk from the host plan, asserted against rca_bn_workspace / (2 C)):
single block: the shapes of test_ops_gpu.py, R = 1, every supported power-of-two C at R = 19; 2 to 4 blocks:
C = 2048 at R = 33, 65, 100 (the rpi == 1 store path), C = 64 at R = 1025, 1100, C = 8 at R = 8200; C = 2048,
R = 8200: 257 blocks (a second trip of reduce_partials' loop) and 2 099 200 vectors > 4096 x 256 (a second
trip of both apply loops), forward and backward; C = 2048, R = 32800: the 1024-block target cap (33 rows a
block, 994 blocks), forward statistics, generated and scored on the device in channel chunks.

Data. ``random`` (mean 1, std 2); ``offset`` (mean 40, std 0.5); ``outlier-row0`` (std 1 around 0, row 0 at
+-90.5: 64 sigma of the channel at R = 8200); ``mixed`` (channel scales 2**-8, 1, 2**6 in turn); ``relu-edge`` (half the residuals cancel the
pre-activation to within one bf16 ulp). gamma steps by 0.25 from one 8-channel group to the next.

What the shift k_c = x[0, c] buys. It removes the channel's mean from E[x**2] - E[x]**2 only as far as row 0 is
typical: the error of var grows with E2 = var + (x[0, c] - mean)**2. ``offset`` loses nothing (E2 < 6 var); in
``outlier-row0`` at R = 8200 E2 = 4097 var, the derived bound is 3.6e-2 var (C = 2048) and 0.21 var (C = 8),
and the kernel's error is far inside it (below) and never clamps to 0. The header of batchnorm.hip now
says so; no kernel changed.

Fixed here: ``ops.batch_norm_act`` guarded only weight.dtype, so a bf16 bias or a non-fp32 running statistic
reached a kernel that reads float*; it now takes the torch composition for those and for non-contiguous
weight / bias (``test_batch_norm_act_falls_back_for_parameters_the_kernel_cannot_read``).

The tests without a ``gpu`` mark run anywhere: the floors, the plans, the data conditions and the slipped
oracles the checkers must reject (``test_checker_rejects_*``).

Measured on one MI355X (the whole file, CPU tests included: 5.7 s, 65 tests; the slowest GPU test 0.75 s),
largest share of its bound per GPU test:
    test_bn_elems (26 shapes)             mean 0.35  var 0.11  scale 0.50  shift 0.25  running_mean 0.34
                                          running_var 0.28  out 0.50  dx 0.50  dgamma 0.12  dbeta 0.01
                                          coef A 0.25  B 0.12  D 0.08, dres bit-equal
    test_bn_elems_over_256_blocks_...     mean 0.20  var 0.06  scale 0.49  shift 0.25  running_var 0.05  out 0.50
                                          dx 0.50  dgamma 0.06  coef A 0.25  B 0.06  D 0.01
    test_bn_forward_statistics_over_...   mean 0.13  var 0.05  shift 0.25  running_var 0.05  out 0.50
    test_bn_apply_unrolled_by_four_...    U = 4 bit-equal to U = 1, out 0.50
    test_bn_wrappers_return_...           bit-equal to the lib() calls (R = 1100, C = 64, every data kind)
    test_batch_norm_act_falls_back_...    0.97 of the composition's bound (bf16 bias and strided weight alike)
out and dx sit at 0.50: the bf16 store, half of REL. ``outlier-row0`` at R = 8200: var uses 0.05 of its bound at
C = 2048 (an error of 1.8e-3 var, where ``random`` has 2e-6 var) and 0.01 at C = 8; var never clamps to 0. No
kernel failed a check; the wrapper fix above was made from reading the code, before any run.
"""
import functools
import math

import pytest
import torch

from ray_community_amd import ops

gpu = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126  # the smallest normal bf16
EPS = torch.tensor(1e-5, dtype=torch.float32).item()  # what the kernel receives
MOM = torch.tensor(0.1, dtype=torch.float32).item()
BOUND = {"mean": 2.0 ** -21, "scale": 2.0 ** -23, "shift": 2.0 ** -22, "out.rel": 2.0 ** -7, "out.a": 2.0 ** -22,
         "dx.rel": 2.0 ** -7, "dx.a": 2.0 ** -22}
KINDS = ("random", "offset", "outlier-row0", "mixed", "relu-edge")
FLAGS = [(True, True), (True, False), (False, True), (False, False)]  # relu, residual

SMALL = [(480, 64), (98, 256), (27, 2048), (50, 8), (33, 128)]  # test_ops_gpu.py's
ROW1 = [(1, 64), (1, 2048)]
CHANNELS = [(19, C) for C in (8, 16, 32, 64, 128, 256, 512, 1024, 2048)]
RAGGED = [(33, 2048), (65, 2048), (100, 2048), (1025, 64), (1100, 64), (8200, 8)]
BIG = (8200, 2048)
HUGE = (32800, 2048)
NBLK = {(33, 2048): 2, (65, 2048): 3, (100, 2048): 4, (1025, 64): 2, (1100, 64): 2, (8200, 8): 2, BIG: 257, HUGE: 994}
UNROLL = (16484, 2048)  # 4 219 904 vectors: the U = 4 loop (needs > 3 x 4096 x 256) and its tail


def _gen(*ints):
    seed = 0
    for v in ints:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _plan(R, C):
    """reduce_plan of batchnorm.hip:284-295."""
    rpi = 256 // (C // 8)
    target = min(max(-(-R // (rpi * 32)), 1), 1024)
    rpb = -(-(-(-R // target)) // rpi) * rpi
    return dict(rpi=rpi, rpb=rpb, nblk=-(-R // rpb))


def _depth(R, C):
    p = _plan(R, C)
    return p["rpb"] // p["rpi"] + (p["rpi"] - 1) + -(-p["nblk"] // 256) + 6 + 3


def _fma(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 is exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


def _emu_sums(t1, p, q, R, C):
    """S1 = sum t1, S2 = sum p * q over the rows of [R, c] fp32 tensors, in the kernels' order and precision:
      * a thread adds the rows rb + r0, rb + r0 + rpi, .. of its block in turn, s2 by fmaf   batchnorm.hip:53-79
      * the rpi rows of an iteration are folded through LDS in turn                          :98-102
      * reduce_partials: thread t folds blocks t, t + 256, .. in turn, a 64-lane xor          :114-129
        butterfly, then red[0] + red[1] + red[2] + red[3]"""
    pl = _plan(R, C)
    rpi, rpb, nblk = pl["rpi"], pl["rpb"], pl["nblk"]
    c = t1.shape[1]
    pad = nblk * rpb - R
    shape = lambda t: torch.nn.functional.pad(t, (0, 0, 0, pad)).view(nblk, rpb // rpi, rpi, c)  # noqa: E731
    t1, p, q = shape(t1), shape(p), shape(q)
    s = torch.zeros(2, nblk, rpi, c, dtype=torch.float32, device=t1.device)
    for i in range(rpb // rpi):
        s = torch.stack([s[0] + t1[:, i], _fma(p[:, i], q[:, i], s[1])])
    part = s[:, :, 0]
    for j in range(1, rpi):
        part = part + s[:, :, j]
    folds = -(-nblk // 256)
    part = torch.nn.functional.pad(part, (0, 0, 0, folds * 256 - nblk)).view(2, folds, 256, c)
    a = part[:, 0]
    for f in range(1, folds):
        a = a + part[:, f]
    a = a.view(2, 4, 64, c)
    lane = torch.arange(64, device=t1.device)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lane ^ o]
    red = a[:, :, 0]
    tot = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    return tot[0], tot[1]


# ------------------------------------------------------------------------------------------ the oracles
def _stats_oracle(x, R, C, keep=None):
    """x [R, c] bf16 -> mean, var (biased), unbiased var, E2 and k of each channel, fp64. ``keep`` [R] bool: the
    rows whose terms reach the sums (the slips that lose block partials); the divisor stays R."""
    xd = x.double()
    k = xd[0]
    d = xd - k
    e2 = (d * d).sum(0) / R
    if keep is not None:
        d = d * keep.to(d.dtype)[:, None]
    m1 = d.sum(0) / R
    var = (d * d).sum(0) / R - m1 * m1
    return dict(mean=k + m1, var=var, unbiased=var * (R / (R - 1)) if R > 1 else var, e2=e2, k=k)


def _var_bound(want, R, C):
    return (3 * _depth(R, C) + 7) * U * want["e2"] + 2.0 ** -20 * (want["var"] + EPS)


def _out_oracle(x, res, scale, shift, relu, emulate=False, store=True):
    """act(x * scale + shift [+ res]) in fp64 and the magnitudes |x scale| + |shift| + |res|. emulate: fmaf, the
    fp32 sum with the residual and (``store``) the bf16 store (batchnorm.hip:209-220)."""
    xd, sc, sh = x.double(), scale.double(), shift.double()
    mags = (xd * sc).abs() + sh.abs()
    f = _fma(x.float(), scale.float().expand_as(x), shift.float().expand_as(x)) if emulate else xd * sc + sh
    if res is not None:
        mags = mags + res.double().abs()
        f = f + res.float() if emulate else f + res.double()
    if relu:
        f = f.clamp_min(0)
    return (f.bfloat16().double() if emulate and store else f.double()), mags


def _bwd_oracle(x, dy, out, stats, gamma, coef, R, relu, emulate=False):
    """The backward from ITS inputs (dy, the forward kernel's out as ReLU mask, x, the kernel's stats; dx from
    the kernel's coef): g, the terms of Sg and Sgx, dgamma, dbeta, A, B, D, dx, all fp64. emulate (needs C =
    x.shape[1]): the sums by ``_emu_sums`` with xf - mean rounded to fp32 (batchnorm.hip:75-76), the finalize in
    fp32 (:175-181), dx = bf16(fmaf(A, g, fmaf(B, x, D))) (:274-275)."""
    g = dy.double()
    if relu:
        g = g * (out.double() > 0)
    mean, invstd = stats[0].double(), stats[1].double()
    gam = torch.ones_like(mean) if gamma is None else gamma.double()
    tgx = g * (x.double() - mean)
    w = dict(g=g, tg=g, tgx=tgx)
    if emulate:
        C = x.shape[1]
        xm = x.float() - stats[0].float()
        sg, sgx = _emu_sums(g.float(), g.float(), xm, R, C)
        iv, mn, Rf = stats[1].float(), stats[0].float(), torch.tensor(float(R), dtype=torch.float32)
        A = gam.float() * iv
        B = -A * iv * iv * (sgx / Rf)
        w.update(dgamma=(sgx * iv).double(), dbeta=sg.double(), A=A.double(), B=B.double(),
                 D=(-A * (sg / Rf) - B * mn).double())
        cf = torch.stack([w["A"], w["B"], w["D"]]).float() if coef is None else coef.float()
        inner = _fma(cf[1].expand_as(xm), x.float(), cf[2].expand_as(xm))
        w["dx32"] = _fma(cf[0].expand_as(xm), g.float(), inner).double()
        w["dx"] = w["dx32"].bfloat16().double()
        w["coef"] = cf
        return w
    sg, sgx = g.sum(0), tgx.sum(0)
    A = gam * invstd
    B = -A * invstd * invstd * sgx / R
    w.update(dgamma=sgx * invstd, dbeta=sg, A=A, B=B, D=-A * sg / R - B * mean, sg=sg, sgx=sgx)
    if coef is not None:
        cf = coef.double()
        w["dx"] = cf[0] * g + cf[1] * x.double() + cf[2]
        w["dx_mags"] = (cf[0] * g).abs() + (cf[1] * x.double()).abs() + cf[2].abs()
    return w


# ------------------------------------------------------------------------------------------ the checkers
class _Shares(dict):
    def up(self, kind, value):
        v = float(value.max()) if value.numel() else 0.0
        v = math.inf if math.isnan(v) else v
        self[kind] = max(self.get(kind, 0.0), v)


def _elem(got, want, mags, kind):
    """Per element: the share of REL |want| + A mags that |got - want| uses (<= 1 passes)."""
    a, b = got.double(), want
    diff = (a - b).abs()
    diff = torch.where((b.abs() < TINY) & (a == 0), torch.zeros_like(diff), diff)  # a flushed denormal
    share = diff / (BOUND[kind + ".rel"] * b.abs() + BOUND[kind + ".a"] * mags).clamp_min(1e-300)
    return torch.where(diff > 0, share, torch.zeros_like(share))


def _elem_floors(raw, kind, f32, want, mags):
    """The two parts of an element's error in the emulate mode: REL, the bf16 store of the fp32 result f32, and
    A, the fp32 result against the exact one over the magnitudes. |bf16(f32) - want| <= 2**-8 |f32| + |f32 -
    want| <= REL |want| + (1 + 2**-8) A mags."""
    ok = f32.abs() >= TINY
    raw.up(kind + ".rel", ((f32.bfloat16().double() - f32).abs() / f32.abs().clamp_min(TINY))[ok])
    raw.up(kind + ".a", ((f32 - want).abs() / mags.clamp_min(1e-300))[mags > 0])


def _score_fwd(got, c, R, C, relu, raw=None):
    """got: stats [4, c], out (or None), rm, rv (or None) on the device of the inputs c (x, res, gamma, beta,
    rm0, rv0, mom; absent ones None) -> the share of its bound every quantity uses (<= 1 passes). ``raw``
    collects the unnormalised errors of the floored quantities."""
    sh, raw = _Shares(), (_Shares() if raw is None else raw)
    x = c["x"]
    want = _stats_oracle(x, R, C)
    st = got["stats"].double()
    assert got["stats"].dtype == torch.float32 and bool(torch.isfinite(st).all()), "stats not finite"
    err = (st[0] - want["mean"]).abs() / (want["k"].abs() + want["e2"].sqrt()).clamp_min(1e-300)
    raw.up("mean", err)
    sh.up("mean", err / BOUND["mean"])
    vb = _var_bound(want, R, C)
    sh.up("var", (st[1] ** -2 - EPS - want["var"]).abs() / vb)
    gam = torch.ones_like(st[0]) if c.get("gamma") is None else c["gamma"].double()
    bet = torch.zeros_like(st[0]) if c.get("beta") is None else c["beta"].double()
    err = (st[2] - gam * st[1]).abs() / (gam * st[1]).abs()
    raw.up("scale", err)
    sh.up("scale", err / BOUND["scale"])
    err = (st[3] - (bet - st[0] * st[2])).abs() / (bet.abs() + (st[0] * st[2]).abs()).clamp_min(1e-300)
    raw.up("shift", err)
    sh.up("shift", err / BOUND["shift"])
    if got.get("rm") is not None:
        m, rm0, rv0 = c["mom"], c["rm0"].double(), c["rv0"].double()
        mb = BOUND["mean"] * (want["k"].abs() + want["e2"].sqrt())
        ub = vb * (R / (R - 1) if R > 1 else 1.0)
        a, b = (1 - m) * rm0, m * want["mean"]
        sh.up("running_mean", (got["rm"].double() - (a + b)).abs() / (m * mb + 2.0 ** -21 * (a.abs() + b.abs()) + 1e-300))
        a, b = (1 - m) * rv0, m * want["unbiased"]
        sh.up("running_var", (got["rv"].double() - (a + b)).abs() / (m * ub + 2.0 ** -21 * (a.abs() + b.abs())))
        if m == 1.0:
            assert torch.equal(got["rm"], got["stats"][0]), "running_mean with momentum 1 is not the mean"
    if got.get("out") is not None:
        assert got["out"].dtype == torch.bfloat16 and bool(torch.isfinite(got["out"]).all()), "out not finite"
        wo, mags = _out_oracle(x, c.get("res"), got["stats"][2], got["stats"][3], relu)
        sh.up("out", _elem(got["out"], wo, mags, "out"))
    return sh


def _score_bwd(got, c, out, stats, R, C, relu, raw=None):
    """got: dx, dres (or None), dgamma, dbeta (or None), coef [3, c]."""
    sh, raw = _Shares(), (_Shares() if raw is None else raw)
    n = _depth(R, C) + 2
    w = _bwd_oracle(c["x"], c["dy"], out, stats, c.get("gamma"), got["coef"], R, relu)
    for name in ("coef", "dgamma", "dbeta"):
        if got.get(name) is not None:
            assert got[name].dtype == torch.float32 and bool(torch.isfinite(got[name]).all()), name
    invstd, mean = stats[1].double(), stats[0].double()
    bg = n * U * w["tg"].abs().sum(0)       # of Sg
    bgx = n * U * w["tgx"].abs().sum(0)     # of Sgx
    if got.get("dbeta") is not None:
        sh.up("dbeta", (got["dbeta"].double() - w["dbeta"]).abs() / (2.0 ** -21 * w["sg"].abs() + bg + 1e-300))
    if got.get("dgamma") is not None:
        sh.up("dgamma", (got["dgamma"].double() - w["dgamma"]).abs()
              / (2.0 ** -21 * w["dgamma"].abs() + invstd * bgx + 1e-300))
    cf = got["coef"].double()
    sh.up("coef.A", (cf[0] - w["A"]).abs() / (2.0 ** -22 * w["A"].abs() + 1e-300))
    bB = (w["A"] * invstd * invstd / R).abs() * bgx + 2.0 ** -21 * w["B"].abs()
    sh.up("coef.B", (cf[1] - w["B"]).abs() / (bB + 1e-300))
    p1, p2 = w["A"] * w["sg"] / R, w["B"] * mean
    bD = (w["A"] / R).abs() * bg + mean.abs() * bB + 2.0 ** -21 * (p1.abs() + p2.abs())
    sh.up("coef.D", (cf[2] - w["D"]).abs() / (bD + 1e-300))
    assert got["dx"].dtype == torch.bfloat16 and bool(torch.isfinite(got["dx"]).all()), "dx not finite"
    sh.up("dx", _elem(got["dx"], w["dx"], w["dx_mags"], "dx"))
    if got.get("dres") is not None:
        wrong = got["dres"].double() != w["g"]  # bit for bit: any difference is infinitely far out
        sh.up("dres", torch.where(wrong, torch.full_like(w["g"], math.inf), torch.zeros_like(w["g"])))
    return sh


def _assert_shares(sh, label):
    print(f"{label}: " + "  ".join(f"{k} {v:.2f}" for k, v in sh.items()))
    bad = {k: v for k, v in sh.items() if not v <= 1.0}
    assert not bad, (label, bad)


# --------------------------------------------------------------------------------------------- the data
def _gamma(C, g):
    return (0.5 + 0.25 * ((torch.arange(C) // 8) % 5) + 0.1 * torch.rand(C, generator=g)).float()


@functools.lru_cache(maxsize=None)
def _case(R, C, kind):
    """x, res, dy [R, C] bf16; gamma, beta, rm0, rv0 [C] fp32; all on the CPU."""
    g = _gen(R, C, KINDS.index(kind))
    z = torch.randn(R, C, generator=g)
    col = torch.arange(C)
    if kind == "random":
        x = 1.0 + 2.0 * z
    elif kind == "offset":
        x = 40.0 + 0.5 * z
    elif kind == "outlier-row0":
        x = z
        x[0] = 90.5 * (1 - 2 * (col % 2))  # 64 sigma at R = 8200: sigma**2 = 1 + 90.5**2 / 8200 = 2
    elif kind == "mixed":
        x = z * torch.tensor([2.0 ** -8, 1.0, 2.0 ** 6])[col % 3]
    else:
        x = 0.5 + z
    x = x.bfloat16()
    gamma, beta = _gamma(C, g), torch.randn(C, generator=g)
    res = torch.randn(R, C, generator=g)
    if kind == "relu-edge":
        s = _stats_oracle(x, R, C)
        scale = gamma.double() / (s["var"] + EPS).sqrt()
        pre = x.double() * scale + (beta.double() - s["mean"] * scale)
        res = torch.where(torch.rand(R, C, generator=g) < 0.5, -pre.float(), res)
    return dict(x=x, res=res.bfloat16(), dy=torch.randn(R, C, generator=g).bfloat16(), gamma=gamma, beta=beta,
                rm0=torch.randn(C, generator=g), rv0=0.5 + torch.rand(C, generator=g))


def _inputs(R, C, kind, res=True, affine=True, mom=1.0, cols=None):
    c = dict(_case(R, C, kind))
    if cols is not None:
        c = {k: (v[:, cols] if v.dim() == 2 else v[cols]) for k, v in c.items()}
    if not res:
        c["res"] = None
    if not affine:
        c["gamma"] = c["beta"] = None
    c["mom"] = mom
    if mom == 1.0:
        c["rm0"], c["rv0"] = torch.zeros_like(c["rm0"]), torch.zeros_like(c["rv0"])
    elif mom is None:
        c["rm0"] = c["rv0"] = None
    return c


def _huge_x(rows, cols, device):
    """The HUGE case: an integer formula (the same bits on any device), about uniform on [-4, 4)."""
    r = torch.arange(rows, device=device, dtype=torch.int64)[:, None]
    c = cols.to(device=device, dtype=torch.int64)[None, :]
    h = (r * 7919 + c * 104729 + (r ^ c) * 31) % 65521
    return ((h - 32760).float() / 8192.0).bfloat16()


# ------------------------------------------------------------------ the kernels as the oracles model them
def _fake_kernel(c, R, C, relu, slip=None):
    """What the three forward and the three backward kernels store, computed by the emulate modes on the CPU:
    the floors are measured on it, and the slips (see ``test_checker_rejects_*``) are built into it.
    Forward finalize in fp32 (batchnorm.hip:143-158), rsqrtf one ulp off."""
    x = c["x"]
    xf = x.float()
    d = xf - xf[0]
    pl = _plan(R, C)
    blk = torch.arange(R) // pl["rpb"]
    if slip == "last-block":
        d = d * (blk != pl["nblk"] - 1).float()[:, None]
    elif slip == "257th-block":
        d = d * (blk % 257 != 256).float()[:, None]
    s1, s2 = _emu_sums(d, d, d, R, C)
    Rf = torch.tensor(float(R), dtype=torch.float32)
    m1 = s1 / Rf
    var = (s2 / Rf - m1 * m1).clamp_min(0)
    mean = xf[0] + m1
    invstd = torch.nextafter(((var + EPS).double() ** -0.5).float(), torch.tensor(math.inf))
    gam = torch.ones_like(mean) if c["gamma"] is None else c["gamma"]
    bet = torch.zeros_like(mean) if c["beta"] is None else c["beta"]
    scale = gam * invstd
    stats = torch.stack([mean, invstd, scale, bet - mean * scale])
    got = dict(stats=stats)
    if c["rm0"] is not None:
        m = torch.tensor(c["mom"], dtype=torch.float32)
        unb = var * (Rf / (Rf - 1)) if R > 1 and slip != "biased" else var
        got["rm"] = (1 - m) * c["rm0"] + m * mean
        got["rv"] = (1 - m) * c["rv0"] + m * unb
    ascale = stats[2]
    if slip == "neighbour-scale":  # channel group 1 reads the scale of group 2 (of group 0 where there are 2)
        ascale = stats[2].clone()
        nb = 2 if C >= 24 else 0
        ascale[8:16] = stats[2][8 * nb: 8 * nb + 8]
    got["out"] = _out_oracle(x, c["res"], ascale, stats[3], relu, emulate=True)[0].bfloat16()
    mask_src = got["out"]
    if slip == "mask-before-residual":
        mask_src = _out_oracle(x, None, stats[2], stats[3], relu, emulate=True)[0]
    w = _bwd_oracle(x, c["dy"], mask_src, stats, c["gamma"], None, R, relu, emulate=True)
    coef = w["coef"]
    if slip == "D-without-B-mean":
        coef = coef.clone()
        coef[2] = (-w["A"] * w["dbeta"] / R).float()
        w = _bwd_oracle(x, c["dy"], mask_src, stats, c["gamma"], coef, R, relu, emulate=True)
    got.update(coef=coef, dx=w["dx"].bfloat16(), dgamma=w["dgamma"].float(), dbeta=w["dbeta"].float(),
               dres=w["g"].bfloat16() if c["res"] is not None else None)
    return got


def _fake_shares(c, R, C, relu, slip=None, raw=None):
    got = _fake_kernel(c, R, C, relu, slip)
    sh = _score_fwd(got, c, R, C, relu, raw)
    sh.update(_score_bwd(got, c, got["out"], got["stats"], R, C, relu, raw))
    if raw is not None:
        st = got["stats"]
        wo, mags = _out_oracle(c["x"], c["res"], st[2], st[3], relu)
        _elem_floors(raw, "out", _out_oracle(c["x"], c["res"], st[2], st[3], relu, emulate=True, store=False)[0], wo, mags)
        w = _bwd_oracle(c["x"], c["dy"], got["out"], st, c["gamma"], got["coef"], R, relu)
        em = _bwd_oracle(c["x"], c["dy"], got["out"], st, c["gamma"], got["coef"], R, relu, emulate=True)
        _elem_floors(raw, "dx", em["dx32"], w["dx"], w["dx_mags"])
    return sh


def _runs():
    """(R, C, kind, relu, res, affine, mom) of every forward + backward run of the file."""
    runs = []
    for R, C in SMALL + RAGGED:
        kinds = KINDS if (R, C) in RAGGED else tuple(k for k in KINDS if k != "outlier-row0")
        runs += [(R, C, "random", relu, res, True, 1.0) for relu, res in FLAGS]
        runs += [(R, C, kind, True, True, True, MOM) for kind in kinds]
    runs += [(R, C, "random", relu, res, True, 1.0) for R, C in ROW1 for relu, res in FLAGS]
    runs += [(R, C, "random", True, True, True, 1.0) for R, C in CHANNELS]
    runs += [(1100, 64, "random", True, True, False, None), (1025, 64, "offset", False, False, False, None)]
    return runs


BIG_RUNS = [("random", True, True, True, 1.0), ("outlier-row0", True, True, True, MOM), ("random", True, False, False, None)]
SUB = torch.cat([torch.arange(64), torch.arange(1984, 2048)])  # the channels the CPU tests take of BIG and HUGE


# ============================================================================== CPU tests: the bounds
def test_plans_reach_the_paths_the_cases_are_named_for():
    for (R, C), nblk in NBLK.items():
        assert _plan(R, C)["nblk"] == nblk, (R, C, _plan(R, C))
    assert all(_plan(R, C)["nblk"] == 1 for R, C in SMALL + ROW1 + CHANNELS)
    assert NBLK[BIG] > 256 and BIG[0] * BIG[1] // 8 > 4096 * 256
    assert _plan(*HUGE)["rpb"] == 33 and -(-HUGE[0] // 32) > 1024  # the target hit its cap: more than 32 rows a block
    assert UNROLL[0] * UNROLL[1] // 8 > 4 * 4096 * 256  # the unrolled loop and a tail
    assert _plan(65, 2048)["rpb"] * 3 != 65 and _plan(1025, 64)["rpb"] * 2 != 1025 and _plan(8200, 8)["rpb"] * 2 != 8200


def _floors():
    raw, derived = _Shares(), _Shares()
    for R, C, kind, relu, res, affine, mom in _runs():
        derived_run = _fake_shares(_inputs(R, C, kind, res, affine, mom), R, C, relu, raw=raw)
        for k, v in derived_run.items():
            derived.up(k, torch.tensor(v))
    for kind, relu, res, affine, mom in BIG_RUNS:  # a channel subset: the channels are independent
        c = _inputs(*BIG, kind, res, affine, mom, cols=SUB)
        for k, v in _fake_shares(c, *BIG, relu, raw=raw).items():
            derived.up(k, torch.tensor(v))
    c = dict(x=_huge_x(HUGE[0], SUB, "cpu"), res=None, gamma=None, beta=None, rm0=None, rv0=None, mom=None, dy=None)
    got = _fake_kernel(dict(c, dy=torch.zeros_like(c["x"])), *HUGE, False)
    for k, v in _score_fwd(dict(stats=got["stats"]), c, *HUGE, False, raw).items():
        derived.up(k, torch.tensor(v))
    return raw, derived


def test_bounds_are_twice_the_measured_floors():
    """The reference for BOUND, and the emulate mode inside every derived bound."""
    f, derived = _floors()
    for kind in BOUND:
        print(f"    {kind:<10} {f[kind]:.2e}   2**{math.log2(BOUND[kind]):.0f} = {BOUND[kind]:.2e}")
    print("    derived bounds, share used by the emulate mode: "
          + "  ".join(f"{k} {v:.2f}" for k, v in derived.items() if k not in ("mean", "scale", "shift", "out", "dx", "dres")))
    for kind in BOUND:
        assert 0 < f[kind] <= BOUND[kind] / 2, (kind, f[kind])
        assert BOUND[kind] == 2.0 ** math.ceil(math.log2(2 * f[kind])), (kind, f[kind])
    assert all(v <= 1.0 for v in derived.values()), derived
    assert BOUND["out.rel"] < 1 and BOUND["dx.rel"] < 1


def test_data_conditions():
    for R, C in RAGGED + [BIG]:
        cols = SUB if (R, C) == BIG else None
        s = _stats_oracle(_inputs(R, C, "offset", cols=cols)["x"], R, C)
        assert bool((s["mean"].abs() > 40 * s["var"].sqrt()).all())  # mean 40, std 0.5: the shift matters
        s = _stats_oracle(_inputs(R, C, "outlier-row0", cols=cols)["x"], R, C)
        far = (s["k"] - s["mean"]).abs() / s["var"].sqrt()
        if R == 8200:  # 64 sigma; the outlier barely moves the true variance, and the bound stays under the variance
            assert bool((far > 60).all()) and bool((far < 68).all()), (R, C, float(far.min()), float(far.max()))
            assert bool((s["var"] < 2.2).all()) and bool((_var_bound(s, R, C) < 0.25 * s["var"]).all())
        c = _inputs(R, C, "relu-edge", cols=cols)
        st = _fake_kernel(c, R, C, True)["stats"] if cols is None else None
        if st is not None:
            pre, _ = _out_oracle(c["x"], c["res"], st[2], st[3], False)
            p0, _ = _out_oracle(c["x"], None, st[2], st[3], False)
            near = pre.abs() <= 2.0 ** -7 * p0.abs()  # within one bf16 ulp of the term that was cancelled
            assert float(near.double().mean()) > 0.4, (R, C, float(near.double().mean()))
        s = _stats_oracle(_inputs(R, C, "mixed", cols=cols)["x"], R, C)
        assert float(s["var"].max() / s["var"].min()) > 2.0 ** 26
    g = _case(100, 2048, "random")["gamma"].view(-1, 8)
    assert bool(((g[1:] - g[:-1]).abs().amin(1) > 0.1).all())  # neighbouring channel groups differ


# ================================================================ CPU tests: the checkers reject slips
def _rejected(sh, *kinds):
    return [k for k in kinds if not sh.get(k, 0.0) <= 1.0]


@pytest.mark.parametrize("R,C", [(33, 2048), (100, 2048), (1100, 64)])
def test_checker_rejects_the_biased_variance_in_running_var(R, C):
    c = _inputs(R, C, "random", mom=1.0)
    _assert_shares(_fake_shares(c, R, C, True), "intact")
    assert _rejected(_fake_shares(c, R, C, True, slip="biased"), "running_var") == ["running_var"]
    c = _inputs(R, C, "random", mom=MOM)
    assert _rejected(_fake_shares(c, R, C, True, slip="biased"), "running_var") == ["running_var"]


@pytest.mark.parametrize("R,C", RAGGED)
@pytest.mark.parametrize("kind", ["random", "offset"])
def test_checker_rejects_the_dropped_partials_of_the_last_block(R, C, kind):
    c = _inputs(R, C, kind)
    _assert_shares(_fake_shares(c, R, C, True), "intact")
    sh = _fake_shares(c, R, C, True, slip="last-block")
    assert "var" in _rejected(sh, "var", "mean", "running_var"), sh
    # not just one channel: each whose variance the lost rows move by more than twice its bound
    bad = _fake_kernel(c, R, C, True, slip="last-block")["stats"].double()
    want = _stats_oracle(c["x"], R, C)
    pl = _plan(R, C)
    lost = _stats_oracle(c["x"], R, C, keep=torch.arange(R) < (pl["nblk"] - 1) * pl["rpb"])
    felt = (lost["var"] - want["var"]).abs() > 2 * _var_bound(want, R, C)
    assert float(felt.double().mean()) > 0.9
    assert bool(((bad[1] ** -2 - EPS - want["var"]).abs() > _var_bound(want, R, C))[felt].all())


def test_checker_rejects_every_257th_block_partial_dropped():
    """reduce_partials without its loop: block 256 of BIG's 257, rows 8192..8199 of 8200."""
    for kind in ("random", "outlier-row0"):
        c = _inputs(*BIG, kind, cols=SUB)
        _assert_shares(_fake_shares(c, *BIG, True), "intact")
        bad = _fake_kernel(c, *BIG, True, slip="257th-block")["stats"].double()
        want = _stats_oracle(c["x"], *BIG)
        rej = (bad[1] ** -2 - EPS - want["var"]).abs() > _var_bound(want, *BIG)
        lost = _stats_oracle(c["x"], *BIG, keep=torch.arange(BIG[0]) < 8192)
        felt = (lost["var"] - want["var"]).abs() > 2 * _var_bound(want, *BIG)
        assert felt.sum() >= 0.75 * len(SUB) and bool(rej[felt].all()), (kind, int(felt.sum()))


@pytest.mark.parametrize("R,C", [(480, 64), (100, 2048), (8200, 8)])
def test_checker_rejects_a_relu_mask_taken_before_the_residual_add(R, C):
    c = _inputs(R, C, "random")
    got = _fake_kernel(c, R, C, True, slip="mask-before-residual")
    good = _fake_kernel(c, R, C, True)
    sh = _score_bwd(got, c, good["out"], good["stats"], R, C, True)
    assert set(_rejected(sh, "dres", "dx", "dbeta", "dgamma")) >= {"dres", "dx", "dbeta"}, sh
    # each element whose two masks differ and whose dy is not zero
    differ = ((good["out"] > 0) != (_out_oracle(c["x"], None, good["stats"][2], good["stats"][3], True)[0] > 0))
    differ &= c["dy"] != 0
    assert differ.any() and bool((got["dres"] != good["dres"])[differ].all())


@pytest.mark.parametrize("R,C", [(480, 64), (65, 2048), (8200, 8)])
@pytest.mark.parametrize("kind", ["random", "offset"])
def test_checker_rejects_a_d_coefficient_without_b_mean(R, C, kind):
    c = _inputs(R, C, kind)
    sh = _fake_shares(c, R, C, True, slip="D-without-B-mean")
    assert set(_rejected(sh, "coef.D", "coef.A", "coef.B")) == {"coef.D"}, sh
    # the checker of dx follows the kernel's own coef, so it is coef.D alone that sees the slip -- in every
    # channel whose B * mean stands above twice the bound of D
    got, good = _fake_kernel(c, R, C, True, slip="D-without-B-mean"), _fake_kernel(c, R, C, True)
    gone = (good["coef"][1].double() * good["stats"][0].double()).abs()
    moved = (got["coef"][2] - good["coef"][2]).abs().double()
    assert bool((moved > 0.5 * gone)[gone > 1e-4].all()) and float((gone > 1e-4).double().mean()) > 0.5


@pytest.mark.parametrize("R,C", [(19, 16), (480, 64), (100, 2048)])
def test_checker_rejects_a_channel_group_reading_its_neighbours_scale(R, C):
    c = _inputs(R, C, "random")
    got = _fake_kernel(c, R, C, True, slip="neighbour-scale")
    sh = _score_fwd(got, c, R, C, True)
    assert _rejected(sh, "out", "mean", "var", "scale", "shift") == ["out"], sh
    good = _fake_kernel(c, R, C, True)
    wo, mags = _out_oracle(c["x"], c["res"], good["stats"][2], good["stats"][3], True)
    share = _elem(got["out"], wo, mags, "out")
    assert bool((share[:, :8] <= 1).all()) and bool((share[:, 16:] <= 1).all())
    # each element of the group that is not cut off by the ReLU and that the wrong scale moves by twice its bound
    moved = (c["x"].double() * (got["stats"][2] - good["stats"][2].roll(-8 if C >= 24 else 8)).double())[:, 8:16].abs()
    tol = (BOUND["out.rel"] * wo.abs() + BOUND["out.a"] * mags)[:, 8:16]
    felt = (good["out"][:, 8:16] > 0) & (got["out"][:, 8:16] > 0) & (moved > 2 * tol)
    assert float(felt.double().mean()) > 0.3 and bool((share[:, 8:16] > 1)[felt].all())


def test_checker_rejects_a_zeroed_element():
    R, C = 480, 64
    c = _inputs(R, C, "random", res=False)
    got = _fake_kernel(c, R, C, False)
    wo, mags = _out_oracle(c["x"], None, got["stats"][2], got["stats"][3], False)
    zero = torch.zeros_like(got["out"])
    share = _elem(zero, wo, mags, "out")
    assert bool((share > 1)[wo.abs() > 2 * BOUND["out.a"] * mags].all()) and float((share > 1).double().mean()) > 0.99


# ========================================================================================= GPU tests
def _p(t):
    return 0 if t is None else t.data_ptr()


def _lib_call(name, *args):
    from ray_community_amd.ops._lib import check, stream_ptr

    check(getattr(ops.lib(), name)(*args, stream_ptr(torch.device("cuda"))), name)


def _bn_run(c, R, C, relu, backward=True):
    """c on the device -> what rca_bn_fwd and rca_bn_bwd wrote, and the plan's block count."""
    L = ops.lib()
    nws = int(L.rca_bn_workspace(R, C))
    assert nws % (2 * C) == 0
    ws = torch.empty(nws, device="cuda")
    x = c["x"]
    stats = torch.empty(4, C, device="cuda")
    out = torch.empty_like(x)
    rm = None if c["rm0"] is None else c["rm0"].clone()
    rv = None if c["rv0"] is None else c["rv0"].clone()
    mom = 0.0 if c["mom"] is None else c["mom"]
    _lib_call("rca_bn_fwd", x.data_ptr(), _p(c["res"]), _p(c["gamma"]), _p(c["beta"]), _p(rm), _p(rv), stats.data_ptr(),
              ws.data_ptr(), out.data_ptr(), R, C, EPS, mom, int(relu))
    got = dict(stats=stats, out=out, rm=rm, rv=rv, nblk=nws // (2 * C))
    if backward:
        coef = torch.empty(3, C, device="cuda")
        dx = torch.empty_like(x)
        dres = None if c["res"] is None else torch.empty_like(x)
        dgamma = None if c["gamma"] is None else torch.empty(C, device="cuda")
        dbeta = None if c["beta"] is None else torch.empty(C, device="cuda")
        _lib_call("rca_bn_bwd", c["dy"].data_ptr(), out.data_ptr(), x.data_ptr(), stats.data_ptr(), _p(c["gamma"]),
                  _p(dgamma), _p(dbeta), coef.data_ptr(), ws.data_ptr(), dx.data_ptr(), _p(dres), R, C, int(relu))
        got.update(coef=coef, dx=dx, dres=dres, dgamma=dgamma, dbeta=dbeta)
    torch.cuda.synchronize()
    return got


def _to(c, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _run_and_check(R, C, kind, relu, res, affine, mom, on_device=False):
    """One forward + backward through lib(), scored on the CPU (on the device for the large cases)."""
    c = _inputs(R, C, kind, res, affine, mom)
    dc = _to(c, "cuda")
    got = _bn_run(dc, R, C, relu)
    assert got["nblk"] == _plan(R, C)["nblk"] == NBLK.get((R, C), 1), (R, C, got["nblk"])
    if on_device:
        c = dc
    else:
        got = _to(got, "cpu")
    sh = _score_fwd(got, c, R, C, relu)
    sh.update(_score_bwd(got, c, got["out"], got["stats"], R, C, relu))
    _assert_shares(sh, f"bn R={R} C={C} {kind} relu={relu} res={res} affine={affine} mom={mom}")
    return dc, got


@gpu
@pytest.mark.parametrize("R,C", SMALL + ROW1 + CHANNELS + RAGGED, ids=str)
def test_bn_elems(R, C):
    mine = [r for r in _runs() if r[:2] == (R, C)]
    assert mine
    for run in mine:
        _run_and_check(*run)


@gpu
@pytest.mark.parametrize("run", BIG_RUNS, ids=str)
def test_bn_elems_over_256_blocks_and_the_apply_grid_cap(run):
    """257 partial rows (reduce_partials folds a second one into thread 0) and 2 099 200 vectors on 4096 x 256
    threads; the last run passes null gamma / beta and null running statistics."""
    dc, got = _run_and_check(*BIG, *run, on_device=True)
    assert got["nblk"] == 257


@gpu
def test_bn_forward_statistics_over_the_1024_block_cap():
    R, C = HUGE
    x = _huge_x(R, torch.arange(C), "cuda")
    c = dict(x=x, res=None, gamma=None, beta=None, rm0=torch.zeros(C, device="cuda"), rv0=torch.zeros(C, device="cuda"),
             mom=1.0)
    got = _bn_run(c, R, C, False, backward=False)
    assert got["nblk"] == NBLK[HUGE] == 994
    sh = _Shares()
    for lo in range(0, C, 256):
        cols = slice(lo, lo + 256)
        cc = dict(c, x=x[:, cols], rm0=c["rm0"][cols], rv0=c["rv0"][cols])
        part = dict(stats=got["stats"][:, cols], rm=got["rm"][cols], rv=got["rv"][cols], out=got["out"][:, cols])
        for k, v in _score_fwd(part, cc, R, C, False).items():
            sh.up(k, torch.tensor(v))
    _assert_shares(sh, f"bn R={R} C={C} forward statistics")


@gpu
def test_bn_apply_unrolled_by_four_is_bit_equal():
    R, C = UNROLL
    L = ops.lib()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(R, C, device="cuda", generator=g).bfloat16()
    res = torch.randn(R, C, device="cuda", generator=g).bfloat16()
    stats = torch.zeros(4, C, device="cuda")
    stats[2] = _gamma(C, _gen(5)).cuda()
    stats[3] = torch.randn(C, device="cuda", generator=g)
    outs = []
    old = L.rca_bn_set_unroll(1)
    try:
        for u in (1, 4):
            L.rca_bn_set_unroll(u)
            out = torch.full_like(x, float("nan"))
            _lib_call("rca_bn_apply", x.data_ptr(), res.data_ptr(), stats.data_ptr(), out.data_ptr(), R, C, 1)
            torch.cuda.synchronize()
            outs.append(out)
    finally:
        L.rca_bn_set_unroll(old)
    assert L.rca_bn_set_unroll(old) == old
    assert torch.equal(outs[0], outs[1])
    wo, mags = _out_oracle(x, res, stats[2], stats[3], True)
    share = _elem(outs[1], wo, mags, "out")
    del wo, mags
    _assert_shares(_Shares(out=float(share.max())), f"bn apply U=4 R={R} C={C}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_bn_wrappers_return_the_kernels_bits(kind):
    """ops.batch_norm_act with autograd and ops.affine_act_ against the lib() calls scored above."""
    R, C = 1100, 64
    dc, got = _run_and_check(R, C, kind, True, True, True, MOM, on_device=True)
    nchw = lambda t: t.view(1, R, 1, C).permute(0, 3, 1, 2)  # noqa: E731
    x, res = nchw(dc["x"]).clone().requires_grad_(True), nchw(dc["res"]).clone().requires_grad_(True)
    assert ops.bn_supported(x)
    w, b = dc["gamma"].clone().requires_grad_(True), dc["beta"].clone().requires_grad_(True)
    rm, rv = dc["rm0"].clone(), dc["rv0"].clone()
    out = ops.batch_norm_act(x, w, b, rm, rv, training=True, momentum=MOM, eps=EPS, residual=res, relu=True)
    out.backward(nchw(dc["dy"]))
    torch.cuda.synchronize()
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(R, C)  # noqa: E731
    assert torch.equal(flat(out), got["out"]) and torch.equal(rm, got["rm"]) and torch.equal(rv, got["rv"])
    assert torch.equal(flat(x.grad), got["dx"]) and torch.equal(flat(res.grad), got["dres"])
    assert torch.equal(w.grad, got["dgamma"]) and torch.equal(b.grad, got["dbeta"])
    y = nchw(dc["x"]).clone()
    assert ops.affine_act_(y, got["stats"], nchw(dc["res"]), True) is y
    assert torch.equal(flat(y), got["out"])


@gpu
def test_batch_norm_act_falls_back_for_parameters_the_kernel_cannot_read():
    """A bf16 bias, a strided weight: not float* rows of C, so the torch composition runs and gives the oracle's
    result. Its reduction order is torch's own: the statistics are allowed R u (a sequential sum) where the
    kernel has BOUND, per element A = R * 2**-24 * 4 for mean, scale, shift and the product."""
    R, C = 480, 64
    c = _inputs(R, C, "random", res=False)
    s = _stats_oracle(c["x"], R, C)
    nchw = lambda t: t.view(1, R, 1, C).permute(0, 3, 1, 2)  # noqa: E731
    x = nchw(c["x"].cuda())
    for which in ("bias", "weight"):
        gamma, beta = c["gamma"].cuda(), c["beta"].cuda()
        if which == "bias":
            beta = beta.bfloat16()
        else:
            gamma = torch.stack([gamma, gamma], 1)[:, 0]
            assert not gamma.is_contiguous()
        rm, rv = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        out = ops.batch_norm_act(x, gamma, beta, rm, rv, training=True, momentum=1.0, eps=EPS, relu=True)
        torch.cuda.synchronize()
        scale = gamma.double().cpu() / (s["var"] + EPS).sqrt()
        shift = beta.double().cpu() - s["mean"] * scale
        wo, mags = _out_oracle(c["x"], None, scale, shift, True)
        got = out.permute(0, 2, 3, 1).reshape(R, C).cpu()
        assert got.dtype == torch.bfloat16
        diff = (got.double() - wo).abs()
        tol = BOUND["out.rel"] * wo.abs() + 4 * R * U * mags
        print(f"fallback {which}: largest share {float((diff / tol.clamp_min(1e-300)).max()):.2f}")
        assert bool((diff <= tol).all()), which
        assert bool(((rm.double().cpu() - s["mean"]).abs() <= R * U * (s["k"].abs() + s["e2"].sqrt())).all())
