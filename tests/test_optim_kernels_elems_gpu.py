"""The optimizer half of ops/csrc/loss_optim.hip -- sumsq_partial_kernel, adamw_kernel, adamw_split_kernel
and adamw_split_seg_kernel -- checked per element against oracles written here in int64 and float64,
independent of ops/reference.py, of autograd and of the other kernels.

Metric.
  * Sum of squares: exact. The data are small integers (0, +-1, +-2, +-3) whose total sum of squares
    stays under 2**24, so every fp32 partial and every combination of partials is an exact integer in
    any order; ``got == int64 reference`` with ``==``.
  * AdamW: one update per element from inputs the test wrote itself (the ``sumsq`` word included, so
    the clip arithmetic is scored apart from the reduction). Each of the new master p, m and v is
    scored per element, |got - want| <= tol, in the GEMM form -- a relative constant times the sum of
    the absolute values of the terms that are added:
        m:  tol = B_m (|b1 m| + |(1 - b1) g'|)                      g' = g * grad_mul * clip_coef
        v:  tol = B_v v_new                                         (every term is positive)
        p:  tol = B_p (|p| + lr (wd |p| + |mh| / den)) + lr du      den = sqrt(vh) + eps
            du  = B_m (|b1 m| + |(1 - b1) g'|) / (bc1 den) + |mh| / den**2 * B_v sqrt(vh) / 2
    du is what u = wd p + mh / den inherits, to first order, from an m and a v that sit at their own
    bounds; cancellation in m's EMA therefore loosens that element's bound and no other. A term sum of
    zero leaves tol = 0: the value must be exact. Nothing is excused except an oracle value under the
    smallest fp32 normal (2**-126) that comes back as zero.
  * The bf16 copy of the fp32-master format equals the RNE rounding of the returned master exactly. In
    the split format hi equals it except at exact ties (lo == 0x8000), where hi is the upper half + 1:
    one ulp larger in magnitude than RNE when RNE rounds down, equal to it when RNE rounds up. Both the
    "only at ties" part and the direction are asserted.
  * Everything else is bitwise: the identity step of the split format, one grid setting against
    another, W^T against W.t(), padding and sentinel words against what they held before.

Bounds: none is taken from a kernel. ``_adam_oracle`` states the update exactly as adam_elem and
clip_coef do (it cites the lines); its ``emulate`` mode rounds to fp32 where the kernel rounds (the
hyper-parameters as the C call receives them, 1 - b1 and 1 - b2, g * gm, both products of the v term,
the three explicit fmas, both divisions, sqrtf, sqrtf + eps, and in clip_coef sqrtf, the product with
|grad_mul|, nrm + 1e-6f and the division). The floor of a quantity is the worst error of that mode
against the exact one, in units of the element's term sum, over every case of this file, computed on
the CPU; the bound is twice the floor rounded up to a power of two
(``test_bounds_are_twice_the_measured_floors``; p's floor is taken after m's and v's bounds, since du
uses them):

    quantity   floor      bound
    adam.m     4.22e-07   2**-20 = 9.54e-07   (1.f - 0.9f is 2.4e-7 from 0.1; four roundings of 6e-8 follow)
    adam.v     5.31e-07   2**-19 = 1.91e-06   (1.f - 0.95f is 2.4e-7 from 0.05; five roundings follow)
    adam.p     5.95e-08   2**-23 = 1.19e-07   (the last fma's rounding: half an fp32 ulp)

Data. Sum of squares: random integers at a density that keeps the total near 2**21, with non-zero
entries forced at every structural index (``_ss_struct``: the first and last element of the tensor,
of the first vectors, of each block-, trip- and loop-boundary vector, of the last vector of the
four-deep loop and the first of the one-deep loop, and every tail element); each tensor is a view at a
multiple of 64 elements into a buffer whose other words hold 2.0, so a read outside the view changes
the sum. AdamW (``_adam_case``): the elements cycle through seven classes -- generic; g = m = v = 0; g
= 0 with old state; m tuned against g' so that the EMA cancels to 2**-12 of its terms; generic with p
= +-0; m and g' of opposite sign; fresh state (m = v = 0) -- while |g| walks from 2**-40 to 2**20 (so
eps decides some elements and not others) and |p| over eight binades, both signs. The parameter sets
are the full cross of step {1, 10000} x wd {0, 0.1} x grad_mul {1, 0.5, -0.5} x clipping {off with a
null sumsq, sumsq given with max_norm = 0, active, inactive, sumsq == 0}; lr = 1e-3, betas (0.9,
0.95), eps = 1e-8. The size over the flat kernel's grid cap (4096 x 256 x 8 + 8 x 300 + 5) is scored
on every 1021st element plus the first and last vector of each trip and the tail, because the fp64
oracle of all 8.4 M elements takes longer than a test should; its bf16 copy is checked on every
element. The segmented cases run three steps; the floors take their inputs from a CPU trajectory of
the emulating oracle, the GPU test scores each step on the state the kernel itself left.

The tests without a ``gpu`` mark run anywhere: they recompute the floors, run the split / join table
through ops.reference on the CPU, and show that the checkers reject every slipped oracle listed in
``test_*_rejects_*`` on the elements the data class was built for.

The FlatParameters layout rounds every parameter to 64 elements, so the 1-D segments FlatAdamW builds
are multiples of 8 long even where the parameters are not (37, 131 x 37); the partial 8-group of a 1-D
tile is reached by the direct call alone. rca_adamw_split_seg cannot check R and C on the host (the
table is device memory); its contract comment now says 128 and names the Python caller that enforces it.

Measured on one MI355X (the whole file, CPU tests included, takes 11 s on the device, 33 tests; the
slowest GPU test 0.3 s, test_adamw_over_the_flat_grid_cap[g_bf16]; the slowest of all the floor table,
3 s). Worst share of an element's bound per test, m / v / p:
    test_adamw_elements[fp32 | master | split, g_bf16]      0.42  0.25  0.50  (the three formats alike)
    test_adamw_elements[fp32 | master | split, g_fp32]      0.38  0.25  0.49
    test_adamw_over_the_flat_grid_cap[g_bf16 / g_fp32]      0.36  0.25  0.49 / 0.38  0.25  0.48
    test_adamw_split_under_a_wrapped_grid (4 cases)         0.42  0.26  0.50
    test_adamw_segmented_under_wrapped_grids_...            0.44  0.28  0.44
    test_adamw_segmented_direct_call_...                    0.39  0.25  0.50
Every kernel sits on the emulating oracle's floor (half of a bound or less). The sums of squares, the
one-hot probes (41 bf16 and 37 fp32 indices), the identity step over all 393 221 patterns (denormals are
kept, not flushed), the bf16 copies, the tie rule of hi, W^T and the comparisons between grids were
exact on the first run. No kernel defect was found: loss_optim.hip changes in a comment only.
"""
import functools
import math

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.ops import reference

gpu = pytest.mark.gpu

TINY32 = 2.0 ** -126  # the smallest normal fp32
BOUND = {"adam.m": 2.0 ** -20, "adam.v": 2.0 ** -19, "adam.p": 2.0 ** -23}
LR, B1, B2, EPS_ADAM = 1e-3, 0.9, 0.95, 1e-8


def _gen(*ints):
    seed = 0
    for v in ints:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ===================================================================== 1. sum of squares
SS_BLK, SS_CAP = 256, 1024          # lanes per block, the block cap of rca_sumsq (loss_optim.hip:320-321)
SS_STRIDE = SS_BLK * SS_CAP         # vectors per trip of the capped grid


def _ss_vec(bf16):
    return 8 if bf16 else 4


def _ss_grid(n, bf16):
    """(nv, stride in vectors) of the launch rca_sumsq makes for n elements."""
    nv = n // _ss_vec(bf16)
    nb = min(SS_CAP, max(1, -(-nv // SS_BLK)))
    return nv, nb * SS_BLK


def _ss_sizes(bf16):
    vec, S = _ss_vec(bf16), SS_STRIDE
    sizes = [1, 7, 8, 9, SS_BLK * vec - 1, SS_BLK * vec, SS_BLK * vec + 1, (S - 1) * vec, S * vec, (S + 1) * vec]
    if bf16:  # nv = 3 S (no lane enters the four-deep loop), 3 S + 1 (lane 0 alone does), 3 S + 2
        sizes += [3 * S * vec + 5, (3 * S + 1) * vec + 5, (3 * S + 2) * vec + 5]
    sizes.append((4 * S + 1000) * vec + vec - 1)  # both loops in lanes 0..999, four one-deep trips in the rest, a tail
    return sizes


def _ss_struct(n, bf16):
    """The structural element indices of a size: see the module docstring."""
    vec = _ss_vec(bf16)
    nv, stride = _ss_grid(n, bf16)
    vs = {0, 1, nv - 1, SS_BLK - 1, SS_BLK}
    for k in (1, 2, 3, 4):
        vs |= {k * stride - 1, k * stride, k * stride + 1}
    if bf16 and nv > 3 * stride:
        lanes = min(stride, nv - 3 * stride)  # lanes 0 .. lanes - 1 take the four-deep loop (once: nv < 7 stride)
        assert nv < 7 * stride
        vs |= {lanes - 1, lanes - 1 + stride, lanes - 1 + 2 * stride, lanes - 1 + 3 * stride}  # its last vectors
        vs |= {lanes, lanes + 3 * stride, 4 * stride}  # the first vectors of the one-deep loop
    idx = {0, n - 1} | set(range(nv * vec, n))
    for k in vs:
        if 0 <= k < nv:
            idx |= {k * vec, k * vec + vec - 1}
    return sorted(i for i in idx if 0 <= i < n)


@functools.lru_cache(maxsize=None)
def _ss_case(n, bf16, pad64):
    """(buffer, pad, int64 sum of squares): the tensor is buffer[pad: pad + n], pad a multiple of 64."""
    g = _gen(11, n, bf16, pad64)
    pad = 64 * pad64
    dt = torch.bfloat16 if bf16 else torch.float32
    buf = torch.full((pad + n + 64,), 2.0, dtype=dt)
    if n == 0:
        return buf, pad, 0
    dens = min(1.0, 2.0 ** 21 / (14.0 / 3.0 * n))
    vals = torch.randint(1, 4, (n,), generator=g) * (1 - 2 * torch.randint(0, 2, (n,), generator=g))
    x = torch.where(torch.rand(n, generator=g) < dens, vals, torch.zeros_like(vals))
    st = torch.tensor(_ss_struct(n, bf16))
    x[st] = vals[st]
    total = int((x * x).sum())
    assert total < 2 ** 23
    buf[pad: pad + n] = x.to(dt)
    return buf, pad, total


def _ss_ref(x, bf16, drop=None):
    """int64 sum of squares of a tensor of integers. The slips: drop = ("vector", k), ("tail", j: an
    element index) or ("trip2",): the vectors of the second grid trip."""
    sq = x.long() ** 2
    total = int(sq.sum())
    vec = _ss_vec(bf16)
    nv, stride = _ss_grid(x.numel(), bf16)
    if drop is None:
        return total
    if drop[0] == "vector":
        return total - int(sq[drop[1] * vec: (drop[1] + 1) * vec].sum())
    if drop[0] == "tail":
        return total - int(sq[drop[1]])
    assert drop[0] == "trip2"
    return total - int(sq[stride * vec: min(2 * stride, nv) * vec].sum())


def _ss_check(got, want, label):
    assert got.dtype == torch.float32 and got.numel() == 1, label
    assert float(got) == want, (label, float(got), want)


SS_CHAIN = [(True, 9), (False, 0), (False, (SS_STRIDE + 1) * 4), (True, SS_BLK * 8 + 1), (True, 0), (False, 7),
            (True, (3 * SS_STRIDE + 1) * 8 + 5), (False, 1)]


# ===================================================================== 2. AdamW
def _f32(x):
    return x.float().double()


def _r32(x):
    return float(torch.tensor(float(x), dtype=torch.float64).float())


def _hp(step=1, wd=0.0, gm=1.0, sumsq=None, max_norm=0.0, lr=LR):
    return dict(lr=lr, b1=B1, b2=B2, eps=EPS_ADAM, wd=wd, step=step, gm=gm, sumsq=sumsq, max_norm=max_norm)


def _clip_coef(hp, emulate=False, slip=None):
    """clip_coef, loss_optim.hip:337-341: 1 without a sumsq pointer or with max_norm <= 0; else
    min(1, max_norm / (sqrtf(sumsq) * fabsf(grad_mul) + 1e-6f)). The slips: "clip_no_mul" leaves
    grad_mul out of the norm, "clip_no_fabs" uses it with its sign."""
    if hp["sumsq"] is None or hp["max_norm"] <= 0:
        return 1.0
    r = _r32 if emulate else float
    mul = 1.0 if slip == "clip_no_mul" else (r(hp["gm"]) if slip == "clip_no_fabs" else abs(r(hp["gm"])))
    nrm = r(r(math.sqrt(r(hp["sumsq"]))) * mul)
    return min(1.0, r(r(hp["max_norm"]) / r(nrm + r(1e-6))))


def _adam_oracle(st, hp, emulate=False, slip=None, wd=None):
    """p, g, m, v -> the new p, m, v in fp64, with the term sums of the metric. adam_elem,
    loss_optim.hip:347-355, called with g * gm, gm = grad_mul * clip_coef (:362 and :381; :504 and
    :465; :545 and :551-565):
        m  = fmaf(b1, m, (1 - b1) * g)                       :349
        v  = fmaf(b2, v, ((1 - b2) * g) * g)                 :350
        mh = m / bc1, vh = v / bc2                           :351-352
        u  = fmaf(wd, p, mh / (sqrtf(vh) + eps))             :353
        p  = fmaf(-lr, u, p)                                 :354
    bc1 = 1 - b1**step and bc2 = 1 - b2**step come from the host (parallel/optim.py:150). ``wd``
    overrides hp["wd"] with a per-element tensor (the segmented kernel's decay flag). emulate rounds
    where the kernel rounds: see the module docstring.
    The slips: "no_bc", "step+1", "eps_in_sqrt", "l2" (wd * p added to g, no decoupled decay),
    "decay_anyway" (wd = 0.1 where 0 was asked for), "betas" (swapped), and the two of _clip_coef."""
    R = _f32 if emulate else (lambda x: x)
    r = _r32 if emulate else float
    p, g, m, v = (st[k].double() for k in ("p", "g", "m", "v"))
    b1, b2 = (hp["b2"], hp["b1"]) if slip == "betas" else (hp["b1"], hp["b2"])
    step = hp["step"] + (1 if slip == "step+1" else 0)
    bc1, bc2 = (1.0, 1.0) if slip == "no_bc" else (1.0 - b1 ** step, 1.0 - b2 ** step)
    wdv = hp["wd"] if wd is None else wd
    if slip == "decay_anyway":
        wdv = 0.1
    wdv = R(wdv.double()) if torch.is_tensor(wdv) else r(wdv)
    lr, eps, bc1, bc2 = r(hp["lr"]), r(hp["eps"]), r(bc1), r(bc2)
    b1, b2 = r(b1), r(b2)
    omb1, omb2 = r(1.0 - b1), r(1.0 - b2)
    gm = r(r(hp["gm"]) * _clip_coef(hp, emulate, slip))
    gs = R(g * gm)
    if slip == "l2":
        gs = gs + wdv * p
        wdv = 0.0
    t1 = R(omb1 * gs)
    m1 = R(b1 * m + t1)
    v1 = R(b2 * v + R(R(omb2 * gs) * gs))
    mh, vh = R(m1 / bc1), R(v1 / bc2)
    den = torch.sqrt(vh + eps) if slip == "eps_in_sqrt" else R(R(torch.sqrt(vh)) + eps)
    u = R(wdv * p + R(mh / den))
    p1 = R(p - lr * u)
    Tm = (b1 * m).abs() + t1.abs()
    return dict(p=p1, m=m1, v=v1, Tm=Tm, Tp=p.abs() + lr * (wdv * p.abs() + mh.abs() / den), den=den, mh=mh, vh=vh,
                lr=lr, bc1=bc1)


def _adam_tol(kind, want):
    if kind == "m":
        return BOUND["adam.m"] * want["Tm"]
    if kind == "v":
        return BOUND["adam.v"] * want["v"]
    du = (BOUND["adam.m"] * want["Tm"] / (want["bc1"] * want["den"])
          + want["mh"].abs() / want["den"] ** 2 * BOUND["adam.v"] * torch.sqrt(want["vh"]) / 2)
    return BOUND["adam.p"] * want["Tp"] + want["lr"] * du


def _adam_bad(kind, got, want):
    """-> (failing elements, each element's share of its bound). got: fp32, any device."""
    assert got.dtype == torch.float32, kind
    a, b = got.detach().cpu().double(), want[kind]
    diff, tol = (a - b).abs(), _adam_tol(kind, want)
    ok = ((diff <= tol) | ((b.abs() < TINY32) & (a == 0))) & torch.isfinite(a)
    share = torch.where(diff > 0, diff / tol.clamp_min(1e-300), torch.zeros_like(diff))
    share = torch.where(ok & (tol == 0), torch.zeros_like(share), share)
    return ~ok, share


_WORST = {}


def _adam_check(got, want, label):
    """got: dict p, m, v (fp32) from a kernel; every element of each within its bound."""
    for kind in ("m", "v", "p"):
        bad, share = _adam_bad(kind, got[kind], want)
        w = float(share[~bad].max()) if bool((~bad).any()) else 0.0
        key = label.split(" ")[0]
        _WORST[(key, kind)] = max(_WORST.get((key, kind), 0.0), w)
        assert not bool(bad.any()), (label, kind, int(bad.sum()), int(bad.flatten().nonzero()[0]), float(share.max()))


def _report(key):
    print(f"{key}: worst share of a bound  " + "  ".join(f"{k} {_WORST.get((key, k), 0.0):.2f}" for k in ("m", "v", "p")))


# ---- bit patterns: the split master and RNE, by integer formulas of this file
def _bits32(x):
    return x.contiguous().view(torch.int32).long() & 0xFFFFFFFF


def _from_bits32(M):
    return (M - ((M >> 31) << 32)).to(torch.int32).view(torch.float32)


def _to16(x):
    return (x - ((x >> 15) << 16)).to(torch.int16)


def _split(p):
    """fp32 -> (hi as bf16, lo as int16): hi = (M + 0x8000) >> 16, lo = M & 0xFFFF."""
    M = _bits32(p.float())
    return _to16(((M + 0x8000) >> 16) & 0xFFFF).view(torch.bfloat16), _to16(M & 0xFFFF)


def _join(hi, lo):
    """M = ((hi - (lo >> 15)) << 16) | lo."""
    h = hi.contiguous().view(torch.int16).long() & 0xFFFF
    lw = lo.long() & 0xFFFF
    return _from_bits32((((h - (lw >> 15)) & 0xFFFF) << 16) | lw)


def _rne16(p):
    """The RNE bf16 pattern of finite fp32 values, as integers 0..65535."""
    M = _bits32(p)
    return ((M + 0x7FFF + ((M >> 16) & 1)) >> 16) & 0xFFFF


def _check_hi(hi, lo, label):
    """hi against the RNE rounding of the joined master: equal except at exact ties, where it is the
    upper half + 1 (never below RNE, one above it exactly when RNE rounds the tie down)."""
    hi, lo = hi.detach().cpu(), lo.detach().cpu()
    M = _bits32(_join(hi, lo))
    h = hi.view(torch.int16).long() & 0xFFFF
    rne = _rne16(_from_bits32(M))
    tie = (M & 0xFFFF) == 0x8000
    assert bool((h == rne)[~tie].all()), (label, "hi differs from RNE off a tie")
    up = (M >> 16) & 0xFFFF
    assert bool((h == up + 1)[tie].all()), (label, "a tie not rounded up in magnitude")
    assert bool(((h - rne)[tie] == 1 - (up[tie] & 1)).all()), label
    return int(tie.sum())


ADAM_CLASSES = 7
CLIP_MODES = {"off": (None, 0.0), "zero_max": (12345.678, 0.0), "active": (12345.678, 1.0),
              "inactive": (1.2345e-4, 1.0), "zero": (0.0, 1.0)}
PSETS = [(step, wd, gm, clip) for step in (1, 10000) for wd in (0.0, 0.1) for gm in (1.0, 0.5, -0.5) for clip in CLIP_MODES]
ADAM_SIZES = (5, 8, 8 * 256 + 3)
ADAM_BIG = 4096 * 256 * 8 + 8 * 300 + 5
ADAM_BIG_PSET = (1, 0.1, 0.5, "active")
WRAP_SIZES = (8 * 4096 + 5, 3 * 8 * 4096 + 8 * 77 + 3)
WRAP_PSETS = [(1, 0.1, -0.5, "active"), (10000, 0.0, 1.0, "off")]


def _pset_hp(pset):
    step, wd, gm, clip = pset
    s, mx = CLIP_MODES[clip]
    return _hp(step=step, wd=wd, gm=gm, sumsq=s, max_norm=mx)


@functools.lru_cache(maxsize=None)
def _adam_case(n, bf16, pset):
    """p, m, v fp32 and g (bf16 or fp32) of n elements, and each element's class: module docstring."""
    hp = _pset_hp(pset)
    gen = _gen(21, n, bf16, PSETS.index(pset))
    gm = hp["gm"] * _clip_coef(hp)
    i = torch.arange(n)
    cls = i % ADAM_CLASSES
    e = (-40 + (i * 7) % 61).double()
    rnd = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    sgn = lambda: 1.0 - 2.0 * (rnd() < 0.5).double()
    g = sgn() * (1.0 + rnd()) * 2.0 ** e
    g = torch.where((cls == 1) | (cls == 2), torch.zeros_like(g), g)
    g = g.bfloat16() if bf16 else g.float()
    gs = g.double() * gm
    m = gs * 0.5 * torch.randn(n, generator=gen, dtype=torch.float64)
    v = gs * gs * (0.5 + rnd())
    old = 2.0 ** e
    m = torch.where(cls == 2, old * sgn() * (0.5 + rnd()), m)
    v = torch.where(cls == 2, old * old * (0.5 + rnd()), v)
    m = torch.where(cls == 3, -(1.0 - B1) / B1 * gs * (1.0 + 2.0 ** -12), m)
    m = torch.where(cls == 5, -gs * (0.25 + rnd()), m)
    zero = (cls == 1) | (cls == 6)
    m = torch.where(zero, torch.zeros_like(m), m)
    v = torch.where(zero, torch.zeros_like(v), v)
    k = (i // ADAM_CLASSES) % 8
    p = sgn() * (1.0 + rnd()) * 2.0 ** (k.double() - 6.0)
    zeros = torch.zeros_like(p)
    p = torch.where(cls == 4, torch.where(k % 2 == 0, zeros, -zeros), p)
    return dict(p=p.float(), g=g, m=m.float(), v=v.float(), cls=cls, gs=gs)


def _big_sel():
    """The scored elements of ADAM_BIG: every 1021st, the first and last vector of each trip, the tail."""
    n, trip = ADAM_BIG, 4096 * 256 * 8
    sp = list(range(0, 16)) + list(range(trip - 16, trip + 16)) + list(range(n - 5 - 16, n))
    return torch.unique(torch.cat([torch.arange(0, n, 1021), torch.tensor(sp)]))


def _sub(st, sel):
    return {k: (t[sel] if torch.is_tensor(t) else t) for k, t in st.items()}


# ===================================================================== 4. the segmented kernel
SEG_LR, SEG_WD, SEG_CLIP, SEG_SCALE, SEG_SUMSQ, SEG_STEPS = 1e-2, 0.1, 0.5, 0.5, 400.0, 3


def _seg_net():
    """Registration order is the reverse of the layout: [256 x 256], [384 x 128], the 131 x 37 fused
    weight (1-D tiles between two matrices), [128 x 384], the plain 37 x 129 weight, then the no-decay
    vectors; the last 1-D range holds the decay boundary."""
    from ray_community_amd.parallel.fused_linear import FusedWgradLinear

    nn = torch.nn
    return nn.ModuleList([nn.Linear(129, 37), nn.LayerNorm(37), FusedWgradLinear(384, 128), FusedWgradLinear(37, 131),
                          FusedWgradLinear(128, 384), nn.LayerNorm(384), FusedWgradLinear(256, 256)])


def _seg_layout(net, flat, wd):
    """Per element: the decay of its parameter by default_no_decay on the named parameters (0 on
    padding), and whether it belongs to a parameter at all."""
    from ray_community_amd.parallel.flat import default_no_decay

    wdv = torch.zeros(flat.numel, dtype=torch.float64)
    used = torch.zeros(flat.numel, dtype=torch.bool)
    for name, p in net.named_parameters():
        off = flat.param_offset[id(p)]
        wdv[off: off + p.numel()] = 0.0 if default_no_decay(name, p) else wd
        used[off: off + p.numel()] = True
    return wdv, used


@functools.lru_cache(maxsize=None)
def _seg_data():
    """The layout of _seg_net on the CPU, bf16 start weights and the bf16 gradients of each step
    (zero on padding, as the backward leaves it)."""
    from ray_community_amd.parallel.flat import FlatParameters

    net = _seg_net().to(torch.bfloat16)
    flat = FlatParameters(net)
    wdv, used = _seg_layout(net, flat, SEG_WD)
    gen = _gen(41, flat.numel)
    w0 = (0.05 * torch.randn(flat.numel, generator=gen) * used).bfloat16()
    grads = [(2.0 ** -3 * torch.randn(flat.numel, generator=gen) * used).bfloat16() for _ in range(SEG_STEPS)]
    return dict(numel=flat.numel, decay_end=flat.decay_end, wdv=wdv, used=used, w0=w0, grads=grads)


def _seg_hp(step):
    return _hp(step=step, wd=SEG_WD, gm=SEG_SCALE, sumsq=SEG_SUMSQ, max_norm=SEG_CLIP, lr=SEG_LR)


def _seg_cpu_trajectory():
    """(inputs, step) of each step, the state advanced by the emulating oracle: the floors' cases."""
    d = _seg_data()
    st = dict(p=d["w0"].float(), m=torch.zeros(d["numel"]), v=torch.zeros(d["numel"]))
    out = []
    for s in range(SEG_STEPS):
        st = dict(st, g=d["grads"][s])
        out.append((st, s + 1))
        em = _adam_oracle(st, _seg_hp(s + 1), emulate=True, wd=d["wdv"])
        st = dict(p=em["p"].float(), m=em["m"].float(), v=em["v"].float())
    return out


# the direct call: rows (off, n, first tile, matrix?, R, C, decay) within the documented contract
# (offsets multiples of 8, R and C multiples of 128); FlatParameters cannot produce a matrix without
# decay, two adjacent matrices after a ragged 1-D range, or a 1-D length that is no multiple of 8
DIRECT_ROWS = [(0, 4096 + 8 * 3 + 5, 0, 0, 0, 0, 1), (4128, 128 * 256, 2, 1, 128, 256, 0),
               (4128 + 32768, 256 * 128, 4, 1, 256, 128, 1), (69664, 13, 6, 0, 0, 0, 0)]
DIRECT_TILES, DIRECT_LEN = 7, 69664 + 16
DIRECT_PSET = (1, 0.1, 0.5, "active")


@functools.lru_cache(maxsize=None)
def _direct_case():
    return _adam_case(DIRECT_LEN, True, DIRECT_PSET)


def _seg_model(rows, st, hp, emulate=False, slip=None):
    """A CPU model of adamw_split_seg_kernel over a table: (p, m, v in fp64, covered mask, the W^T of
    each matrix row as bf16). Elements outside every segment keep their inputs. The slips: "shift"
    (tile = b - first + 1: the first tile of every segment is never visited, nor its part of W^T),
    "swap" (two 8-row groups of each W^T exchanged), "decay" (the flag ignored: wd everywhere)."""
    n = st["p"].numel()
    wdv = torch.zeros(n, dtype=torch.float64)
    cov, upd = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    for off, cnt, _, mat, R, C, decay in rows:
        wdv[off: off + cnt] = hp["wd"] if (decay or slip == "decay") else 0.0
        cov[off: off + cnt] = True
        seg = torch.ones(cnt, dtype=torch.bool)
        if slip == "shift":
            if mat:
                seg.view(R, C)[:128, :128] = False
            else:
                seg[:4096] = False
        upd[off: off + cnt] = seg
    o = _adam_oracle(st, hp, emulate=emulate, wd=wdv)
    res = {k: torch.where(upd, o[k], st[k].double()) for k in ("p", "m", "v")}
    wts = []
    for off, cnt, _, mat, R, C, _ in rows:
        if not mat:
            continue
        hi = _split(res["p"][off: off + cnt].float())[0].view(R, C)
        wt = hi.t().contiguous()
        if slip == "shift":
            wt[:128, :128] = 0
        if slip == "swap":
            wt[0:8], wt[8:16] = wt[8:16].clone(), wt[0:8].clone()
        wts.append(wt)
    return res, cov, wts, o


def _seg_check(got, got_wts, rows, st, hp, label):
    """Kernel results over a table against the exact model: covered elements within the bounds of
    section 2, uncovered ones bit-unchanged, hi the rounding of the master, W^T == W.t()."""
    _, cov, _, want = _seg_model(rows, st, hp)
    _adam_check({k: got[k][cov] for k in ("p", "m", "v")}, _sub(want, cov), label)
    for k in ("p", "m", "v"):
        assert torch.equal(got[k][~cov], st[k][~cov]), (label, k, "an element outside every segment changed")
    mats = [r for r in rows if r[3]]
    assert len(got_wts) == len(mats)
    for (off, cnt, _, _, R, C, _), wt in zip(mats, got_wts):
        assert torch.equal(wt, got["hi"][off: off + cnt].view(R, C).t()), (label, "W^T", off)


def _as_kernel(res, wts):
    """A model's outputs stored as the kernel stores them."""
    p = res["p"].float()
    return dict(p=p, m=res["m"].float(), v=res["v"].float(), hi=_split(p)[0]), wts


# ======================================================================== CPU tests: the bounds
def _floor_cases():
    for n in ADAM_SIZES:
        for bf16 in (True, False):
            for pset in PSETS:
                yield _adam_case(n, bf16, pset), _pset_hp(pset), None
    sel = _big_sel()
    for bf16 in (True, False):
        yield _sub(_adam_case(ADAM_BIG, bf16, ADAM_BIG_PSET), sel), _pset_hp(ADAM_BIG_PSET), None
    for n in WRAP_SIZES:
        for bf16 in (True, False):
            for pset in WRAP_PSETS:
                yield _adam_case(n, bf16, pset), _pset_hp(pset), None
    d = _seg_data()
    for st, step in _seg_cpu_trajectory():
        yield st, _seg_hp(step), d["wdv"]
    wdv = torch.zeros(DIRECT_LEN, dtype=torch.float64)
    for off, cnt, _, _, _, _, decay in DIRECT_ROWS:
        wdv[off: off + cnt] = 0.1 * decay
    yield _direct_case(), _pset_hp(DIRECT_PSET), wdv


def _floors(kinds):
    f = dict.fromkeys(kinds, 0.0)
    for st, hp, wdv in _floor_cases():
        ex, em = _adam_oracle(st, hp, wd=wdv), _adam_oracle(st, hp, emulate=True, wd=wdv)
        for kind in kinds:
            diff = (em[kind[5:]] - ex[kind[5:]]).abs()
            if kind == "adam.m":
                unit = ex["Tm"]
            elif kind == "adam.v":
                unit = ex["v"]
            else:  # what m's and v's bounds leave over
                diff = (diff - (_adam_tol("p", ex) - BOUND["adam.p"] * ex["Tp"])).clamp_min(0)
                unit = ex["Tp"]
            assert bool((diff[unit == 0] == 0).all()), kind
            f[kind] = max(f[kind], float((diff / unit.clamp_min(1e-300))[unit > 0].max()))
    return f


def test_bounds_are_twice_the_measured_floors():
    """The reference for BOUND: m and v first, then p with their bounds inside its inherited term."""
    f = _floors(("adam.m", "adam.v"))
    f.update(_floors(("adam.p",)))
    for kind in BOUND:
        print(f"    {kind:<10} {f[kind]:.2e}   2**{math.log2(BOUND[kind]):.0f} = {BOUND[kind]:.2e}")
    for kind in BOUND:
        assert 0 < f[kind] <= BOUND[kind] / 2, (kind, f[kind])
        assert BOUND[kind] == 2.0 ** math.ceil(math.log2(2 * f[kind])), (kind, f[kind])


def test_adam_data_holds_every_class():
    """Every class at every position of an 8-element group; |g| over 2**-40 .. 2**20; |p| over eight
    binades and both zeros; the tuned elements cancel to 2**-12 of their terms; eps decides some
    elements (sqrt(vh) < eps) and not others."""
    st = _adam_case(ADAM_SIZES[-1], False, PSETS[0])
    assert {(c, i % 8) for i, c in enumerate(st["cls"].tolist())} == {
        (c, j) for c in range(ADAM_CLASSES) for j in range(8)}
    live = st["g"] != 0
    ex = torch.floor(torch.log2(st["g"][live].double().abs()))
    assert ex.min() == -40 and ex.max() == 20
    pz = st["p"][st["cls"] == 4]
    assert bool((pz == 0).all()) and bool(torch.signbit(pz).any()) and not bool(torch.signbit(pz).all())
    pe = torch.floor(torch.log2(st["p"][st["cls"] != 4].double().abs()))
    assert set(pe.tolist()) == set(range(-6, 2)) and bool((st["p"] < 0).any()) and bool((st["p"] > 0).any())
    want = _adam_oracle(st, _pset_hp(PSETS[0]))
    c3 = st["cls"] == 3
    assert bool((want["m"].abs()[c3] < 2.0 ** -11 * want["Tm"][c3]).all()) and bool((want["m"][c3] != 0).all())
    small = torch.sqrt(want["vh"])[live] < EPS_ADAM
    assert small.any() and (~small).any()


# ================================================================ CPU tests: the checkers reject slips
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_sumsq_checker_rejects_a_dropped_vector_tail_element_and_trip(bf16):
    """At every size where the path exists: each structural vector, each tail element, and the whole
    second grid trip carry a non-zero square, so an exact comparison sees their loss."""
    vec = _ss_vec(bf16)
    for n in _ss_sizes(bf16):
        buf, pad, want = _ss_case(n, bf16, 1 + n % 3)
        x = buf[pad: pad + n].float()
        assert _ss_ref(x, bf16) == want
        _ss_check(torch.tensor([float(want)]), want, "intact")
        nv, stride = _ss_grid(n, bf16)
        slips = [("vector", k) for k in sorted({i // vec for i in _ss_struct(n, bf16) if i // vec < nv})]
        slips += [("tail", j) for j in range(nv * vec, n)]
        if nv > stride:
            slips.append(("trip2",))
        assert slips
        for slip in slips:
            bad = _ss_ref(x, bf16, slip)
            assert bad != want, (n, slip)
        for slip in (slips[0], slips[-1]):
            with pytest.raises(AssertionError):
                _ss_check(torch.tensor([float(_ss_ref(x, bf16, slip))]), want, str(slip))
    big = _ss_sizes(bf16)[-1]
    nv, stride = _ss_grid(big, bf16)
    assert nv > 4 * stride and big % vec == vec - 1
    if bf16:  # the hand-off sizes sit on both sides of the first lane entering the four-deep loop
        assert [_ss_grid(n, True)[0] - 3 * SS_STRIDE for n in _ss_sizes(True)[-4:-1]] == [0, 1, 2]


def _stored(o):
    return {k: o[k].float() for k in ("p", "m", "v")}


def _rejected(bad_out, want):
    return _adam_bad("m", bad_out["m"], want)[0] | _adam_bad("v", bad_out["v"], want)[0] | _adam_bad("p", bad_out["p"], want)[0]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_checker_rejects_every_slip(n, bf16):
    """Each slipped oracle, stored as the kernel stores it, is rejected on the elements built for it:
    the fresh-state class (m = v = 0, p != 0), within the window of |g'| where the slip changes the
    update at all. The emulating oracle itself passes everywhere."""
    seen = dict.fromkeys(("no_bc", "step+1", "eps_in_sqrt", "l2", "decay_anyway", "betas", "clip_no_mul", "clip_no_fabs",
                          "group", "tail"), 0)
    for pset in PSETS:
        step, wd, gm, clip = pset
        st, hp = _adam_case(n, bf16, pset), _pset_hp(pset)
        want = _adam_oracle(st, hp)
        _adam_check(_stored(_adam_oracle(st, hp, emulate=True)), want, "intact")
        fresh, a = st["cls"] == 6, st["gs"].abs()
        slips = {"betas": fresh}
        if step == 1:  # at step 10000 both corrections are 1
            slips["no_bc"] = slips["step+1"] = fresh & (a > 2.0 ** -20)
        slips["eps_in_sqrt"] = fresh & (a > 2.0 ** -30) & (a < 2.0 ** -16)
        if wd:
            slips["l2"] = fresh & (a <= 2.0 ** -4)
        else:
            slips["decay_anyway"] = fresh
        if clip == "active" and abs(gm) != 1.0:
            slips["clip_no_mul"] = fresh
        if clip in ("active", "inactive") and gm < 0:
            slips["clip_no_fabs"] = fresh
        for slip, felt in slips.items():
            rej = _rejected(_stored(_adam_oracle(st, hp, slip=slip)), want)
            assert bool(rej[felt].all()), (pset, slip)
            seen[slip] += int(felt.sum())
        # an 8-element group, or the tail, that was never updated: the fresh elements and the ones
        # with g = 0 and old state (m must shrink by b1) show it
        shows = fresh | (st["cls"] == 2)
        good = _stored(_adam_oracle(st, hp, emulate=True))
        nv = n // 8
        for name, lo, hi in [("group", 8 * k, 8 * k + 8) for k in sorted({0, nv // 2, nv - 1}) if k >= 0 and nv] + (
                [("tail", nv * 8, n)] if n % 8 else []):
            bad = {k: good[k].clone() for k in good}
            for k in bad:
                bad[k][lo:hi] = st[k][lo:hi]
            felt = torch.zeros(n, dtype=torch.bool)
            felt[lo:hi] = shows[lo:hi]
            assert felt.any(), (n, name, lo)
            rej = _rejected(bad, want)
            assert bool(rej[felt].all()) and not bool(rej[:lo].any()) and not bool(rej[hi:].any()), (pset, name, lo)
            seen[name] += int(felt.sum())
            with pytest.raises(AssertionError):
                _adam_check(bad, want, name)
    for slip, cnt in seen.items():
        if (slip == "tail" and n % 8 == 0) or (slip == "group" and n < 8):
            continue
        if n >= 2048:
            assert cnt > 0, slip
    if n >= 2048:
        assert seen["eps_in_sqrt"] > 100


def test_seg_checker_rejects_a_shifted_table_swapped_rows_and_an_ignored_flag():
    st, hp = _direct_case(), _pset_hp(DIRECT_PSET)
    res, cov, wts, _ = _seg_model(DIRECT_ROWS, st, hp, emulate=True)
    assert int((~cov).sum()) == 3 + 3  # the gaps the table leaves: 4125..4127 and the last 3 words
    _seg_check(*_as_kernel(res, wts), DIRECT_ROWS, st, hp, "intact")
    for slip in ("shift", "swap", "decay"):
        res, _, wts, _ = _seg_model(DIRECT_ROWS, st, hp, emulate=True, slip=slip)
        with pytest.raises(AssertionError):
            _seg_check(*_as_kernel(res, wts), DIRECT_ROWS, st, hp, slip)
    # the ignored flag is seen by every fresh element of the two segments without decay
    want = _seg_model(DIRECT_ROWS, st, hp)[3]
    bad = _stored(_seg_model(DIRECT_ROWS, st, hp, emulate=True, slip="decay")[0])
    nod = torch.zeros(DIRECT_LEN, dtype=torch.bool)
    for off, cnt, _, _, _, _, decay in DIRECT_ROWS:
        nod[off: off + cnt] = not decay
    felt = nod & (st["cls"] == 6)
    assert felt.sum() > 1000 and bool(_rejected(bad, want)[felt].all())
    # a shifted table: every fresh element of each segment's first tile
    bad = _stored(_seg_model(DIRECT_ROWS, st, hp, emulate=True, slip="shift")[0])
    first = torch.zeros(DIRECT_LEN, dtype=torch.bool)
    first[:4096] = True
    first[69664: 69664 + 13] = True
    for off, cnt, _, mat, R, C, _ in DIRECT_ROWS:
        if mat:
            first[off: off + cnt].view(R, C)[:128, :128] = True
    rej = _rejected(bad, want)
    assert bool(rej[first & (st["cls"] == 6)].all()) and not bool(rej[cov & ~first].any())


# ===================================================================== 3. the split format, exhaustively
SPLIT_LOS = (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
SPLIT_TAIL = (0x00008000, 0x80008000, 0x007F8000, 0x3F7FFFFF, 0xBF7F8000)  # the 5 elements of the scalar tail


@functools.lru_cache(maxsize=None)
def _split_table():
    """The intended fp32 patterns M = upper << 16 | lo: every upper half with a finite exponent (NaN
    and inf patterns replaced by 0) x SPLIT_LOS; a pair whose carry would leave the finite range
    (upper 0x7F7F or 0xFF7F with lo >= 0x8000: hi would be an inf pattern) is replaced by 0. Every
    finite hi arises, as upper or as upper + 1. Returns M (int64), hi (bf16), lo (int16)."""
    up = torch.arange(65536)
    up = torch.where((up & 0x7F80) == 0x7F80, torch.zeros_like(up), up)
    lo = torch.tensor(SPLIT_LOS)
    M = ((up[:, None] << 16) | lo[None, :]).flatten()
    carry_out = ((M >> 16) & 0x7FFF) == 0x7F7F
    M = torch.where(carry_out & ((M & 0xFFFF) >= 0x8000), torch.zeros_like(M), M)
    M = torch.cat([M, torch.tensor(SPLIT_TAIL)])
    hi = ((M + 0x8000) >> 16) & 0xFFFF
    assert bool(((hi & 0x7F80) != 0x7F80).all()) and set(hi.tolist()) == set(up.tolist())
    return M, _to16(hi).view(torch.bfloat16), _to16(M & 0xFFFF)


def test_split_join_table_on_the_cpu():
    """ops.reference.split_master / join_master over the table: the carry at lo >= 0x8000, across an
    exponent boundary, out of the denormals, +-0, negative weights; and this file's own formulas."""
    M, hi, lo = _split_table()
    p = _from_bits32(M)
    assert M.numel() == 65536 * len(SPLIT_LOS) + len(SPLIT_TAIL) and M.numel() % 8 == 5
    h2, l2 = reference.split_master(p)
    assert torch.equal(h2.view(torch.int16), hi.view(torch.int16)) and torch.equal(l2, lo)
    assert torch.equal(_bits32(reference.join_master(hi, lo)), M)
    h3, l3 = _split(p)
    assert torch.equal(h3.view(torch.int16), hi.view(torch.int16)) and torch.equal(l3, lo)
    assert torch.equal(_bits32(_join(hi, lo)), M)
    ties = _check_hi(hi, lo, "table")
    assert ties >= 65000
    # the named patterns are there
    pats = set(M.tolist())
    assert {0x00000000, 0x80000000, 0x00008000, 0x007F8000, 0x3F7F8000, 0xBF7FFFFF, 0x80008001} <= pats
    # torch's own rounding agrees with _rne16 off the denormals torch may flush
    norm = (M & 0x7F800000) != 0
    assert torch.equal((p.bfloat16().view(torch.int16).long() & 0xFFFF)[norm], _rne16(p)[norm])


# ========================================================================================= GPU tests
def _lib_call(name, *args):
    from ray_community_amd.ops._lib import check, stream_ptr

    check(getattr(ops.lib(), name)(*args, stream_ptr(torch.device("cuda"))), name)


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_sumsq_exact(bf16):
    """Every size of _ss_sizes as a view at a multiple of 64 elements: ops.grad_sumsq, and rca_sumsq on
    a workspace of its own, overwriting and accumulating onto 5.0."""
    ws = torch.zeros(ops.SUMSQ_WS, device="cuda")
    outs = []
    for n in _ss_sizes(bf16):
        buf, pad, want = _ss_case(n, bf16, 1 + n % 3)
        view = buf.cuda()[pad: pad + n]
        assert view.data_ptr() % 128 == 0 and view.numel() == n
        out = torch.full((2,), 5.0, device="cuda")
        _lib_call("rca_sumsq", view.data_ptr(), n, 0 if bf16 else 1, ws.data_ptr(), out[:1].data_ptr(), 0)
        _lib_call("rca_sumsq", view.data_ptr(), n, 0 if bf16 else 1, ws.data_ptr(), out[1:].data_ptr(), 1)
        outs.append((n, want, ops.grad_sumsq([view]), out))
    torch.cuda.synchronize()
    for n, want, got, out in outs:
        _ss_check(got.cpu(), want, f"grad_sumsq n={n}")
        assert out.cpu().tolist() == [want, want + 5], (n, out.cpu().tolist(), want)
    assert int(ws[1024:1025].view(torch.int32).item()) == 0


@gpu
def test_sumsq_accumulate_chain_of_mixed_dtypes():
    """A list of bf16 and fp32 tensors with empty ones inside and in front: exact, the same with the
    empty ones taken out, a preset ``out`` overwritten, the ticket word zero afterwards and a second
    call bit-identical."""
    xs, want = [], 0
    for j, (bf16, n) in enumerate(SS_CHAIN):
        buf, pad, w = _ss_case(n, bf16, 1 + j % 4)
        xs.append(buf.cuda()[pad: pad + n])
        want += w
    assert want < 2 ** 24 and sum(x.numel() == 0 for x in xs) == 2
    first = ops.grad_sumsq(xs).clone()
    _ss_check(first.cpu(), want, "chain")
    _ss_check(ops.grad_sumsq([x for x in xs if x.numel()]).cpu(), want, "chain without the empty tensors")
    out = torch.full((1,), 777.0, device="cuda")
    _ss_check(ops.grad_sumsq([xs[1]] + xs, out=out).cpu(), want, "chain behind an empty tensor, preset out")
    _ss_check(ops.grad_sumsq([xs[1]]).cpu(), 0, "an empty tensor alone")
    again = ops.grad_sumsq(xs)
    assert torch.equal(again.view(torch.int32), first.view(torch.int32))
    ws = ops._workspace(xs[0].device, "sumsq", ops.SUMSQ_WS)
    torch.cuda.synchronize()
    assert int(ws[1024:1025].view(torch.int32).item()) == 0


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_sumsq_one_hot_probes(bf16):
    """A zero tensor of the largest size with one 3.0 at each structural index, one index per launch:
    exactly 9.0 every time (a dropped and a doubled element cannot cancel)."""
    n = _ss_sizes(bf16)[-1]
    idx = _ss_struct(n, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    buf = torch.full((64 + n + 64,), 2.0, dtype=dt, device="cuda")
    view = buf[64: 64 + n]
    view.zero_()
    outs = torch.full((len(idx),), -1.0, device="cuda")
    for k, i in enumerate(idx):
        view[i] = 3.0
        ops.grad_sumsq([view], out=outs[k: k + 1])
        view[i] = 0.0
    got = outs.cpu()
    wrong = [(idx[k], float(got[k])) for k in range(len(idx)) if float(got[k]) != 9.0]
    assert not wrong, wrong[:8]
    assert len(idx) > 30 and n - 1 in idx and 0 in idx


def _padded(t, fill=1.0):
    """t on the device as a view at 64 elements into a buffer of sentinels -> (buffer, view)."""
    n = t.numel()
    buf = torch.full((n + 128,), fill, dtype=torch.float32).to(t.dtype).cuda()
    buf[64: 64 + n] = t.cuda()
    return buf, buf[64: 64 + n]


def _sentinels_intact(bufs, n, label):
    for name, b in bufs.items():
        s = torch.cat([b[:64], b[64 + n:]]).float().cpu()
        assert bool((s == 1.0).all()), (label, name, "written outside its range")


def _adam_launch(fmt, st, hp):
    """One update through parallel.optim.adamw_update_ -> dict p, m, v (fp32, device) and w / hi / lo.
    A sumsq pointer together with max_norm = 0 is the one combination adamw_update_ cannot express
    (it passes the pointer only when clipping): that case calls rca_adamw / rca_adamw_split itself."""
    from ray_community_amd.ops._lib import stream_ptr
    from ray_community_amd.parallel.optim import AdamWStep, adamw_update_

    n = st["g"].numel()
    bufs, views = {}, {}
    src = dict(g=st["g"], m=st["m"], v=st["v"])
    if fmt == "split":
        src["hi"], src["lo"] = _split(st["p"])
    else:
        src["p"] = st["p"]
        if fmt == "master":
            src["w"] = torch.full((n,), 7.0, dtype=torch.bfloat16)
    for k, t in src.items():
        bufs[k], views[k] = _padded(t)
    sumsq = torch.tensor([hp["sumsq"] if hp["sumsq"] is not None else 1e30], device="cuda")
    step = AdamWStep(hp["lr"], hp["b1"], hp["b2"], hp["eps"], 1.0 - hp["b1"] ** hp["step"], 1.0 - hp["b2"] ** hp["step"],
                     hp["step"], hp["gm"], hp["max_norm"] if hp["sumsq"] is not None else 0.0, sumsq, 1.0)
    g, m, v = views["g"], views["m"], views["v"]
    if hp["sumsq"] is not None and hp["max_norm"] == 0.0:
        rest = (g.data_ptr(), 0 if g.dtype == torch.bfloat16 else 1, m.data_ptr(), v.data_ptr(), n, step.lr, step.b1, step.b2,
                step.eps, hp["wd"], step.bc1, step.bc2, step.grad_scale, sumsq.data_ptr(), 0.0, stream_ptr(g.device))
        if fmt == "split":
            rc = ops.lib().rca_adamw_split(views["hi"].data_ptr(), views["lo"].data_ptr(), *rest)
        else:
            rc = ops.lib().rca_adamw(views["p"].data_ptr(), views["w"].data_ptr() if fmt == "master" else 0, *rest)
        assert rc == 0
    elif fmt == "split":
        adamw_update_(views["hi"], g, m, v, step, hp["wd"], lo=views["lo"])
    elif fmt == "master":
        adamw_update_(views["w"], g, m, v, step, hp["wd"], master=views["p"])
    else:
        adamw_update_(views["p"], g, m, v, step, hp["wd"])
    return bufs, views


def _adam_collect(fmt, bufs, views, st, label):
    """After the launch: sentinels, the gradient unchanged, the model-weight copy; -> p, m, v on the CPU."""
    n = st["g"].numel()
    _sentinels_intact(bufs, n, label)
    assert torch.equal(views["g"].cpu(), st["g"]), (label, "the gradient changed")
    if fmt == "split":
        hi, lo = views["hi"].cpu(), views["lo"].cpu()
        _check_hi(hi, lo, label)
        p = _join(hi, lo)
    else:
        p = views["p"].cpu()
        if fmt == "master":
            assert torch.equal(views["w"].cpu().view(torch.int16), p.bfloat16().view(torch.int16)), (label, "bf16 copy")
    return dict(p=p, m=views["m"].cpu(), v=views["v"].cpu())


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["g_bf16", "g_fp32"])
@pytest.mark.parametrize("fmt", ["fp32", "master", "split"])
def test_adamw_elements(fmt, bf16):
    """Every parameter set at the small sizes, each format and gradient dtype: one update per element
    against the fp64 oracle."""
    key = f"adamw[{fmt},{'bf16' if bf16 else 'fp32'}]"
    runs = []
    for n in ADAM_SIZES:
        for pset in PSETS:
            st, hp = _adam_case(n, bf16, pset), _pset_hp(pset)
            runs.append((n, pset, st, hp) + _adam_launch(fmt, st, hp))
    torch.cuda.synchronize()
    for n, pset, st, hp, bufs, views in runs:
        label = f"{key} n={n} {pset}"
        _adam_check(_adam_collect(fmt, bufs, views, st, label), _adam_oracle(st, hp), label)
    _report(key)


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["g_bf16", "g_fp32"])
def test_adamw_over_the_flat_grid_cap(bf16):
    """4096 x 256 x 8 + 8 x 300 + 5 elements with an fp32 master and a bf16 copy: 300 lanes take a
    second trip and 5 elements the scalar tail. Scored on _big_sel(); the bf16 copy, the sentinels
    and "m or v changed" on every element."""
    key = f"adamw-big[{'bf16' if bf16 else 'fp32'}]"
    st, hp = _adam_case(ADAM_BIG, bf16, ADAM_BIG_PSET), _pset_hp(ADAM_BIG_PSET)
    assert ADAM_BIG // 8 > 4096 * 256 and ADAM_BIG % 8 == 5
    bufs, views = _adam_launch("master", st, hp)
    torch.cuda.synchronize()
    _sentinels_intact(bufs, ADAM_BIG, key)
    assert torch.equal(views["w"], views["p"].bfloat16())
    sel = _big_sel()
    dsel = sel.cuda()
    got = {k: views[k][dsel].cpu() for k in ("p", "m", "v")}
    _adam_check(got, _adam_oracle(_sub(st, sel), hp), key)
    # no element outside the scored set was left alone: a live element's m or v moves (m alone can sit
    # on a fixed point of its EMA by coincidence: one generic element of this case does)
    live = (st["cls"] != 1).cuda()
    assert bool(((views["m"] != st["m"].cuda()) | (views["v"] != st["v"].cuda()))[live].all())
    assert bool((views["m"] == 0)[~live].all())
    _report(key)


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["g_bf16", "g_fp32"])
@pytest.mark.parametrize("n", WRAP_SIZES)
def test_adamw_split_under_a_wrapped_grid(n, bf16):
    """rca_adamw_split_set_blocks 1, 3 and 7: up to 16 grid-stride trips at a small n, bit-identical
    to the default grid and within the bounds."""
    key = f"adamw-wrap[{n},{'bf16' if bf16 else 'fp32'}]"
    L = ops.lib()
    for pset in WRAP_PSETS:
        st, hp = _adam_case(n, bf16, pset), _pset_hp(pset)
        res = {}
        try:
            for nb in (4096, 1, 3, 7):
                L.rca_adamw_split_set_blocks(nb)
                bufs, views = _adam_launch("split", st, hp)
                torch.cuda.synchronize()
                res[nb] = (_adam_collect("split", bufs, views, st, f"{key} blocks={nb}"), views["hi"].cpu(), views["lo"].cpu())
        finally:
            L.rca_adamw_split_set_blocks(4096)
        _adam_check(res[4096][0], _adam_oracle(st, hp), f"{key} {pset}")
        for nb in (1, 3, 7):
            for k in ("p", "m", "v"):
                assert torch.equal(res[nb][0][k].view(torch.int32), res[4096][0][k].view(torch.int32)), (key, nb, k)
            assert torch.equal(res[nb][1].view(torch.int16), res[4096][1].view(torch.int16)), (key, nb, "hi")
            assert torch.equal(res[nb][2], res[4096][2]), (key, nb, "lo")
    _report(key)


@gpu
@pytest.mark.parametrize("path", ["flat", "segment"])
def test_split_master_identity_step_over_every_pattern(path):
    """lr = 0, wd = 0, g = 0, m = v = 0 leaves p bit-unchanged (fmaf(-0, u, p) == p): every (hi, lo)
    of the table comes back as it went in, through rca_adamw_split and through a 1-D segment of
    rca_adamw_split_seg, and joins to the intended pattern -- denormals and both zeros included."""
    M, hi, lo = _split_table()
    n = M.numel()
    src = dict(hi=hi, lo=lo, g=torch.zeros(n, dtype=torch.bfloat16), m=torch.zeros(n), v=torch.zeros(n))
    bufs, views = {}, {}
    for k, t in src.items():
        bufs[k], views[k] = _padded(t)
    ptrs = [views[k].data_ptr() for k in ("hi", "lo", "g")] + [0, views["m"].data_ptr(), views["v"].data_ptr()]
    hps = (0.0, B1, B2, EPS_ADAM, 0.0, 0.1, 0.05, 1.0, 0, 0.0)
    if path == "flat":
        _lib_call("rca_adamw_split", *ptrs, n, *hps)
    else:
        segs = torch.tensor([[0, n, 0, 0, 0, 0, 1, 0]], dtype=torch.int64, device="cuda")
        _lib_call("rca_adamw_split_seg", *ptrs, segs.data_ptr(), 1, (n + 4095) // 4096, *hps)
    torch.cuda.synchronize()
    _sentinels_intact(bufs, n, path)
    got_hi, got_lo = views["hi"].cpu(), views["lo"].cpu()
    dh = (got_hi.view(torch.int16) != hi.view(torch.int16)).nonzero().flatten()
    dl = (got_lo != lo).nonzero().flatten()
    assert dh.numel() == 0 and dl.numel() == 0, (path, [hex(int(M[i])) for i in torch.cat([dh, dl])[:8]])
    assert torch.equal(_bits32(_join(got_hi, got_lo)), M)
    assert bool((views["m"] == 0).all()) and bool((views["v"] == 0).all())


def _seg_run(blocks):
    """Three FlatAdamW steps of _seg_net under one grid setting -> per step (hi, lo, m, v, [W^T ...])
    on the CPU. Start weights, gradients and the sumsq word are the test's own."""
    from ray_community_amd.parallel import FlatAdamW
    from ray_community_amd.parallel.flat import FlatParameters

    d = _seg_data()
    net = _seg_net().to(device="cuda", dtype=torch.bfloat16)
    flat = FlatParameters(net)
    assert flat.numel == d["numel"] and flat.decay_end == d["decay_end"]
    flat.data.copy_(d["w0"].cuda())
    opt = FlatAdamW(flat, lr=SEG_LR, weight_decay=SEG_WD, max_grad_norm=SEG_CLIP)
    assert opt.split_master and opt.transposed_weights
    L = ops.lib()
    steps = []
    try:
        L.rca_adamw_split_set_blocks(blocks)
        for s in range(SEG_STEPS):
            flat.grad.copy_(d["grads"][s].cuda())
            for p in flat.fused:  # the fused backward wrote these gradients
                p._rca_grad_fresh = False
            flat.precomputed_sumsq = torch.tensor([SEG_SUMSQ], device="cuda")
            opt.step(SEG_SCALE)
            torch.cuda.synchronize()
            mats = [p for p in net.parameters() if getattr(p, "_rca_wt", None) is not None]
            assert sorted(tuple(p.shape) for p in mats) == [(128, 384), (256, 256), (384, 128)]
            for p in mats:
                assert torch.equal(p._rca_wt, p.detach().t()), (blocks, s, tuple(p.shape))
            steps.append((flat.data.cpu().clone(), opt.lo.cpu().clone(), opt.m.cpu().clone(), opt.v.cpu().clone()))
    finally:
        L.rca_adamw_split_set_blocks(4096)
    if blocks == 4096:  # the table _setup_transposed built: what the layout was chosen for
        rows = opt._segs.cpu().tolist()
        kinds = [bool(r[3]) for r in rows]
        assert kinds == [True, True, False, True, False, False], rows
        assert [r[6] for r in rows] == [1, 1, 1, 1, 1, 0] and rows[4][0] + rows[4][1] == flat.decay_end == rows[5][0]
        assert all(r[1] > 4096 and r[1] % 4096 for r in (rows[2], rows[4])) and rows[5][1] % 4096
        assert opt._seg_blocks == 4 + 3 + 2 + 3 + 2 + 1
    return steps


@gpu
def test_adamw_segmented_under_wrapped_grids_against_the_oracle():
    """FlatAdamW with W^T on over a layout of three matrices (tilesC 2, 1 and 3; 2, 3 and 1 tile rows),
    1-D tiles between them and the decay boundary inside the last 1-D range; grids of 1, 2, 3 and 5
    blocks and the default. One block walks every tile of every segment in order: the forward segment
    scan, the LDS image reused by consecutive matrix tiles and the 1-D / matrix hand-over all run.
    After each of 3 steps: bit-identical across grids, within the bounds against the oracle (decay by
    default_no_decay per parameter), padding untouched, every W^T == W.t()."""
    d = _seg_data()
    base = _seg_run(4096)
    p_in, m_in, v_in = d["w0"].float(), torch.zeros(d["numel"]), torch.zeros(d["numel"])
    for s, (hi, lo, m, v) in enumerate(base):
        st = dict(p=p_in, g=d["grads"][s], m=m_in, v=v_in)
        want = _adam_oracle(st, _seg_hp(s + 1), wd=d["wdv"])
        _check_hi(hi, lo, f"seg step {s}")
        got = dict(p=_join(hi, lo), m=m, v=v)
        _adam_check(got, want, f"adamw-seg step={s + 1}")
        pad = ~d["used"]
        assert bool((got["p"][pad] == 0).all()) and bool((m[pad] == 0).all()) and bool((v[pad] == 0).all())
        p_in, m_in, v_in = got["p"], m, v
    for blocks in (1, 2, 3, 5):
        other = _seg_run(blocks)
        for s in range(SEG_STEPS):
            for k, (a, b) in enumerate(zip(other[s], base[s])):
                assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                   b.view(torch.int16) if b.dtype == torch.bfloat16 else b), (blocks, s, "hi lo m v".split()[k])
    _report("adamw-seg")


@gpu
def test_adamw_segmented_direct_call_with_a_hand_built_table():
    """rca_adamw_split_seg on DIRECT_ROWS: a ragged 1-D segment (a partial 8-group in its last tile), a
    matrix without decay, an adjacent matrix with decay, a 13-element segment without; grids of 1, 2
    blocks and the default."""
    st, hp = _direct_case(), _pset_hp(DIRECT_PSET)
    n = DIRECT_LEN
    hi0, lo0 = _split(st["p"])
    L = ops.lib()
    res = {}
    try:
        for nb in (4096, 1, 2):
            L.rca_adamw_split_set_blocks(nb)
            bufs, views = {}, {}
            for k, t in dict(hi=hi0, lo=lo0, g=st["g"], m=st["m"], v=st["v"]).items():
                bufs[k], views[k] = _padded(t)
            wts = [torch.full((C, R), 7.0, dtype=torch.bfloat16, device="cuda") for _, _, _, mat, R, C, _ in DIRECT_ROWS if mat]
            it = iter(wts)
            segs = torch.tensor([[off, cnt, first, next(it).data_ptr() if mat else 0, R, C, decay, 0]
                                 for off, cnt, first, mat, R, C, decay in DIRECT_ROWS], dtype=torch.int64, device="cuda")
            sumsq = torch.tensor([hp["sumsq"]], device="cuda")
            _lib_call("rca_adamw_split_seg", views["hi"].data_ptr(), views["lo"].data_ptr(), views["g"].data_ptr(), 0,
                      views["m"].data_ptr(), views["v"].data_ptr(), segs.data_ptr(), len(DIRECT_ROWS), DIRECT_TILES,
                      hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], 1.0 - hp["b1"] ** hp["step"],
                      1.0 - hp["b2"] ** hp["step"], hp["gm"], sumsq.data_ptr(), hp["max_norm"])
            torch.cuda.synchronize()
            _sentinels_intact(bufs, n, f"direct blocks={nb}")
            hi, lo = views["hi"].cpu(), views["lo"].cpu()
            _check_hi(hi, lo, f"direct blocks={nb}")
            res[nb] = (dict(p=_join(hi, lo), m=views["m"].cpu(), v=views["v"].cpu(), hi=hi), [w.cpu() for w in wts], lo)
    finally:
        L.rca_adamw_split_set_blocks(4096)
    _seg_check(res[4096][0], res[4096][1], DIRECT_ROWS, st, hp, "adamw-direct")
    for nb in (1, 2):
        for k in ("p", "m", "v"):
            assert torch.equal(res[nb][0][k].view(torch.int32), res[4096][0][k].view(torch.int32)), (nb, k)
        assert torch.equal(res[nb][2], res[4096][2])
        for a, b in zip(res[nb][1], res[4096][1]):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (nb, "W^T")
    _report("adamw-direct")
