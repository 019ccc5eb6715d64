"""The gfx950 flash attention forward and backward (ops/csrc/attention.hip, attention_fwd_wide.hip,
attention_fwd_hs.hip, attention_dq.hip, attention_dkdv.hip), checked per (batch, token, head) row
against a float64 oracle written here, independent of ops/reference.py and of autograd.

Metric: ``_row_err`` = max_d |out - want| / den for every (batch, token, head) row, so a row with
small values is not hidden behind a large one. For O and dV den = max_d |want| of the row. dQ and dK
rows can cancel to (nearly) nothing -- causal row 0 of dQ is exactly zero -- so their den is
max(row max, median row max of that (batch, head)): a cancelled row is scored against its head's
typical scale and no row is left out. LSE (fp32, log2 domain) is an absolute difference in log2 units.

Bounds: none is taken from a kernel. The oracle has a second mode that rounds where the kernels round
(``_head_emulated`` cites every point); the floor of a quantity is the worst ``_row_err`` of that mode
against the exact one over every case of this file (``RUNS``), measured on the CPU, and its bound is
twice the floor rounded up to a power of two (``test_bounds_are_twice_the_measured_floors``):

    quantity   floor      bound
    O          5.68e-3    2**-6  = 1.56e-2
    LSE        5.14e-6    2**-16 = 1.53e-5   (log2 units)
    dQ         1.06e-1    2**-2  = 2.50e-1
    dK         5.31e-2    2**-3  = 1.25e-1
    dV         6.94e-3    2**-6  = 1.56e-2

The dQ and dK floors are set by the spiked cases: their rows are nearly one-hot, so dS = P (dP - delta)
is a small difference of large terms and inherits the bf16 rounding of O through delta = rowsum(dO * O).
On the random cases the same floors are 6.5e-3 and 6.0e-3 (1.1e-2 / 2.1e-2 and 5.5e-3 / 1.4e-2 on the
mixed and scale cases).

Data: ``spiked`` (q_i leans on k_i and k_{i+1}, V alternates in sign) puts weight on the causal
diagonal in every row, so a one-key slip of the mask moves every row far beyond the bound; plain
``random`` covers the ordinary regime; ``mixed`` scales V and dO of batch element 1 by 2**-6. The tests
without a ``gpu`` mark run anywhere and guard the data: the exact oracle agrees with fp64 autograd,
the floors sit under half the bounds, every causal spiked case is sensitive to a dropped key i and to
a leaked key i + 1 at (at least) 99 % of its rows and at every row that begins or ends a 32-row block,
and ``_check_rows`` rejects the slipped oracle at each of those rows.

Measured on one MI355X, worst ``_row_err`` per test as O / LSE / dQ / dK / dV (the whole file, CPU tests
included, takes 6 s on the device):
    test_rows_d128, every path but fwd-hs   5.83e-3 / 3.02e-6 / 9.27e-2 / 4.57e-2 / 6.80e-3
    test_rows_d128, fwd-hs                  6.95e-3 / 3.02e-6 / 9.27e-2 / 4.57e-2 / 6.80e-3
    test_rows_d64                           8.34e-3 / 2.78e-6 / 1.06e-1 / 4.65e-2 / 6.94e-3
    test_rows_with_a_scale_of_its_own       5.70e-3 / 2.46e-6 / 2.61e-2 / 1.25e-2 / 6.42e-3
    test_rows_from_strided_views            5.54e-3 / 3.21e-6 / 6.83e-2 / 5.45e-2 / 6.19e-3
    test_rows_of_mixed_magnitude            5.38e-3 / 9.86e-7 / 1.07e-2 / 5.21e-3 / 5.75e-3
The kernels sit on the oracle's rounding floor on every path; the largest share of a bound any row used is
0.53 (O, spiked 1x384x4x2x64 causal).
"""
import contextlib
import functools
import math

import pytest
import torch

from ray_community_amd import ops

gpu = pytest.mark.gpu

KINDS = ("O", "LSE", "dQ", "dK", "dV")
BOUND = {"O": 2.0 ** -6, "LSE": 2.0 ** -16, "dQ": 2.0 ** -2, "dK": 2.0 ** -3, "dV": 2.0 ** -6}
LN2 = math.log(2.0)
NAN = float("nan")


# ------------------------------------------------------------------------------------ the oracle
def _mask(S, causal, slip=0):
    """[query, key] bool. slip 0: the true mask; -1: key i dropped from row i (row 0 keeps key 0);
    +1: key i + 1 leaked into row i."""
    if not causal:
        return torch.ones(S, S, dtype=torch.bool)
    i = torch.arange(S)
    m = i[None, :] <= i[:, None] + slip
    m[0, 0] = True
    return m


def _head_exact(q, k, v, do, scale, mask):
    """One (batch, query head) in float64, closed form: q, do [S, D], its kv head's k, v [S, D].
    Returns O, LSE2 = logsumexp(scale * s) / ln 2, dQ and this head's contributions to dK and dV."""
    s = (q @ k.T * scale).masked_fill(~mask, -math.inf)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[:, None])
    o = p @ v
    dp = do @ v.T
    delta = (do * o).sum(-1)
    ds = p * (dp - delta[:, None])
    return o, lse / LN2, scale * ds @ k, scale * ds.T @ q, p.T @ do


def _bf(x):
    return x.bfloat16().float()


def _head_emulated(q, k, v, do, scale, mask):
    """The same head in the kernels' arithmetic: float32 where they keep float32 (MFMA accumulators,
    exp2 arguments, row sums, LSE, delta) and a bf16 rounding at each of these points:
      * scale2 = scale * log2(e) as a float32 product          attention.hip:519, 535 and 556
      * P, relative to the running max, ahead of P.V           attention.hip:163-164, attention_fwd_wide.hip:120-121,
                                                               attention_fwd_hs.hip:179-180 and 212-213
        (the row sum adds the unrounded P, attention.hip:159-162)
      * O on the way out                                       attention.hip:226 (store4 -> f2bf, common.h:27)
      * delta = rowsum(dO * O) from that bf16 O                attention.hip:304-306, attention_dq.hip:37-47
      * P = exp2(s * scale2 - LSE) ahead of P^T.dO             attention_dkdv.hip:145 and 529, 534, 571, 584
      * dS = P * (dP - delta), P unrounded, ahead of dS^T.Q    attention_dkdv.hip:146 and 530, 535, 572, 585; the same
        and dS.K; scale is applied to the sums afterwards      registers are the workspace tiles (attention_dkdv.hip:
                                                               576-604) that attention_dq.hip:149 reads;
                                                               attention.hip:363-364
      * dQ, and dK / dV after the sum over the G query heads   attention.hip:396, attention_dq.hip:171,
        of a kv head (returned unrounded: ``_oracle`` rounds)  attention_dkdv.hip:197-199 and 633-635
    Returns float32 tensors; O and dQ are rounded, the dK / dV contributions are not."""
    f32 = torch.float32
    q, k, v, do = (t.to(f32) for t in (q, k, v, do))
    scale = torch.tensor(scale, dtype=f32)
    scale2 = scale * torch.tensor(1.4426950408889634, dtype=f32)
    x = ((q @ k.T) * scale2).masked_fill(~mask, -math.inf)
    m = x.amax(-1)
    p = torch.exp2(x - m[:, None])
    lsum = p.sum(-1)
    o = _bf((_bf(p) @ v) / lsum[:, None])
    lse2 = m + torch.log2(lsum)
    p = torch.exp2(x - lse2[:, None])
    delta = (do * o).sum(-1)
    ds = _bf(p * (do @ v.T - delta[:, None]))
    return o, lse2, _bf(scale * (ds @ k)), scale * (ds.T @ q), _bf(p).T @ do


def _oracle(c, causal, scale, emulate=False, slip=0):
    """Every head of a case: O, dQ [B, S, Hq, D], LSE [B, Hq, S], dK, dV [B, S, Hk, D], float64."""
    B, S, Hq, D = c["q"].shape
    Hk = c["k"].shape[2]
    G = Hq // Hk
    scale = D ** -0.5 if scale is None else scale
    mask = _mask(S, causal, slip)
    head = _head_emulated if emulate else _head_exact
    acc = torch.float32 if emulate else torch.float64
    out = dict(O=torch.zeros(B, S, Hq, D, dtype=acc), LSE=torch.zeros(B, Hq, S, dtype=acc),
               dQ=torch.zeros(B, S, Hq, D, dtype=acc), dK=torch.zeros(B, S, Hk, D, dtype=acc),
               dV=torch.zeros(B, S, Hk, D, dtype=acc))
    for b in range(B):
        for h in range(Hq):
            o, lse2, dq, dk, dv = head(c["q"][b, :, h].double(), c["k"][b, :, h // G].double(),
                                       c["v"][b, :, h // G].double(), c["do"][b, :, h].double(), scale, mask)
            out["O"][b, :, h], out["LSE"][b, h], out["dQ"][b, :, h] = o, lse2, dq
            out["dK"][b, :, h // G] += dk
            out["dV"][b, :, h // G] += dv
    if emulate:
        out["dK"], out["dV"] = _bf(out["dK"]), _bf(out["dV"])
    return {n: t.double() for n, t in out.items()}


# ------------------------------------------------------------------------------------ the metric
def _row_err(out, want, kind):
    """Per-row error of one quantity (see the module docstring): [B, S, H], or [B, Hq, S] for LSE.
    A row of O or dV whose ``want`` is exactly zero scores 0 if ``out`` is zero there and inf if not."""
    a, b = out.detach().cpu().double(), want.double()
    if kind == "LSE":
        return (a - b).abs()
    num, den = (a - b).abs().amax(-1), b.abs().amax(-1)
    if kind in ("dQ", "dK"):
        den = torch.maximum(den, den.median(dim=1, keepdim=True).values)
    err = num / den.clamp_min(1e-300)
    return torch.where(den > 0, err, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)))


def _check_rows(got, want, label, bound=None):
    """The assertion every comparison below makes, for each quantity in ``got``: dtype (bf16; LSE
    fp32), shape, finiteness, and every row within its bound. Prints and returns the worst rows."""
    bound = BOUND if bound is None else bound
    worst = {}
    for kind in KINDS:
        if kind not in got:
            continue
        t = got[kind]
        assert t.dtype == (torch.float32 if kind == "LSE" else torch.bfloat16), (label, kind, t.dtype)
        assert tuple(t.shape) == tuple(want[kind].shape), (label, kind, tuple(t.shape))
        assert torch.isfinite(t).all(), (label, kind)
        worst[kind] = _row_err(t, want[kind], kind).max().item()
    print(f"{label}: worst row " + "  ".join(f"{k} {w:.3e} ({w / bound[k]:.2f} x bound)" for k, w in worst.items()))
    for kind, w in worst.items():
        assert w < bound[kind], (label, kind, w, bound[kind])
    return worst


# ------------------------------------------------------------------------------------- case data
SPIKE_A = {128: 0.6, 64: 0.9}  # the diagonal score sits 6 to 7 above the noise after D**-0.5
# (kind, B, S, Hq, Hk, D) -> seed, where the default seed fails the sensitivity condition
RESEEDED = {}


@functools.lru_cache(maxsize=None)
def _case(kind, B, S, Hq, Hk, D):
    """q, do [B, S, Hq, D] and k, v [B, S, Hk, D] in bf16, on the CPU, from one seeded generator."""
    G = Hq // Hk
    seed = RESEEDED.get((kind, B, S, Hq, Hk, D), ((B * 1000 + S) * 100 + Hq) * 1000 + Hk * 200 + D)
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, S + 1, Hk, D, generator=g).bfloat16().float()  # key S only shapes q[S - 1]
    v = torch.randn(B, S, Hk, D, generator=g)
    q = torch.randn(B, S, Hq, D, generator=g)
    do = torch.randn(B, S, Hq, D, generator=g)
    if kind == "spiked":
        v += 1.5 * (1.0 - 2.0 * (torch.arange(S) % 2))[None, :, None, None]
        q += SPIKE_A[D] * (k[:, :-1] + k[:, 1:]).repeat_interleave(G, dim=2)
    elif kind == "mixed":
        v[1] *= 2.0 ** -6
        do[1] *= 2.0 ** -6
    else:
        assert kind == "random"
    return dict(q=q.bfloat16(), k=k[:, :S].bfloat16(), v=v.bfloat16(), do=do.bfloat16())


@functools.lru_cache(maxsize=None)
def _want(run, emulate=False, slip=0):
    """The oracle of a run = (kind, B, S, Hq, Hk, D, causal, scale), computed once and shared."""
    *case, causal, scale = run
    return _oracle(_case(*case), causal, scale, emulate, slip)


# B, S, Hq, Hk, head sizes, why
SHAPES = [
    (1, 128, 2, 1, (128, 64)),   # one key tile, diagonal only
    (1, 384, 4, 2, (128, 64)),   # S % 256 != 0: 4-wave forward, dq_qw falls to 1, fwd modes 1 / 2 fall back
    (1, 512, 4, 4, (128, 64)),   # two 256-row workgroups, dq_qw = 2, G = 1
    (3, 256, 9, 3, (128,)),      # G = 3; B * Hk = 9 takes the xcd_remap branch, grid not a multiple of 8
    (2, 256, 16, 4, (128, 64)),  # B * Hk = 8: the XCD-grouped branch at its smallest
]


def _matrix_run(B, S, Hq, Hk, D, causal):
    return ("spiked" if causal else "random", B, S, Hq, Hk, D, causal, None)


MATRIX = [_matrix_run(B, S, Hq, Hk, D, causal) for B, S, Hq, Hk, Ds in SHAPES for D in Ds for causal in (True, False)]
SCALE_RUNS = [("random", 1, 384, 4, 2, 128, True, sc) for sc in (0.03, 0.2)]
SCALE_RUNS += [("random", 1, 256, 4, 2, 64, True, sc) for sc in (0.03, 0.2)]
STRIDE_RUNS = [("spiked", 2, 256, 4, 2, 128, True, None), ("spiked", 2, 256, 4, 2, 64, True, None)]
MIXED_RUN = ("mixed", 2, 256, 4, 2, 128, True, None)
RUNS = MATRIX + SCALE_RUNS + STRIDE_RUNS + [MIXED_RUN]
SPIKED_CAUSAL = [r for r in RUNS if r[0] == "spiked" and r[6]]


def _id(run):
    kind, B, S, Hq, Hk, D, causal, scale = run
    tail = "" if scale is None else f"-scale{scale}"
    return f"{kind}-{B}x{S}x{Hq}x{Hk}x{D}-{'causal' if causal else 'full'}{tail}"


# ---------------------------------------------------------------- CPU tests: guard the test data
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Hq,Hk", [(2, 2), (3, 1)])
def test_exact_oracle_matches_fp64_autograd(Hq, Hk, causal):
    """The closed-form backward against autograd through a plain softmax attention, G = 1 and 3."""
    c = _case("spiked", 2, 128, Hq, Hk, 64)
    scale = 0.11
    want = _oracle(c, causal, scale)
    q, k, v = (c[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    kk, vv = (t.repeat_interleave(Hq // Hk, dim=2) for t in (k, v))
    s = torch.einsum("bihd,bjhd->bhij", q, kk) * scale
    s = s.masked_fill(~_mask(128, causal), -math.inf)
    o = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), vv)
    o.backward(c["do"].double())
    got = dict(O=o.detach(), LSE=torch.logsumexp(s, dim=-1).detach() / LN2, dQ=q.grad, dK=k.grad, dV=v.grad)
    for kind in KINDS:
        assert (got[kind] - want[kind]).abs().max().item() < 1e-10, kind


def test_single_batch_slices_are_admitted_to_the_kernels():
    """k of every B = 1 case here is x[:, :S] of a [1, S + 1, Hk, D] tensor: contiguous, but with a
    batch stride that is not S * stride(1). ``flash_attention`` used to send such an operand to the
    eager reference without a word; the batch stride of one batch element is never used."""
    k = _case("spiked", 1, 128, 2, 1, 128)["k"]
    assert k.is_contiguous() and k.stride(0) != 128 * k.stride(1)
    assert ops._token_major_ok(k)
    two = torch.zeros(2, 129, 1, 64, dtype=torch.bfloat16)[:, :128]
    assert not two.is_contiguous() and not ops._token_major_ok(two)


def test_bounds_are_twice_the_measured_floors():
    """The reference for BOUND: the rounding-emulating oracle against the exact one, worst row over
    every run of the file; each bound is twice its floor rounded up to a power of two."""
    floor = dict.fromkeys(KINDS, 0.0)
    for run in RUNS:
        exact, emu = _want(run), _want(run, True)
        for kind in KINDS:
            e = _row_err(emu[kind], exact[kind], kind).max().item()
            floor[kind] = max(floor[kind], e)
    for kind in KINDS:
        print(f"{kind}: floor {floor[kind]:.3e}, bound {BOUND[kind]:.3e} = 2**{math.log2(BOUND[kind]):.0f}")
    for kind in KINDS:
        assert 0 < floor[kind] < BOUND[kind] / 2, kind
        assert BOUND[kind] == 2.0 ** math.ceil(math.log2(2 * floor[kind])), kind


def _edge_rows(S):
    """Rows that are first or last in a 32-row block (hence in every 64-, 128- and 256-row block)."""
    return [i for i in range(S) if i % 32 in (0, 31)]


def _slip_sensitivity(run, slip):
    """[B, S, Hq] bool: row (b, i, h) moves by >= 2 x bound in its O, its LSE, or the dV row of the
    key that slipped (key i for the drop, key i + 1 for the leak); and the rows where a slip acts."""
    _, B, S, Hq, Hk, D, _, _ = run
    true, bad = _want(run), _want(run, False, slip)
    sens = _row_err(bad["O"], true["O"], "O") >= 2 * BOUND["O"]
    sens |= (_row_err(bad["LSE"], true["LSE"], "LSE") >= 2 * BOUND["LSE"]).transpose(1, 2)
    dv = (_row_err(bad["dV"], true["dV"], "dV") >= 2 * BOUND["dV"]).repeat_interleave(Hq // Hk, dim=2)
    live = torch.ones(S, dtype=torch.bool)
    if slip < 0:
        sens |= dv
        live[0] = False
    else:
        sens[:, :-1] |= dv[:, 1:]
        live[S - 1] = False
    return sens, live


@pytest.mark.parametrize("slip", [-1, 1], ids=["drop", "leak"])
@pytest.mark.parametrize("run", SPIKED_CAUSAL, ids=_id)
def test_spiked_cases_are_sensitive_to_a_one_key_mask_slip(run, slip):
    S = run[2]
    sens, live = _slip_sensitivity(run, slip)
    frac = sens[:, live].double().mean().item()
    print(f"{_id(run)} slip {slip:+d}: {100 * frac:.2f} % of rows sensitive")
    assert frac >= 0.99
    edges = [i for i in _edge_rows(S) if live[i]]
    assert sens[:, edges].all()


@pytest.mark.parametrize("slip", [-1, 1], ids=["drop", "leak"])
@pytest.mark.parametrize("run", SPIKED_CAUSAL, ids=_id)
def test_check_rows_rejects_a_slip_at_any_block_edge_row(run, slip, capsys):
    """The slipped oracle, rounded as the kernels' outputs are, standing in for ONE block-edge row
    (its O, its LSE and the slipped key's dV row; every head) fails ``_check_rows``; intact, it passes."""
    S = run[2]
    true, bad = _want(run), _want(run, False, slip)

    def rounded(w):
        return {k: t.float() if k == "LSE" else t.bfloat16() for k, t in w.items()}

    _check_rows(rounded(true), true, f"intact {_id(run)}")
    for i in _edge_rows(S):
        if (slip < 0 and i == 0) or (slip > 0 and i == S - 1):
            continue
        fake = {k: t.clone() for k, t in true.items()}
        key = i if slip < 0 else i + 1
        fake["O"][:, i], fake["LSE"][:, :, i] = bad["O"][:, i], bad["LSE"][:, :, i]
        fake["dV"][:, key] = bad["dV"][:, key]
        with pytest.raises(AssertionError):
            _check_rows(rounded(fake), true, f"slip {slip:+d} at row {i}")
    capsys.readouterr()  # one line per row: not worth keeping


# ------------------------------------------------------------------------------------- GPU tests
@contextlib.contextmanager
def _policy(**switches):
    """Select kernel paths with the library's setters (fwd_nw, fwd_mode, bwd_mode, dkdv_hs, hs_nops,
    dq_qw); every change is put back."""
    lib, prev = ops.lib(), []
    try:
        for name, value in switches.items():
            setter = getattr(lib, f"rca_attn_set_{name}")
            prev.append((setter, setter(value)))
        yield
    finally:
        for setter, old in reversed(prev):
            setter(old)


def _run(run, via="split", **switches):
    """Forward and backward of a run on the GPU. via: "split" = contiguous q, k, v through
    flash_attention; "qkv" = flash_attention_qkv on the fused rows; "views" = q, k, v as head slices of
    one NaN-padded [B, S, heads, D] buffer through flash_attention, with a non-contiguous dO."""
    kind, B, S, Hq, Hk, D, causal, scale = run
    c = _case(kind, B, S, Hq, Hk, D)
    assert ops.flash_attention_supported(S, D, Hq, Hk)  # the kernels, not the reference
    do = c["do"].cuda()
    with _policy(**switches):
        if via == "qkv":
            qkv = torch.cat([c[n].reshape(B * S, -1) for n in ("q", "k", "v")], dim=1).cuda().requires_grad_(True)
            o = ops.flash_attention_qkv(qkv, B, S, Hq, Hk, D, causal=causal, scale=scale)
            lse = o.grad_fn.saved_tensors[-1]
            o.backward(do.reshape(B * S, Hq * D))
            g = qkv.grad.view(B, S, Hq + 2 * Hk, D)
            o, grads = o.view(B, S, Hq, D), (g[:, :, :Hq], g[:, :, Hq: Hq + Hk], g[:, :, Hq + Hk:])
        else:
            if via == "views":
                # heads: NaN | q | NaN | k | NaN | v | NaN
                buf = torch.full((B, S, Hq + 2 * Hk + 4, D), NAN, dtype=torch.bfloat16, device="cuda")
                at = (1, Hq + 2, Hq + Hk + 3)
                qkv = []
                for n, a in zip(("q", "k", "v"), at):
                    view = buf[:, :, a: a + c[n].shape[2]]
                    view.copy_(c[n])
                    qkv.append(view.detach().requires_grad_(True))
                    assert not qkv[-1].is_contiguous() and ops._token_major_ok(qkv[-1])
                assert int(torch.isnan(buf).all(-1).sum()) == 4 * B * S
                wide = torch.full((B, S, Hq, 2 * D), NAN, dtype=torch.bfloat16, device="cuda")
                wide[..., :D] = do
                do = wide[..., :D]
                assert not do.is_contiguous()
            else:
                qkv = [c[n].cuda().requires_grad_(True) for n in ("q", "k", "v")]
            o = ops.flash_attention(*qkv, causal, scale)
            assert type(o.grad_fn).__name__.startswith("_FlashAttn")
            lse = o.grad_fn.saved_tensors[-1]
            o.backward(do)
            grads = tuple(t.grad for t in qkv)
        torch.cuda.synchronize()
    return dict(O=o.detach().cpu(), LSE=lse.cpu(), dQ=grads[0].cpu(), dK=grads[1].cpu(), dV=grads[2].cpu())


# D = 128 kernel paths. S % 256 != 0 runs the 4-wave forward and dq_qw = 1 whatever is set, and sends
# forward modes 1 / 2 back to mode 0, so those switches are exercised where S % 256 == 0 only.
PATHS = {
    "default": dict(fwd_mode=0, fwd_nw=8, bwd_mode=1, dq_qw=2, hs_nops=1),
    "fwd-4-waves": dict(fwd_mode=0, fwd_nw=4),
    "fwd-wide": dict(fwd_mode=1),
    "fwd-hs": dict(fwd_mode=2),
    "dq-1-block": dict(bwd_mode=1, dq_qw=1),
    "ds-nops-3": dict(bwd_mode=1, hs_nops=3),
    "recompute-dkdv-0": dict(bwd_mode=0, dkdv_hs=0),
    "recompute-dkdv-1": dict(bwd_mode=0, dkdv_hs=1),
    "recompute-dkdv-2": dict(bwd_mode=0, dkdv_hs=2),
}
NEEDS_S256 = ("fwd-4-waves", "fwd-wide", "fwd-hs", "dq-1-block")
MATRIX_128 = [(run, path) for run in MATRIX if run[5] == 128 for path in PATHS
              if run[2] % 256 == 0 or path not in NEEDS_S256]


@gpu
@pytest.mark.parametrize("run,path", MATRIX_128, ids=[f"{_id(r)}-{p}" for r, p in MATRIX_128])
def test_rows_d128(run, path):
    _check_rows(_run(run, **PATHS[path]), _want(run), f"{_id(run)} {path}")


@gpu
@pytest.mark.parametrize("run", [r for r in MATRIX if r[5] == 64], ids=_id)
def test_rows_d64(run):
    """The default forward, the recomputing dQ and the compiler-scheduled dK/dV."""
    assert ops.lib().rca_attn_bwd_ws_bytes(*run[1:6], int(run[6])) == 0
    _check_rows(_run(run), _want(run), _id(run))


@gpu
@pytest.mark.parametrize("via", ["split", "qkv"])
@pytest.mark.parametrize("run", SCALE_RUNS, ids=_id)
def test_rows_with_a_scale_of_its_own(run, via):
    """scale reaches the forward and dK/dV as scale * log2(e) and every gradient's last factor as scale."""
    _check_rows(_run(run, via=via), _want(run), f"{_id(run)} {via}")
    if run[5] == 128 and via == "split":
        _check_rows(_run(run, bwd_mode=0), _want(run), f"{_id(run)} {via} recompute")


@gpu
@pytest.mark.parametrize("run", STRIDE_RUNS, ids=_id)
def test_rows_from_strided_views(run):
    _check_rows(_run(run, via="views"), _want(run), f"{_id(run)} views")
    if run[5] == 128:
        _check_rows(_run(run, via="views", bwd_mode=0), _want(run), f"{_id(run)} views recompute")


@gpu
@pytest.mark.parametrize("bwd_mode", [1, 0])
def test_rows_of_mixed_magnitude(bwd_mode):
    """Batch element 1 has V and dO (so O, dQ, dK, dV) 2**-6 of element 0's: its rows hold the bound too."""
    got, want = _run(MIXED_RUN, bwd_mode=bwd_mode), _want(MIXED_RUN)
    _check_rows(got, want, f"{_id(MIXED_RUN)} bwd_mode={bwd_mode}")
    small = {k: t[1:] for k, t in got.items()}
    _check_rows(small, {k: t[1:] for k, t in want.items()}, f"{_id(MIXED_RUN)} bwd_mode={bwd_mode}, the small element")
    assert want["O"][1].abs().max() < 2.0 ** -4 * want["O"][0].abs().max()
