"""The FP8 paged KV cache without a GPU: the quantiser's properties, the reference paths of
``ops.kv_cache_append_`` / ``paged_attention_decode`` / ``paged_attention_extend`` with scales,
``PagedKVCache(kv_dtype="fp8")``, llama3-tiny generation over an fp8 cache, and the guards of the
data that tests/test_kv_cache_fp8_gpu.py runs the kernels on.

Format: e4m3 bytes plus one fp32 power-of-two scale per (token, kv head); byte times scale is exact
in bf16 and fp32, so attention over an fp8 cache is attention over exactly known values and is
checked against the float64 oracle of the DEQUANTISED cache at the bf16 kernels' bound: metric
``_row_err`` = max_d |out - want| / max_d |want| per (sequence or token, head) row, ``ROW_BOUND`` =
2**-7 = twice the bf16 rounding floor of an output row (tests/test_attention_decode_edges_gpu.py,
whose oracle and metric are copied here; that argument needs exact inputs, fp32 math and a bf16
output, all of which hold).

Case data ("scale-sensitive"): K and V are N(0, 1) times a power of two per (token, kv head); the
four multipliers of a token (K, V x 2 heads) are distinct members of 2^-6, 2^-3 .. 2^6, so its four
scales differ pairwise (``test_case_scales_differ_inside_a_token``). Caches are poisoned outside the live slots (bytes 0x7F = e4m3
NaN, scales NaN), blocks are handed out in shuffled order and block-table padding points at a
block that stays all poison. ``test_*_cases_are_scale_sensitive`` shows on the oracle alone that
setting every scale to 1, swapping k_scale with v_scale, or swapping the two kv heads' scales each
move every sequence of every case by at least 2 * ROW_BOUND, so a kernel that does any of it
fails the GPU tests.
"""
import functools
import itertools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, build_llama
from ray_community_amd.models.kv_cache import PagedKVCache
from ray_community_amd.ops import reference as ref
from test_attention_extend_gpu import _oracle as _extend_oracle

ROW_BOUND = 2.0 ** -7
HK = 2
NAN = float("nan")
FP8 = torch.float8_e4m3fn
POISON = 0x7F  # e4m3 NaN


# ------------------------------------------------- oracle and metric (decode: copied, see above)
def _attend(q, k, v, G, scale):
    """float64 attention of one token: q [Hq, D], k / v [n, Hk, D] -> [Hq, D]; kv head = h // G."""
    out = torch.zeros_like(q)
    for h in range(q.shape[0]):
        s = (k[:, h // G] @ q[h]) * scale
        p = torch.exp(s - s.max())
        out[h] = (p / p.sum()) @ v[:, h // G]
    return out


def _oracle(q, k_cache, v_cache, table, lens, Hq, Hk, D, scale):
    """Paged single-token attention in float64 on the CPU: token i of sequence b lives in slot
    table[b, i // page] * page + i % page. Returns [B, Hq*D]; zeros where the length is 0."""
    page = k_cache.shape[1]
    kf = k_cache.detach().cpu().double().reshape(-1, Hk, D)
    vf = v_cache.detach().cpu().double().reshape(-1, Hk, D)
    qf = q.detach().cpu().double()[:, : Hq * D].reshape(-1, Hq, D)
    table = table.tolist()
    lens = lens.tolist() if torch.is_tensor(lens) else list(lens)
    out = torch.zeros(len(lens), Hq, D, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        slots = [table[b][i // page] * page + i % page for i in range(n)]
        out[b] = _attend(qf[b], kf[slots], vf[slots], Hq // Hk, scale)
    return out.reshape(len(lens), Hq * D)


def _rows(t, D):
    t = t.detach().cpu().double()
    return t.reshape(t.shape[0], -1, D)


def _row_err(out, want, D):
    """[rows, Hq] tensor of max_d |out - want| / max_d |want|; all-zero rows of ``want`` give 0."""
    a, b = _rows(out, D), _rows(want, D)
    num, den = (a - b).abs().amax(-1), b.abs().amax(-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))


def _check_rows(out, want, D, label):
    """bf16, finite, all-zero rows of ``want`` exactly zero, every other row within ROW_BOUND."""
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == tuple(want.shape)
    assert torch.isfinite(out).all(), f"{label}: non-finite output"
    dead = _rows(want, D).abs().amax(-1) == 0
    assert (_rows(out, D)[dead] == 0).all()
    worst = _row_err(out, want, D).max().item() if out.numel() else 0.0
    print(f"{label}: max row err {worst:.3e} (bound {ROW_BOUND:.3e})")
    assert worst < ROW_BOUND, label
    return worst


def _dequant64(fp8, scale):
    """The cache as float64, exactly (dead slots: NaN)."""
    return fp8.double() * scale.double().unsqueeze(-1)


# ------------------------------------------------------------------------------------ case data
EXPS = (-6, -3, 0, 3, 6)  # three binary orders apart: a row's amax / 2^e lies within (0.875, 7]


def _scaled_kv(n, D, g):
    """K, V [n, HK, D] bf16 = N(0, 1) times a power of two per (token, kv head), the four of a token
    distinct (module docstring)."""
    k, v = torch.randn(n, HK, D, generator=g), torch.randn(n, HK, D, generator=g)
    if n:
        pick = torch.stack([torch.randperm(len(EXPS), generator=g)[:2 * HK] for _ in range(n)])
        mul = torch.exp2(torch.tensor(EXPS, dtype=torch.float32)[pick])  # [n, 4]: K heads, then V heads
        k, v = k * mul[:, :HK, None], v * mul[:, HK:, None]
    return k.bfloat16(), v.bfloat16()


def poisoned_cache(num_blocks, page, D, device="cpu"):
    """(k, v, k_scale, v_scale) of an fp8 cache holding the poison pattern everywhere."""
    k = torch.full((num_blocks, page, HK, D), POISON, dtype=torch.uint8, device=device).view(FP8)
    ks = torch.full((num_blocks, page, HK), NAN, dtype=torch.float32, device=device)
    return k, k.clone(), ks, ks.clone()


def _paged_fp8(Ks, Vs, page, perm, D):
    """Quantise the logical per-sequence K / V (``ref.kv_quantize_fp8_ref``) and lay them out in a
    poisoned cache, taking physical blocks in the order ``perm``; unused table entries hold the
    id of a valid block that stays all poison."""
    need = [-(-k.shape[0] // page) for k in Ks]
    assert len(perm) > sum(need)
    pad = perm[sum(need)]
    table = torch.full((len(Ks), max(need + [1])), pad, dtype=torch.int32)
    k8, v8, ks, vs = poisoned_cache(len(perm), page, D)
    nxt = 0
    for b, (k, v) in enumerate(zip(Ks, Vs)):
        blocks = perm[nxt: nxt + need[b]]
        nxt += need[b]
        table[b, : need[b]] = torch.tensor(blocks, dtype=torch.int32)
        slots = torch.tensor([blocks[i // page] * page + i % page for i in range(k.shape[0])], dtype=torch.long)
        for x, x8, xs in ((k, k8, ks), (v, v8, vs)):
            qx, sx = ref.kv_quantize_fp8_ref(x)
            x8.view(torch.uint8).view(-1, HK, D)[slots] = qx.view(torch.uint8)
            xs.view(-1, HK)[slots] = sx
    assert (k8[pad].view(torch.uint8) == POISON).all() and torch.isnan(ks[pad]).all()
    return dict(k=k8, v=v8, ks=ks, vs=vs, table=table)


def _vary(c, variant):
    """The scales of case ``c`` as a wrong kernel would see them."""
    ks, vs = c["ks"], c["vs"]
    if variant == "ones":
        return torch.where(torch.isnan(ks), ks, torch.ones_like(ks)), torch.where(torch.isnan(vs), vs, torch.ones_like(vs))
    if variant == "kv":
        return vs, ks
    if variant == "heads":
        return ks.flip(-1), vs.flip(-1)
    assert variant is None
    return ks, vs


VARIANTS = ("ones", "kv", "heads")

# decode: the issue's matrix
DEC_PAGES, DEC_DS, DEC_GS = (16, 48), (64, 128), (1, 2, 4, 8)


def dec_lens(page):
    return [0, 1, 15, 16, 17, page, page + 1, 300]


@functools.lru_cache(maxsize=None)
def dec_case(page, D, G):
    lens = dec_lens(page)
    g = torch.Generator().manual_seed(8000 + 1000 * page + 10 * D + G)
    kv = [_scaled_kv(n, D, g) for n in lens]
    qkv = torch.randn(len(lens), (HK * G + 2 * HK) * D, generator=g).bfloat16()  # fused row: q leads
    perm = torch.randperm(sum(-(-n // page) for n in lens) + 4, generator=g).tolist()
    c = _paged_fp8([k for k, _ in kv], [v for _, v in kv], page, perm, D)
    c.update(q=qkv, lens=lens, Hq=HK * G, D=D, G=G, page=page, Ks=[k for k, _ in kv], Vs=[v for _, v in kv])
    return c


@functools.lru_cache(maxsize=None)
def dec_want(page, D, G, variant=None):
    """float64 oracle of the dequantised cache, computed once per case."""
    c = dec_case(page, D, G)
    ks, vs = _vary(c, variant)
    return _oracle(c["q"], _dequant64(c["k"], ks), _dequant64(c["v"], vs), c["table"], c["lens"], c["Hq"], HK, D,
                   D ** -0.5)


def run_decode(c, device, **kw):
    lens = torch.tensor(c["lens"], dtype=torch.int32)
    t = [x.to(device) for x in (c["q"], c["k"], c["v"], c["table"], lens)]
    out = ops.paged_attention_decode(*t, c["Hq"], HK, c["D"], k_scale=c["ks"].to(device), v_scale=c["vs"].to(device),
                                     **kw)
    return out.cpu()


# extend: chunk lengths 1, 5, 16, 130; every context starts inside a page of 48 and the 16- and
# 130-token chunks straddle page boundaries; one chunk starts an empty sequence
EXT_PAGE = 48
EXT_SEQS = ((7, 1), (40, 5), (45, 16), (20, 130), (0, 16))
EXT_DS, EXT_GS = (64, 128), (1, 4, 8)


@functools.lru_cache(maxsize=None)
def ext_case(D, G):
    """A case dict in the layout of tests/test_attention_extend_gpu.py::_case, plus the fp8 cache."""
    page, seqs = EXT_PAGE, EXT_SEQS
    g = torch.Generator().manual_seed(9000 + 10 * D + G)
    Hq = HK * G
    T = sum(n for _, n in seqs)
    q = torch.randn(T, Hq * D, generator=g).bfloat16()
    kv = [_scaled_kv(p + n, D, g) for p, n in seqs]
    perm = torch.randperm(sum(-(-(p + n) // page) for p, n in seqs) + 3, generator=g).tolist()
    c = _paged_fp8([k for k, _ in kv], [v for _, v in kv], page, perm, D)
    cu = [0] + list(itertools.accumulate(n for _, n in seqs))
    c.update(page=page, D=D, Hq=Hq, seqs=list(seqs), scale=D ** -0.5, q=q, cu=torch.tensor(cu, dtype=torch.int32),
             lens=torch.tensor([p + n for p, n in seqs], dtype=torch.int32), max_q=max(n for _, n in seqs))
    return c


@functools.lru_cache(maxsize=None)
def ext_want(D, G, variant=None):
    c = ext_case(D, G)
    ks, vs = _vary(c, variant)
    return _extend_oracle(dict(c, k_cache=_dequant64(c["k"], ks), v_cache=_dequant64(c["v"], vs)))


def run_extend(c, device, **kw):
    d = torch.device(device)
    out = ops.paged_attention_extend(c["q"].to(d), c["k"].to(d), c["v"].to(d), c["table"].to(d), c["lens"].to(d),
                                     c["cu"].to(d), c["max_q"], c["Hq"], HK, c["D"], k_scale=c["ks"].to(d),
                                     v_scale=c["vs"].to(d), **kw)
    return out.cpu()


# --------------------------------------------------------------------------------- the quantiser
def magnitude_rows(D, seed=0):
    """bf16 rows [R, D]: N(0, 1) times 2^-120 .. 300, an all-zero row, rows whose amax is exactly
    448 * 2^k, and rows whose amax is the next bf16 above it (450 * 2^k)."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(D, generator=g) * m for m in
            [2.0 ** e for e in (-120, -110, -90, -60, -30, -14, -7, -1, 0, 1, 5)] + [3.0, 100.0, 300.0]]
    rows.append(torch.zeros(D))
    for k in (-130, -20, -3, 0, 7, 100):
        for top in (448.0, 450.0):
            r = (torch.rand(D, generator=g) * 2 - 1) * 440.0
            r[int(torch.randint(D, (1,), generator=g))] = -top if k % 2 else top
            rows.append(r * 2.0 ** k if k > -127 else r * 2.0 ** -100 * 2.0 ** (k + 100))
    return torch.stack(rows).bfloat16()


@pytest.mark.parametrize("D", [64, 128])
def test_quantiser_properties(D):
    x = magnitude_rows(D)
    q, s = ref.kv_quantize_fp8_ref(x)
    assert q.dtype == FP8 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == x.shape[:1]
    xf = x.float()
    amax = xf.abs().amax(-1)
    mant, _ = torch.frexp(s)
    assert (mant == 0.5).all() and (s >= 2.0 ** -126).all()  # powers of two, clamped below
    scaled = amax / s  # exact: a power-of-two divisor
    assert (scaled <= 448).all()
    clamped = s == 2.0 ** -126
    assert clamped.any() and (~clamped).any()
    assert (scaled[~clamped & (amax > 0)] > 224).all()
    zero = amax == 0
    assert zero.sum() == 1 and (s[zero] == 1).all() and (q[zero].view(torch.uint8) == 0).all()
    exact448 = (scaled == 448).sum().item()
    assert exact448 >= 3, "the rows with amax = 448 * 2^k must land on 448 exactly"
    assert torch.isfinite(q.float()).all()
    deq = ref.kv_dequantize_fp8_ref(q, s, torch.float32)
    assert torch.equal(deq.bfloat16().float(), deq)  # exact in bf16
    assert torch.equal(ref.kv_dequantize_fp8_ref(q, s).float(), deq)
    assert ((deq - xf).abs() <= 2.0 ** -4 * xf.abs() + 2.0 ** -10 * s[:, None]).all()
    # the stored element is RNE of the exact quotient, recomputed here without the reference
    want = torch.stack([(xf[r] / s[r]).to(FP8).view(torch.uint8) for r in range(x.shape[0])])
    assert torch.equal(q.view(torch.uint8), want)


def test_scale_is_the_smallest_power_of_two():
    x = magnitude_rows(128)
    _, s = ref.kv_quantize_fp8_ref(x)
    amax = x.float().abs().amax(-1).double()
    s = s.double()
    free = (s > 2.0 ** -126) & (amax > 0)
    assert (amax[free] / (s[free] / 2) > 448).all()  # half the scale would overflow e4m3


# ------------------------------------------------------------------------------ append on the CPU
@pytest.mark.parametrize("D,G", [(64, 1), (128, 2)])
def test_append_reference_path(D, G):
    Hq, page, num_blocks, T = HK * G, 16, 6, 37
    W = (Hq + 2 * HK) * D
    g = torch.Generator().manual_seed(D + G)
    x = magnitude_rows(D, seed=3)
    qkv = torch.randn(T, W, generator=g).bfloat16()
    heads = qkv[:, Hq * D:].view(T, 2 * HK, D)
    pick = torch.randint(x.shape[0], (T, 2 * HK), generator=g)
    heads[:] = x[pick]
    slots = torch.randperm(num_blocks * page, generator=g)[:T].to(torch.int32)
    slots[[0, 5, T - 1]] = -1
    k8, v8, ks, vs = poisoned_cache(num_blocks, page, D)
    ops.kv_cache_append_(k8, v8, qkv, slots, Hq, HK, D, k_scale=ks, v_scale=vs)
    kb, vb = k8.view(torch.uint8).view(-1, HK, D), v8.view(torch.uint8).view(-1, HK, D)
    written = torch.zeros(num_blocks * page, dtype=torch.bool)
    for t in range(T):
        sl = int(slots[t])
        if sl < 0:
            continue
        written[sl] = True
        for h in range(HK):
            for xb, xs, row in ((kb, ks, heads[t, h]), (vb, vs, heads[t, HK + h])):
                q, s = ref.kv_quantize_fp8_ref(row)
                assert torch.equal(xb[sl, h], q.view(torch.uint8)) and xs.view(-1, HK)[sl, h] == s
    assert int(written.sum()) == T - 3
    assert (kb[~written] == POISON).all() and (vb[~written] == POISON).all()
    assert torch.isnan(ks.view(-1, HK)[~written]).all() and torch.isnan(vs.view(-1, HK)[~written]).all()


# ------------------------------------------------------------- decode / extend on the CPU
@pytest.mark.parametrize("page,D,G", [(16, 64, 1), (48, 128, 4), (16, 96, 2)])
def test_decode_reference_equals_the_dequantised_bf16_cache(page, D, G):
    c = dec_case(page, D, G)
    lens = torch.tensor(c["lens"], dtype=torch.int32)
    kd, vd = ref.kv_dequantize_fp8_ref(c["k"], c["ks"]), ref.kv_dequantize_fp8_ref(c["v"], c["vs"])
    assert kd.dtype == torch.bfloat16
    want = ops.paged_attention_decode(c["q"], kd, vd, c["table"], lens, c["Hq"], HK, D)
    got = run_decode(c, "cpu")
    assert torch.equal(got, want)
    _check_rows(got, dec_want(page, D, G), D, f"cpu decode page={page} D={D} G={G}")
    assert (got[0] == 0).all()


@pytest.mark.parametrize("D,G", [(64, 4), (128, 1)])
def test_extend_reference_equals_the_dequantised_bf16_cache(D, G):
    c = ext_case(D, G)
    kd, vd = ref.kv_dequantize_fp8_ref(c["k"], c["ks"]), ref.kv_dequantize_fp8_ref(c["v"], c["vs"])
    want = ops.paged_attention_extend(c["q"], kd, vd, c["table"], c["lens"], c["cu"], c["max_q"], c["Hq"], HK, D)
    got = run_extend(c, "cpu")
    assert torch.equal(got, want)
    _check_rows(got, ext_want(D, G), D, f"cpu extend D={D} G={G}")


# -------------------------------------------------------------------- guards of the GPU cases
def _moved(want, wrong, D, groups):
    """Per group of rows (a sequence), the largest row error of ``wrong`` against ``want``."""
    err = _row_err(wrong, want, D)
    return [err[a:b].max().item() for a, b in groups if b > a]


@pytest.mark.parametrize("variant", VARIANTS)
def test_decode_cases_are_scale_sensitive(variant):
    for page, D, G in itertools.product(DEC_PAGES, DEC_DS, DEC_GS):
        lens = dec_lens(page)
        groups = [(b, b + 1) for b, n in enumerate(lens) if n > 0]
        moved = _moved(dec_want(page, D, G), dec_want(page, D, G, variant), D, groups)
        assert len(moved) == len(lens) - 1
        assert min(moved) >= 2 * ROW_BOUND, (page, D, G, variant, moved)


@pytest.mark.parametrize("variant", VARIANTS)
def test_extend_cases_are_scale_sensitive(variant):
    for D, G in itertools.product(EXT_DS, EXT_GS):
        cu = ext_case(D, G)["cu"].tolist()
        moved = _moved(ext_want(D, G), ext_want(D, G, variant), D, list(zip(cu[:-1], cu[1:])))
        assert len(moved) == len(EXT_SEQS)
        assert min(moved) >= 2 * ROW_BOUND, (D, G, variant, moved)


def test_case_scales_differ_inside_a_token():
    c = dec_case(16, 128, 4)
    live = ~torch.isnan(c["ks"].view(-1, HK)[:, 0])
    four = torch.cat([c["ks"].view(-1, HK)[live], c["vs"].view(-1, HK)[live]], 1)
    assert live.sum() == sum(c["lens"])
    assert all(len(set(r.tolist())) == 4 for r in four)
    assert len(set(four.flatten().tolist())) >= 10  # and they spread over many binary orders


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    c = dec_case(16, 64, 2)
    lens = torch.tensor(c["lens"], dtype=torch.int32)
    kd, vd = ref.kv_dequantize_fp8_ref(c["k"], c["ks"]), ref.kv_dequantize_fp8_ref(c["v"], c["vs"])

    def dec(k=c["k"], v=c["v"], **kw):
        kw = {**dict(k_scale=c["ks"], v_scale=c["vs"]), **kw}
        return ops.paged_attention_decode(c["q"], k, v, c["table"], lens, c["Hq"], HK, 64, **kw)

    dec()
    e = ext_case(64, 4)
    qkv = torch.zeros(3, (c["Hq"] + 2 * HK) * 64, dtype=torch.bfloat16)
    slots = torch.tensor([0, 1, -1], dtype=torch.int32)
    bad = [dict(k=kd, v=vd),                                            # scales with a bf16 cache
           dict(k_scale=None, v_scale=None),                            # fp8 cache without scales
           dict(v_scale=None), dict(k_scale=None),                      # one scale only
           dict(k_scale=c["ks"][:-1]), dict(v_scale=c["vs"][..., :1]),  # wrong shape
           dict(k_scale=c["ks"].double()), dict(v_scale=c["vs"].half()),  # wrong dtype
           dict(k_scale=c["ks"].transpose(0, 1).contiguous().transpose(0, 1))]  # not contiguous
    for kw in bad:
        with pytest.raises(ValueError):
            dec(**kw)
        with pytest.raises(ValueError):
            a = {**dict(k=c["k"], v=c["v"], k_scale=c["ks"], v_scale=c["vs"]), **kw}
            ops.kv_cache_append_(a.pop("k"), a.pop("v"), qkv, slots, c["Hq"], HK, 64, **a)
    for kw in (dict(k_scale=None, v_scale=None), dict(k_scale=e["ks"][:-1]), dict(v_scale=e["vs"].double())):
        with pytest.raises(ValueError):
            a = {**dict(k_scale=e["ks"], v_scale=e["vs"]), **kw}
            ops.paged_attention_extend(e["q"], e["k"], e["v"], e["table"], e["lens"], e["cu"], e["max_q"], e["Hq"], HK,
                                       64, **a)
    with pytest.raises(ValueError):
        dec(k=c["k"].view(torch.uint8), v=c["v"].view(torch.uint8))  # bytes are not an fp8 cache
    # any float q over an fp8 cache on the reference path
    assert ops.paged_attention_decode(c["q"].float(), c["k"], c["v"], c["table"], lens, c["Hq"], HK, 64,
                                      k_scale=c["ks"], v_scale=c["vs"]).dtype == torch.float32
    assert ops.paged_kv_fp8_supported(16, 128, 32, 8) and not ops.paged_kv_fp8_supported(24, 128, 32, 8)
    assert not ops.paged_kv_fp8_supported(16, 96, 32, 8)


# ------------------------------------------------------------------------------- PagedKVCache
class _Cfg:
    num_layers, num_kv_heads, head_dim = 3, HK, 128


def test_paged_kv_cache_fp8():
    cache = PagedKVCache(_Cfg, num_blocks=6, page_size=16, kv_dtype="fp8")
    assert cache.fp8 and len(cache.k) == len(cache.v) == len(cache.k_scale) == len(cache.v_scale) == 3
    for k, s in zip(cache.k + cache.v, cache.k_scale + cache.v_scale):
        assert k.dtype == FP8 and tuple(k.shape) == (6, 16, HK, 128)
        assert s.dtype == torch.float32 and tuple(s.shape) == (6, 16, HK)
    assert cache.scales(1)[0] is cache.k_scale[1] and cache.scales(1)[1] is cache.v_scale[1]
    assert PagedKVCache(_Cfg, 6, kv_dtype=FP8).fp8
    for auto in (None, "auto"):
        plain = PagedKVCache(_Cfg, 6, kv_dtype=auto)
        assert not plain.fp8 and plain.k_scale is None and plain.v_scale is None and plain.k[0].dtype == torch.bfloat16
        assert plain.scales(0) == (None, None)
    with pytest.raises(ValueError):
        PagedKVCache(_Cfg, 6, kv_dtype="e5m2")
    bf16 = PagedKVCache.block_bytes(_Cfg, 16, torch.bfloat16, None)
    fp8 = PagedKVCache.block_bytes(_Cfg, 16, torch.bfloat16, "fp8")
    assert bf16 == 2 * 3 * 16 * HK * 128 * 2 and fp8 * 2 * 128 == bf16 * (128 + 4)  # (D + 4) / 2D, exactly
    assert cache.nbytes == 6 * fp8 and PagedKVCache(_Cfg, 6).nbytes == 6 * bf16


def test_fork_shares_pages_and_scales():
    D, Hq = 128, HK * 2
    cache = PagedKVCache(_Cfg, num_blocks=6, page_size=16, kv_dtype="fp8")
    g = torch.Generator().manual_seed(5)

    def feed(seq, n):
        slots = torch.tensor(cache.allocate(seq, n), dtype=torch.int32)
        qkv = torch.randn(n, (Hq + 2 * HK) * D, generator=g).bfloat16()
        for i in range(_Cfg.num_layers):
            ks, vs = cache.scales(i)
            ops.kv_cache_append_(cache.k[i], cache.v[i], qkv, slots, Hq, HK, D, k_scale=ks, v_scale=vs)
        return slots

    parent = feed("p", 40)
    cache.fork("p", "c", 32)
    shared = sorted({int(s) // 16 for s in parent[:32]})
    before = [(t[shared].view(torch.uint8).clone() if t.dtype == FP8 else t[shared].clone())
              for t in cache.k + cache.v + cache.k_scale + cache.v_scale]
    child = feed("c", 20)
    assert not {int(s) // 16 for s in child} & {int(s) // 16 for s in parent}  # the child writes its own pages
    after = [(t[shared].view(torch.uint8) if t.dtype == FP8 else t[shared])
             for t in cache.k + cache.v + cache.k_scale + cache.v_scale]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert cache.block_table(["c"])[0, :2].tolist() == cache.block_table(["p"])[0, :2].tolist()


# ----------------------------------------------------------------------------- llama3-tiny, CPU
LOGIT_SCALE = 8.0
PROMPTS = ((3, 17, 90, 4, 250, 6, 31), tuple(range(100, 140)), tuple([5, 9, 2, 7, 1, 8] * 21 + [5, 9, 2, 7]))
N_NEW = 12
MODES = {"greedy": dict(temperature=0.0, top_p=1.0, seed=0), "sampled": dict(temperature=0.9, top_p=0.9, seed=8)}


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    m = build_llama("llama3-tiny", dtype=torch.float32).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(LOGIT_SCALE)
    return m


@functools.lru_cache(maxsize=None)
def _plain(mode):
    return _model().generate([list(p) for p in PROMPTS], N_NEW, fused_sampling=True, kv_cache_dtype="fp8",
                             **MODES[mode])


def _drain(eng):
    streams = {}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            streams.setdefault(rid, []).append(tok)
    return streams


@pytest.mark.parametrize("mode", sorted(MODES))
def test_generate_equals_engine_with_fp8_cache(mode):
    eng = GenerationEngine(_model(), max_slots=4, num_blocks=64, fused_sampling=True, kv_cache_dtype="fp8")
    assert eng.cache.fp8
    prm = {k: v for k, v in MODES[mode].items()}
    rids = [eng.add_request(list(p), N_NEW, **prm) for p in PROMPTS]
    streams = _drain(eng)
    assert [streams[r] for r in rids] == _plain(mode)
    assert all(len(s) == N_NEW for s in _plain(mode))


def test_generate_uses_a_given_fp8_cache():
    """A cache passed in keeps its own dtype, and its blocks come back."""
    m = _model()
    cache = PagedKVCache(m.cfg, 32, 16, dtype=torch.float32, kv_dtype="fp8")
    out = m.generate([list(PROMPTS[0])], 4, cache=cache)
    assert len(out[0]) == 4 and cache.k[0].dtype == FP8 and cache.num_free_blocks == 32


@pytest.mark.parametrize("mode", sorted(MODES))
def test_speculative_equals_fused_sampling_with_fp8_cache(mode):
    m = _model()
    out = m.generate([list(p) for p in PROMPTS], N_NEW, speculative=3, kv_cache_dtype="fp8", **MODES[mode])
    assert out == _plain(mode)
    assert m.spec_stats["drafted"] > 0


def test_poisoned_dead_slots_do_not_matter():
    m = _model()
    blocks = sum(-(-(len(p) + N_NEW) // 16) for p in PROMPTS) + 2
    cache = PagedKVCache(m.cfg, blocks, 16, dtype=torch.float32, kv_dtype="fp8")
    for t in cache.k + cache.v:
        t.view(torch.uint8).fill_(POISON)
    for t in cache.k_scale + cache.v_scale:
        t.fill_(NAN)
    out = m.generate([list(p) for p in PROMPTS], N_NEW, fused_sampling=True, cache=cache, **MODES["greedy"])
    assert out == _plain("greedy")
    out = m.generate([list(p) for p in PROMPTS], N_NEW, speculative=3, cache=cache, **MODES["sampled"])
    assert out == _plain("sampled")


def test_cache_bytes_sizes_the_engine():
    m = _model()
    per = PagedKVCache.block_bytes(m.cfg, 16, torch.float32, "fp8")
    assert per == 2 * m.cfg.num_layers * 16 * m.cfg.num_kv_heads * (m.cfg.head_dim + 4)
    eng = GenerationEngine(m, cache_bytes=10 * per + per // 2, kv_cache_dtype="fp8")
    assert eng.cache.num_blocks == 10 and eng.cache.nbytes == 10 * per
    wide = PagedKVCache.block_bytes(m.cfg, 16, torch.float32, None)
    assert GenerationEngine(m, cache_bytes=10 * per + per // 2).cache.num_blocks == (10 * per + per // 2) // wide
    assert GenerationEngine(m).cache.num_blocks == 256 and GenerationEngine(m, num_blocks=7).cache.num_blocks == 7
    with pytest.raises(ValueError):
        GenerationEngine(m, num_blocks=8, cache_bytes=10 * per)
    with pytest.raises(ValueError):
        GenerationEngine(m, cache_bytes=per - 1, kv_cache_dtype="fp8")


def test_deployment_reports_the_fp8_cache():
    import asyncio

    from ray_community_amd.serve.llm import _LlamaDeployment

    per = PagedKVCache.block_bytes(_model().cfg, 16, torch.float32, "fp8")
    dep = _LlamaDeployment(dtype="float32", max_slots=2, cache_bytes=12 * per, kv_cache_dtype="fp8")
    st = asyncio.run(dep.status())
    assert st["kv_cache_dtype"] == "fp8" and st["num_blocks"] == 12 and st["cache_bytes"] == 12 * per
    plain = asyncio.run(_LlamaDeployment(dtype="float32", max_slots=2, num_blocks=16).status())
    assert "kv_cache_dtype" not in plain and "cache_bytes" not in plain
