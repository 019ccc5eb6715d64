"""gfx950 paged decode attention and KV-cache append (ops/csrc/attention_decode.hip) vs the fp32
PyTorch references. Error metric and forward bound are those of tests/test_attention_gpu.py."""
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BOUND = 2e-2
ROW_BOUND = 2.0 ** -7  # twice the bf16 rounding floor of a row
HK = 2


def _err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@functools.lru_cache(maxsize=None)
def _case(page, D, G, q_mul=1.0):
    """B = 6 sequences of lengths [0, 1, page-1, page, page+1, 5*page+3] over caches that are NaN
    everywhere except the live slots, with physical blocks in a random permutation. Returns the
    fused qkv rows (q leads), caches, block table, lengths and the fp32 reference (computed once)."""
    Hq = HK * G
    lens = [0, 1, page - 1, page, page + 1, 5 * page + 3]
    B = len(lens)
    need = [-(-n // page) for n in lens]
    num_blocks = sum(need) + 5
    g = torch.Generator().manual_seed(1000 * page + 10 * D + G)
    perm = torch.randperm(num_blocks, generator=g).tolist()
    table = torch.zeros(B, max(need), dtype=torch.int32)
    k_cache = torch.full((num_blocks, page, HK, D), float("nan"), dtype=torch.bfloat16)
    v_cache = torch.full((num_blocks, page, HK, D), float("nan"), dtype=torch.bfloat16)
    nxt = 0
    for b, n in enumerate(lens):
        blocks = perm[nxt: nxt + need[b]]
        nxt += need[b]
        table[b, : need[b]] = torch.tensor(blocks, dtype=torch.int32)
        for i in range(n):
            k_cache[blocks[i // page], i % page] = torch.randn(HK, D, generator=g).bfloat16()
            v_cache[blocks[i // page], i % page] = torch.randn(HK, D, generator=g).bfloat16()
    qkv = torch.randn(B, (Hq + 2 * HK) * D, generator=g)
    qkv[:, : Hq * D] *= q_mul
    c = dict(Hq=Hq, D=D, lens=lens, qkv=qkv.bfloat16().cuda(), k=k_cache.cuda(), v=v_cache.cuda(),
             table=table.cuda(), cl=torch.tensor(lens, dtype=torch.int32).cuda())
    c["ref"] = ref.paged_attention_decode_ref(c["qkv"].float(), c["k"], c["v"], c["table"], c["cl"], Hq, HK, D)
    assert torch.isfinite(c["ref"]).all()
    return c


def _run(c, q=None, **kw):
    out = ops.paged_attention_decode(c["qkv"] if q is None else q, c["k"], c["v"], c["table"], c["cl"], c["Hq"], HK,
                                     c["D"], **kw)
    torch.cuda.synchronize()
    return out


def _row_err(out, want, D):
    """Per (sequence, head): max_d |out - want| / max_d |want|; all-zero rows of ``want`` give 0
    (as in tests/test_attention_decode_edges_gpu.py, where ROW_BOUND is derived)."""
    a, b = out.double().reshape(out.shape[0], -1, D), want.double().reshape(want.shape[0], -1, D)
    num, den = (a - b).abs().amax(-1), b.abs().amax(-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))


def _check(out, c):
    assert out.shape == (6, c["Hq"] * c["D"]) and out.dtype == torch.bfloat16
    assert torch.isfinite(out).all()
    e = _err(out, c["ref"])
    print(f"err {e:.3e}")
    assert e < BOUND
    assert (out[0] == 0).all()  # context_len 0: an inactive slot writes zeros
    r = _row_err(out, c["ref"], c["D"]).max().item()  # a long row's error is not hidden by a short row's size
    print(f"row err {r:.3e}")
    assert r < ROW_BOUND


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("page", [16, 64])
def test_decode_matches_fp32_reference(page, D, G):
    assert ops.paged_decode_supported(page, D, HK * G, HK)
    c = _case(page, D, G)
    _check(_run(c), c)


@pytest.mark.parametrize("num_splits", [1, 2, 7, None])
def test_decode_splits(num_splits):
    """7 splits leave some of them empty for the short rows; None is the default policy."""
    c = _case(16, 128, 4)
    a = _run(c, num_splits=num_splits)
    _check(a, c)
    b = _run(c, num_splits=num_splits)
    assert torch.equal(a, b)  # fixed-order merge: bitwise reproducible


@pytest.mark.parametrize("num_splits", [1, 3])
def test_decode_large_logits(num_splits):
    """q scaled by 8: the running max moves across pages and across splits."""
    c = _case(16, 128, 4, 8.0)
    _check(_run(c, num_splits=num_splits), c)


def test_decode_reads_q_in_place():
    c = _case(16, 64, 4)
    q = c["qkv"][:, : c["Hq"] * c["D"]].contiguous()
    assert q.stride(0) != c["qkv"].stride(0)
    assert torch.equal(_run(c), _run(c, q=q))


def test_decode_wrapper_rejects_mismatches():
    c = _case(16, 64, 4)
    with pytest.raises(ValueError):
        ops.paged_attention_decode(c["qkv"], c["k"], c["v"], c["table"].long(), c["cl"], c["Hq"], HK, c["D"])
    with pytest.raises(ValueError):
        ops.paged_attention_decode(c["qkv"], c["k"], c["v"], c["table"], c["cl"][:-1], c["Hq"], HK, c["D"])
    with pytest.raises(ValueError):
        ops.paged_attention_decode(c["qkv"][:, :-8], c["k"], c["v"], c["table"], c["cl"], c["Hq"], HK, c["D"])
    with pytest.raises(ValueError):
        ops.paged_attention_decode(c["qkv"], c["k"], c["v"][:, :, :1], c["table"], c["cl"], c["Hq"], HK, c["D"])


def test_kv_cache_append_matches_reference():
    Hq, D, page, num_blocks, T = 8, 128, 16, 8, 37
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(T, (Hq + 2 * HK) * D, generator=g).bfloat16().cuda()
    slots = torch.randperm(num_blocks * page, generator=g)[:T].to(torch.int32)  # out of order, distinct
    slots[[0, 5, 17, 36]] = -1
    slots = slots.cuda()
    sentinel = torch.full((num_blocks, page, HK, D), -7.0, dtype=torch.bfloat16, device="cuda")
    k, v, kr, vr = (sentinel.clone() for _ in range(4))
    ops.kv_cache_append_(k, v, qkv, slots, Hq, HK, D)
    torch.cuda.synchronize()
    ref.kv_cache_append_ref(kr, vr, qkv, slots, Hq, HK, D)
    assert torch.equal(k, kr) and torch.equal(v, vr)
    written = torch.zeros(num_blocks * page, dtype=torch.bool, device="cuda")
    written[slots[slots >= 0].long()] = True
    assert written.sum().item() == T - 4
    flat = k.view(-1, HK * D)
    assert (flat[~written] == -7.0).all() and (v.view(-1, HK * D)[~written] == -7.0).all()
    assert not (flat[written] == -7.0).all(dim=1).any()
