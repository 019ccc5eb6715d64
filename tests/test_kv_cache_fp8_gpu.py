"""The gfx950 FP8 KV-cache kernels (ops/csrc/attention_decode_fp8.hip: quantising append and
decode; ops/csrc/attention_extend_fp8.hip: extend) on the cases, oracle, metric and bound of
tests/test_kv_cache_fp8_cpu.py, whose CPU tests guard the data (scale-sensitive, poisoned dead
slots, permuted block tables).

The append is compared exactly: kernel and CPU reference both round the same exact fp32 quotient
to nearest-even e4m3. Decode and extend are compared per (sequence or token, head) row with the
float64 oracle of the dequantised cache under ``ROW_BOUND`` = 2**-7, the bf16 kernels' bound.
"""
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, build_llama
from ray_community_amd.models.kv_cache import PagedKVCache
from ray_community_amd.ops import reference as ref
from test_kv_cache_fp8_cpu import (DEC_DS, DEC_GS, DEC_PAGES, EXT_DS, EXT_GS, EXT_PAGE, FP8, HK, NAN, POISON, _attend,
                                   _check_rows, _scaled_kv, dec_case, dec_want, ext_case, ext_want, magnitude_rows,
                                   poisoned_cache, run_decode, run_extend)

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------- append
@gpu
@pytest.mark.parametrize("T", [1, 37, 300])
@pytest.mark.parametrize("D,G", [(64, 1), (64, 8), (128, 2)])
def test_quantising_append_is_exact(D, G, T):
    Hq, page, num_blocks = HK * G, 16, 24
    W = (Hq + 2 * HK) * D
    g = torch.Generator().manual_seed(1000 * D + 10 * G + T)
    wide = torch.randn(T, W + 64, generator=g).bfloat16()
    x = magnitude_rows(D, seed=T)  # 2^-120 .. 300, zero rows, amax = 448 * 2^k and just above
    heads = wide[:, 32 + Hq * D: 32 + W].view(T, 2 * HK, D)
    heads[:] = x[torch.randint(x.shape[0], (T, 2 * HK), generator=g)]
    slots = torch.randperm(num_blocks * page, generator=g)[:T].to(torch.int32)  # out of order, distinct
    if T > 1:
        slots[[0, 5, T - 1]] = -1
    qkv_cpu = wide[:, 32: 32 + W]

    want = poisoned_cache(num_blocks, page, D)
    ref.kv_cache_append_ref(want[0], want[1], qkv_cpu, slots, Hq, HK, D, want[2], want[3])

    qkv = wide.cuda()[:, 32: 32 + W]
    # the conditions under which ops.kv_cache_append_ takes the kernel and not the reference
    assert qkv.is_cuda and qkv.dtype == torch.bfloat16 and ops.paged_kv_fp8_supported(page, D, Hq, HK)
    assert qkv.stride(1) == 1 and qkv.stride(0) == W + 64 and qkv.data_ptr() % 16 == 0
    got = poisoned_cache(num_blocks, page, D, "cuda")
    ops.kv_cache_append_(got[0], got[1], qkv, slots.cuda(), Hq, HK, D, k_scale=got[2], v_scale=got[3])
    torch.cuda.synchronize()
    written = torch.zeros(num_blocks * page, dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    assert int(written.sum()) == T - (3 if T > 1 else 0)
    for name, w, o in zip(("k", "v"), want[:2], got[:2]):
        wb, ob = w.view(torch.uint8).view(-1, HK * D), o.cpu().view(torch.uint8).view(-1, HK * D)
        assert torch.equal(ob[written], wb[written]), f"{name} bytes of live slots"
        assert (ob[~written] == POISON).all(), f"{name} bytes of untouched slots"
    for name, w, o in zip(("k_scale", "v_scale"), want[2:], got[2:]):
        ws, os_ = w.view(-1, HK), o.cpu().view(-1, HK)
        assert torch.equal(os_[written], ws[written]), f"{name} of live slots"
        assert torch.isnan(os_[~written]).all(), f"{name} of untouched slots"
        assert not torch.isnan(os_[written]).any()


# ---------------------------------------------------------------------------------------- decode
@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("G", DEC_GS)
@pytest.mark.parametrize("D", DEC_DS)
@pytest.mark.parametrize("page", DEC_PAGES)
def test_decode_per_row(page, D, G, num_splits):
    c = dec_case(page, D, G)
    assert ops.paged_kv_fp8_supported(page, D, c["Hq"], HK)  # the kernel, not the reference
    out = run_decode(c, "cuda", num_splits=num_splits)
    _check_rows(out, dec_want(page, D, G), D, f"fp8 decode page={page} D={D} G={G} splits={num_splits}")
    assert c["lens"][0] == 0 and (out[0] == 0).all()


@gpu
@pytest.mark.parametrize("step", [16, 32])
@pytest.mark.parametrize("page,D,G", [(16, 128, 4), (48, 64, 2), (48, 128, 1)])
def test_decode_both_step_sizes(page, D, G, step):
    """The 16-token step is a measurement knob (32 is the default); both must be right."""
    c = dec_case(page, D, G)
    assert ops.lib().rca_attn_decode_fp8_set_step(step) == 0
    try:
        for num_splits in (1, 3):
            _check_rows(run_decode(c, "cuda", num_splits=num_splits), dec_want(page, D, G), D,
                        f"fp8 decode step={step} page={page} D={D} G={G} splits={num_splits}")
    finally:
        assert ops.lib().rca_attn_decode_fp8_set_step(32) == 0
    assert ops.lib().rca_attn_decode_fp8_set_step(24) != 0


@gpu
@pytest.mark.parametrize("page,D,G", [(16, 128, 4), (48, 64, 8)])
def test_decode_default_splits_and_a_sequence_alone(page, D, G):
    c = dec_case(page, D, G)
    _check_rows(run_decode(c, "cuda", num_splits=None), dec_want(page, D, G), D, f"fp8 decode default splits {page} {D} {G}")
    for num_splits in (1, 3):
        batched = run_decode(c, "cuda", num_splits=num_splits)
        for b, n in enumerate(c["lens"]):
            alone = run_decode(dict(c, q=c["q"][b: b + 1], table=c["table"][b: b + 1], lens=[n]), "cuda",
                               num_splits=num_splits)
            assert torch.equal(alone[0], batched[b]), f"sequence {b} (length {n}), {num_splits} splits"


# ---------------------------------------------------------------------------------------- extend
@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("G", EXT_GS)
@pytest.mark.parametrize("D", EXT_DS)
def test_extend_per_row(D, G, num_splits):
    c = ext_case(D, G)
    assert ops.paged_kv_fp8_supported(EXT_PAGE, D, c["Hq"], HK)
    out = run_extend(c, "cuda", num_splits=num_splits)
    _check_rows(out, ext_want(D, G), D, f"fp8 extend D={D} G={G} splits={num_splits}")


# ------------------------------------------------------------ append, then decode, then extend
class _Cfg:
    num_layers, num_kv_heads, head_dim = 1, HK, 128


RT_LENS = [1, 33, 80]
RT_CHUNKS = [(0, 1), (1, 7), (2, 20), (1, 16), (2, 30), (1, 10), (2, 30)]  # (sequence, tokens), interleaved
RT_EXT = [3, 5, 17]  # then each sequence grows by a chunk that attends through extend


@functools.lru_cache(maxsize=None)
def _round_trip_data():
    """Originals, and the float64 oracles over their CPU-quantised, dequantised values."""
    G, D = 4, _Cfg.head_dim
    Hq = HK * G
    g = torch.Generator().manual_seed(10)
    kv = [_scaled_kv(n + e, D, g) for n, e in zip(RT_LENS, RT_EXT)]
    q_dec = torch.randn(len(RT_LENS), Hq * D, generator=g).bfloat16()
    q_ext = [torch.randn(e, Hq * D, generator=g).bfloat16() for e in RT_EXT]
    deq = []
    for k, v in kv:
        (k8, ks), (v8, vs) = ref.kv_quantize_fp8_ref(k), ref.kv_quantize_fp8_ref(v)
        deq.append((k8.double() * ks.double()[..., None], v8.double() * vs.double()[..., None]))
    scale = D ** -0.5
    want_dec = torch.stack([_attend(q_dec[b].double().reshape(Hq, D), k[:n], v[:n], G, scale)
                            for b, ((k, v), n) in enumerate(zip(deq, RT_LENS))]).reshape(len(RT_LENS), -1)
    want_ext = torch.cat([torch.stack([_attend(q_ext[b][i].double().reshape(Hq, D), k[: n + i + 1], v[: n + i + 1], G, scale)
                                       for i in range(e)]).reshape(e, -1)
                          for b, ((k, v), n, e) in enumerate(zip(deq, RT_LENS, RT_EXT))])
    return G, D, kv, q_dec, q_ext, want_dec, want_ext


@gpu
def test_append_decode_extend_round_trip():
    G, D, kv, q_dec, q_ext, want_dec, want_ext = _round_trip_data()
    Hq, dev = HK * G, "cuda"
    cache = PagedKVCache(_Cfg, num_blocks=14, page_size=16, device=dev, kv_dtype="fp8")
    cache.k[0].view(torch.uint8).fill_(POISON)
    cache.v[0].view(torch.uint8).fill_(POISON)
    cache.k_scale[0].fill_(NAN)
    cache.v_scale[0].fill_(NAN)
    ks, vs = cache.scales(0)

    def append(s, lo, hi, q_rows=None):
        slots = torch.tensor(cache.allocate(s, hi - lo), dtype=torch.int32, device=dev)
        q_rows = torch.full((hi - lo, Hq * D), NAN, dtype=torch.bfloat16) if q_rows is None else q_rows
        rows = torch.cat([q_rows, kv[s][0][lo:hi].reshape(hi - lo, -1), kv[s][1][lo:hi].reshape(hi - lo, -1)], 1)
        rows = rows.to(dev)
        ops.kv_cache_append_(cache.k[0], cache.v[0], rows, slots, Hq, HK, D, k_scale=ks, v_scale=vs)
        return rows

    done = [0] * len(RT_LENS)
    for s, t in RT_CHUNKS:
        append(s, done[s], done[s] + t)
        done[s] += t
    assert done == RT_LENS
    ids = list(range(len(RT_LENS)))
    out = ops.paged_attention_decode(q_dec.to(dev), cache.k[0], cache.v[0], cache.block_table(ids),
                                     cache.context_lens(ids), Hq, HK, D, k_scale=ks, v_scale=vs)
    _check_rows(out.cpu(), want_dec, D, "fp8 round trip, decode")
    fused = torch.cat([append(s, n, n + e, q_ext[s]) for s, (n, e) in enumerate(zip(RT_LENS, RT_EXT))])
    cu = torch.tensor([0, 3, 8, 25], dtype=torch.int32, device=dev)
    for num_splits in (1, 2):
        out = ops.paged_attention_extend(fused, cache.k[0], cache.v[0], cache.block_table(ids), cache.context_lens(ids),
                                         cu, max(RT_EXT), Hq, HK, D, num_splits=num_splits, k_scale=ks, v_scale=vs)
        _check_rows(out.cpu(), want_ext, D, f"fp8 round trip, extend, {num_splits} split(s)")


# ---------------------------------------------------------------------------- llama3-tiny, GPU
@gpu
def test_llama_tiny_generates_over_an_fp8_cache():
    torch.manual_seed(0)
    m = build_llama("llama3-tiny", device="cuda", dtype=torch.bfloat16).eval()
    cfg = m.cfg
    assert ops.paged_kv_fp8_supported(16, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 1024, (n,), generator=g).tolist() for n in (5, 40, 130)]
    cache = PagedKVCache(cfg, 32, 16, device="cuda", kv_dtype="fp8")
    logits = m.prefill(prompts, None, cache, ["a", "b", "c"])
    logits2 = m.decode_step(logits.argmax(-1), cache, ["a", "b", "c"])
    logits3 = m.extend([[1, 2, 3], [4, 5], [6]], cache, ["a", "b", "c"], num_splits=None)
    assert all(torch.isfinite(x).all() for x in (logits, logits2, logits3))
    assert cache.k[0].dtype == FP8 and torch.isfinite(cache.k_scale[0].view(-1, cfg.num_kv_heads)[:5]).all()
    out = m.generate(prompts, 6, kv_cache_dtype="fp8")
    eng = GenerationEngine(m, max_slots=4, num_blocks=32, kv_cache_dtype="fp8")
    rids = [eng.add_request(list(p), 6) for p in prompts]
    streams = {}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            streams.setdefault(rid, []).append(tok)
    assert [streams[r] for r in rids] == out and all(len(s) == 6 for s in out)
