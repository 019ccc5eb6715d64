"""The MFMA paged decode kernel (ops/csrc/attention_decode_mfma.hip: G = 8 opt-in, G = 16) against
the float64 oracle, metric, bound and NaN-poisoned cache layout of
tests/test_attention_decode_edges_gpu.py. ``ROW_BOUND`` = 2**-7 is twice the bf16 rounding floor;
tests/test_attention_extend_gpu.py holds the bf16-P MFMA extend kernel to the same bound. Every kernel
test names ``kernel="mfma"``, which never falls back.
"""
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import build_llama
from ray_community_amd.models.llama import LlamaConfig
from test_attention_decode_edges_gpu import HK, NAN, ROW_BOUND, _check_rows, _oracle, _paged, _row_err
from test_kv_cache_fp8_cpu import _dequant64, dec_case, poisoned_cache
from test_llama_generate import _prompt, _teacher_forced

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(page, D, G, lens=None, width=None):
    """Random K / V of the given lengths in a NaN-poisoned cache, the fused qkv row (q leads), and
    the oracle. Default lengths: every tail of a 16-key tile and of a 32-key step, a step that
    straddles pages, the zero row."""
    lens = list(lens or [0, 1, 15, 16, 17, 31, 32, 33, 5 * page + 3])
    g = torch.Generator().manual_seed(1000 * page + 10 * D + G)
    Ks = [torch.randn(n, HK, D, generator=g).bfloat16() for n in lens]
    Vs = [torch.randn(n, HK, D, generator=g).bfloat16() for n in lens]
    q = torch.randn(len(lens), (HK * G + 2 * HK) * D, generator=g).bfloat16()
    perm = torch.randperm(sum(-(-n // page) for n in lens) + 3, generator=g).tolist()
    k, v, table = _paged(Ks, Vs, page, perm, width)
    want = _oracle(q, k, v, table, lens, HK * G, HK, D, D ** -0.5)
    return dict(q=q, k=k, v=v, table=table, lens=lens, Hq=HK * G, D=D, want=want)


def _run(c, rows=slice(None), **kw):
    lens = torch.tensor(c["lens"], dtype=torch.int32)[rows]
    t = [x.cuda() for x in (c["q"][rows], c["k"], c["v"], c["table"][rows], lens)]
    return ops.paged_attention_decode(*t, c["Hq"], HK, c["D"], **kw).cpu()


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("page", [16, 48])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [8, 16])
def test_per_row(G, D, page, num_splits):
    c = _case(page, D, G)
    out = _run(c, kernel="mfma", num_splits=num_splits)
    _check_rows(out, c["want"], D, f"mfma G={G} D={D} page={page} splits={num_splits}")
    assert (out[0] == 0).all()


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("G", [8, 16])
def test_fp8_cache(G, num_splits):
    """Caches written by the quantising append kernel; the oracle runs over byte x scale."""
    D, page = 128, 16
    c = dec_case(page, D, G)  # K / V with a power-of-two factor per (token, kv head), block table, q
    Hq, dev = HK * G, "cuda"
    k8, v8, ks, vs = poisoned_cache(c["k"].shape[0], page, D, dev)
    for b, n in enumerate(c["lens"]):
        if n:
            slots = torch.tensor([int(c["table"][b, i // page]) * page + i % page for i in range(n)], dtype=torch.int32)
            rows = torch.cat([torch.zeros(n, Hq * D, dtype=torch.bfloat16), c["Ks"][b].reshape(n, -1),
                              c["Vs"][b].reshape(n, -1)], 1)
            ops.kv_cache_append_(k8, v8, rows.to(dev), slots.to(dev), Hq, HK, D, k_scale=ks, v_scale=vs)
    lens = torch.tensor(c["lens"], dtype=torch.int32)
    out = ops.paged_attention_decode(c["q"].to(dev), k8, v8, c["table"].to(dev), lens.to(dev), Hq, HK, D, k_scale=ks,
                                     v_scale=vs, kernel="mfma", num_splits=num_splits).cpu()
    want = _oracle(c["q"], _dequant64(k8.cpu(), ks.cpu()), _dequant64(v8.cpu(), vs.cpu()), c["table"], c["lens"], Hq, HK,
                   D, D ** -0.5)
    _check_rows(out, want, D, f"mfma fp8 G={G} splits={num_splits}")
    assert c["lens"][0] == 0 and (out[0] == 0).all()


@pytest.mark.parametrize("num_splits", [1, 4])
def test_a_sequence_alone_equals_its_batched_row(num_splits):
    lens = (40, 7, 0, 215, 64)
    batched = _run(_case(16, 128, 16, lens, 24), kernel="mfma", num_splits=num_splits)
    c = _case(16, 128, 16, lens)  # the same seed and data, the table as narrow as it can be
    assert c["table"].shape[1] == 14
    alone = _run(c, rows=slice(3, 4), kernel="mfma", num_splits=num_splits)
    assert torch.equal(alone[0], batched[3]) and alone.abs().max() > 0


def test_auto_dispatch(monkeypatch):
    assert ops.paged_decode_supported(16, 128, 32, 2) and ops.paged_kv_fp8_supported(16, 128, 32, 2)
    c16, c8 = _case(16, 128, 16), _case(16, 128, 8)
    monkeypatch.delenv("RCA_ATTN_DECODE", raising=False)
    assert torch.equal(_run(c16), _run(c16, kernel="mfma"))
    assert torch.equal(_run(c8), _run(c8, kernel="valu"))
    monkeypatch.setenv("RCA_ATTN_DECODE", "mfma")
    assert torch.equal(_run(c8), _run(c8, kernel="mfma"))


def test_extend_and_fused_append_at_g16():
    """The neighbours of the decode that G = 16 newly reaches on the kernel path."""
    page, D, G = 16, 128, 16
    c = _case(page, D, G)
    Hq, B, dev = HK * G, len(c["lens"]), "cuda"
    lens = torch.tensor(c["lens"], dtype=torch.int32, device=dev)
    t = [x.to(dev) for x in (c["q"], c["k"], c["v"], c["table"])]
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev)
    ext = ops.paged_attention_extend(*t, lens, cu, 1, Hq, HK, D).cpu()
    _check_rows(ext, c["want"], D, "extend G=16, one row per sequence")
    assert _row_err(ext, _run(c, kernel="mfma").double(), D).max().item() < 2 * ROW_BOUND
    # fused RoPE + append against the two ops, bit for bit, on the live rows (length >= 1)
    cs = ops.rope_cos_sin(256, D, 500000.0).to(dev)
    pos = (lens - 1).clamp_min(0)
    slots = torch.where(lens > 0, t[3].gather(1, (pos // page)[:, None].long())[:, 0] * page + pos % page,
                        torch.full_like(pos, -1))
    a = [torch.full_like(t[1], NAN), torch.full_like(t[2], NAN), t[0].clone()]
    f = [x.clone() for x in a]
    rot = ops.apply_rope_(a[2].clone(), cs, 1, Hq, HK, D, pos)
    a[2] = torch.where((lens > 0)[:, None], rot, a[2])
    ops.kv_cache_append_(a[0], a[1], a[2], slots, Hq, HK, D)
    ops.rope_kv_append_decode_(f[2], cs, f[0], f[1], t[3], lens, Hq, HK, D)
    for x, y in zip(a, f):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    assert not torch.isnan(f[0]).all()


def test_refusals():
    c4, c16 = _case(16, 128, 4), _case(16, 128, 16)
    lens = torch.tensor(c16["lens"], dtype=torch.int32)
    with pytest.raises(ValueError):
        _run(c4, kernel="mfma")
    with pytest.raises(ValueError):
        _run(c16, kernel="valu")
    with pytest.raises(ValueError):
        _run(c16, kernel="tensor")
    with pytest.raises(ValueError):  # CPU tensors: the reference path
        ops.paged_attention_decode(c16["q"], c16["k"], c16["v"], c16["table"], lens, 32, HK, 128, kernel="mfma")
    with pytest.raises(ValueError):  # fp32 q
        ops.paged_attention_decode(c16["q"].float().cuda(), c16["k"].cuda(), c16["v"].cuda(), c16["table"].cuda(),
                                   lens.cuda(), 32, HK, 128, kernel="mfma")
    t = [x.cuda() for x in (c4["q"], c4["k"], c4["v"], c4["table"], torch.tensor(c4["lens"], dtype=torch.int32))]
    out = torch.full((len(c4["lens"]), 8 * 128), 7.0, dtype=torch.bfloat16, device="cuda")
    rc = ops.lib().rca_attn_decode_paged_mfma(t[0].data_ptr(), t[0].stride(0), t[1].data_ptr(), t[2].data_ptr(), None,
                                              None, t[3].data_ptr(), t[4].data_ptr(), out.data_ptr(), None, None,
                                              len(c4["lens"]), 8, HK, 128, 16, t[3].shape[1], t[1].shape[0],
                                              128 ** -0.5, 1, None)
    torch.cuda.synchronize()
    assert rc == -1 and (out == 7.0).all()


def test_llama_with_16_heads_per_kv_head():
    """bf16 model on the GPU against its fp32 twin on the reference path, teacher-forced, under the
    criterion of tests/test_llama_generate.py::test_cached_path_on_gpu_is_as_accurate_as_full_forward."""
    cfg = LlamaConfig(vocab_size=1024, hidden_size=1024, intermediate_size=512, num_layers=2, num_heads=16,
                      num_kv_heads=1, max_seq_len=256, name="g16-tiny")
    assert cfg.head_dim == 64 and ops.paged_decode_supported(16, 64, 16, 1)
    torch.manual_seed(0)
    m = build_llama(cfg, device="cuda", dtype=torch.bfloat16).eval()
    ref_model = build_llama(cfg, dtype=torch.float32).eval()
    ref_model.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    cached, want, own = _teacher_forced(m, ref_model, "cuda")
    scale = want.abs().max().item()
    e_cached, e_full = (cached - want).abs().max().item(), (own - want).abs().max().item()
    print(f"cached err {e_cached:.3e}, full bf16 forward err {e_full:.3e}, max |logit| {scale:.3e}")
    assert torch.isfinite(cached).all()
    assert e_cached <= 2 * e_full + 1e-3 * scale
    prompts = [_prompt(5, 1), _prompt(130, 3)]
    assert m.generate(prompts, 6, graph_decode=True) == m.generate(prompts, 6)
