"""The shared AdamW layer (``parallel/optim.py``): the one-range update primitive, and the flat
and ZeRO optimizers built on it agreeing when fed the same gradients at world 1."""
import pytest
import torch


def _hp(step=1, clip=0.0, coef=1.0, grad_scale=1.0):
    from ray_community_amd.parallel.optim import AdamWStep

    return AdamWStep(1e-2, 0.9, 0.95, 1e-8, 1 - 0.9 ** step, 1 - 0.95 ** step, step, grad_scale, clip,
                     torch.zeros(1), coef)


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("dtype,fmt", [(torch.float32, "auto"), (torch.bfloat16, "fp32"), (torch.bfloat16, "split")],
                         ids=["fp32_model", "bf16_fp32_master", "bf16_split_master"])
def test_flat_adamw_matches_sharded_adamw_world1(dtype, fmt, clip):
    """Same fed gradients, three steps: whole-buffer ranges (flat) against per-bucket chunks
    (ZeRO at world 1). Without clipping every element sees the same arithmetic: bitwise. With
    clipping only the summation order of the norm differs (whole buffer vs chunk list), a
    relative 1e-7 on the coefficient: the tolerances of ``test_world1_matches_flat_adamw`` (fp32
    values) and of ``test_sharded_adamw_matches_flat_adamw_gpu`` (bf16 weights, one rounding)."""
    from ray_community_amd.models import build_llama
    from ray_community_amd.parallel import DistributedDataParallel, FlatAdamW, ShardedAdamW, ShardedDataParallel

    torch.manual_seed(0)
    w1 = DistributedDataParallel(build_llama("llama3-tiny", dtype=dtype), bucket_cap_mb=0.2)
    torch.manual_seed(0)
    w2 = ShardedDataParallel(build_llama("llama3-tiny", dtype=dtype), bucket_cap_mb=0.2)
    assert w1.flat.offsets == w2.flat.offsets and len(w2.flat.buckets) > 2
    o1 = FlatAdamW(w1.flat, lr=1e-3, max_grad_norm=clip, master_format=fmt)
    o2 = ShardedAdamW(w2, lr=1e-3, max_grad_norm=clip, master_format=fmt)
    assert o1.split_master == o2.split_master == (fmt == "split")
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        grad = (torch.randn(w1.flat.numel, generator=gen) * 0.01).to(dtype)
        w1.flat.grad.copy_(grad)
        w2.flat.grad.copy_(grad)
        o1.step(0.5)
        o2.step(0.5)
    assert o1.step_count == o2.step_count == 3

    def same(a, b, what, bf16=False):
        if clip is None:
            assert torch.equal(a, b), what
        elif bf16:
            a, b = a.float(), b.float()
            assert torch.allclose(a, b, atol=1e-5, rtol=8e-3), (what, (a - b).abs().max())
        else:
            assert torch.allclose(a, b, atol=2e-5, rtol=1e-4), (what, (a - b).abs().max())

    if clip is not None:
        assert o1.grad_norm() > clip  # the clip is active
        assert o2.grad_norm() == pytest.approx(o1.grad_norm(), rel=1e-5)
    same(w1.flat.data, w2.flat.data, "weights", bf16=dtype == torch.bfloat16)
    m1, m2 = o1.master, o2.master
    for bi, s, e, o, _ in o2.chunks:
        n = e - s
        same(o1.m[s:e], o2.m[o: o + n], ("m", bi))
        same(o1.v[s:e], o2.v[o: o + n], ("v", bi))
        if o1.master_weights:  # an fp32 model is its own master
            same(m1[s:e], m2[o: o + n], ("master", bi))


@pytest.mark.parametrize("fmt", ["inplace", "fp32", "split"])
def test_update_primitive_cpu_is_the_reference(fmt):
    from ray_community_amd.ops import reference as ref
    from ray_community_amd.parallel.optim import adamw_update_

    torch.manual_seed(3)
    n = 200
    p0 = torch.randn(n)
    g = (torch.randn(n) * 0.1).to(torch.float32 if fmt == "inplace" else torch.bfloat16)
    hp = _hp(step=2, clip=0.5, coef=0.25, grad_scale=0.5)
    m, v = torch.rand(n), torch.rand(n)
    pr, mr, vr = p0.clone(), m.clone(), v.clone()
    if fmt == "split":
        w, lo = ref.split_master(p0)
        pr = ref.join_master(w, lo)
        adamw_update_(w, g, m, v, hp, 0.1, lo=lo)
        got = ref.join_master(w, lo)
    elif fmt == "fp32":
        w, master = p0.to(torch.bfloat16), p0.clone()
        adamw_update_(w, g, m, v, hp, 0.1, master=master)
        got = master
        assert torch.equal(w, master.to(torch.bfloat16))
    else:
        got = p0.clone()
        adamw_update_(got, g, m, v, hp, 0.1)
    ref.adamw_ref(pr, g, mr, vr, hp.lr, hp.b1, hp.b2, hp.eps, 0.1, hp.step, grad_mul=0.5, clip=0.25)
    assert torch.equal(got, pr) and torch.equal(m, mr) and torch.equal(v, vr)


def test_update_primitive_empty_range_is_a_noop(monkeypatch):
    from ray_community_amd.parallel import optim

    def no_lib():
        raise AssertionError("the kernel library is not needed for an empty range")

    monkeypatch.setattr(optim, "lib", no_lib)
    monkeypatch.setattr(optim.ops.reference, "adamw_ref", lambda *a, **k: no_lib())
    e = torch.zeros(0)
    w, lo = torch.zeros(0, dtype=torch.bfloat16), torch.zeros(0, dtype=torch.int16)
    assert optim.adamw_update_(e, e, e, e, _hp(), 0.1) is None
    assert optim.adamw_update_(w, w, e, e, _hp(), 0.1, master=e) is None
    assert optim.adamw_update_(w, w, e, e, _hp(), 0.1, lo=lo) is None


def test_update_primitive_rejects_views_of_unequal_length():
    from ray_community_amd.parallel.optim import adamw_update_

    w, g, m, v = torch.zeros(8), torch.zeros(8), torch.zeros(8), torch.zeros(16)[12:20]  # cut short: 4
    with pytest.raises(ValueError, match="equal length"):
        adamw_update_(w, g, m, v, _hp(), 0.1)
    assert not m.any()


@pytest.mark.gpu
def test_update_primitive_rejects_unsupported_grad_dtype_gpu():
    from ray_community_amd.parallel.optim import adamw_update_

    dev = "cuda:0"
    w, m, v = (torch.zeros(64, device=dev) for _ in range(3))
    g = torch.zeros(64, dtype=torch.float16, device=dev)
    with pytest.raises(TypeError, match="unsupported grad dtype torch.float16"):
        adamw_update_(w, g, m, v, _hp()._replace(sumsq=torch.zeros(1, device=dev)), 0.1)
    assert not w.any() and not m.any() and not v.any()
