"""The W8A16 kernel and the dequantiser (ops/csrc/linear_w8.hip) through ``ops.linear_w8`` on the cases,
float64 oracle and bound of tests/test_linear_w8_cpu.py (its CPU tests guard the checker), then quantised
models end to end.

Views: x is ``buf[2 : 2 + M, c0 : c0 + K]`` of a NaN-filled allocation, ``out=`` a view inside a
sentinel-filled allocation that must be bit-identical outside the view, both with the (row stride - cols,
c0) pairs of tests/test_gemm_rows_gpu.py; the weight bytes and the scales are followed by poison (0x7F
bytes = NaN in e4m3, NaN scales) inside larger allocations, so a read past N or K shows.

Worst share of the bound per GPU test, measured on one MI355X (the file's 17 tests take 5 s; the slowest,
the contract test, 0.4 s):
    test_linear_w8_rows_coded                      M=1 0.935  2 0.932  5 0.955  16 0.973  17 0.990  32 0.976  33 0.976
    test_linear_w8_rows_exact_binades_nonfinite    exact: bit for bit; binades 0.979; nonfinite 0.961
    test_rows_do_not_depend_on_the_batch           bit for bit
    test_dequant_kernel_is_exact                   bit for bit
    test_large_m_path_is_inside_the_bound          M=33 0.892 / 0.805   M=300 0.923 / 0.877
The share is set by the rounding term (an element just above a power of two); the fp32 emulation of
tests/test_linear_w8_cpu.py reaches 0.976 on the CPU. The kernel passed every case at its first device run.
"""
import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, QuantLinear, build_llama
from ray_community_amd.ops import reference as ref
from ray_community_amd.ops._lib import lib, stream_ptr
from test_linear_w8_cpu import KINDS, KS, MS, NS, PADS, case, fails, kind_shapes, splits

gpu = pytest.mark.gpu
SLACK = 2


def _sentinel(rows, width):
    idx = torch.arange(rows * width, dtype=torch.int64)
    bits = (idx * 40503 + 0x1234) & 0xFFFF
    return (bits - ((bits >> 15) << 16)).to(torch.int16).view(rows, width)


def _device_operands(c, sel):
    """(x view, q, s, out allocation, out view) on the GPU, padded and poisoned as the docstring says."""
    M, N, K = c["M"], c["N"], c["K"]
    (px, cx), (po, co) = PADS[sel % 3], PADS[(sel + 1) % 3]
    xbuf = torch.full((M + 2 * SLACK, K + px), float("nan"), dtype=torch.bfloat16)
    xbuf[SLACK:SLACK + M, cx:cx + K] = c["x"]
    x = xbuf.cuda()[SLACK:SLACK + M, cx:cx + K]
    qbuf = torch.full((N * K + 4096,), 0x7F, dtype=torch.uint8)
    qbuf[:N * K] = c["q"].view(torch.uint8).reshape(-1)
    q = qbuf.cuda()[:N * K].view(N, K)
    sbuf = torch.full((N + 64,), float("nan"), dtype=torch.float32)
    sbuf[:N] = c["s"]
    s = sbuf.cuda()[:N]
    obuf = _sentinel(M + 2 * SLACK, N + po).view(torch.bfloat16).cuda()
    out = obuf[SLACK:SLACK + M, co:co + N]
    assert x.stride(0) == K + px and out.stride(0) == N + po and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    return x, q, s, obuf, out, co


def _run(c, sel, kernel_only=False):
    """One call on the case's views; asserts the guard band and the bound; returns (share, out on the CPU)."""
    M, N, K = c["M"], c["N"], c["K"]
    x, q, s, obuf, out, co = _device_operands(c, sel)
    # the conditions under which ops.linear_w8 takes the HIP paths and not the reference
    assert ops.linear_w8_supported(M, N, K, x, q, s, out) and ops.kernels_available()
    assert lib().rca_linear_w8_splits(N, K) == splits(N, K)
    if kernel_only:
        ops._linear_w8_kernel(x, q.view(torch.float8_e4m3fn), s, out)
    else:
        assert ops.linear_w8(x, q, s, out=out) is out
    torch.cuda.synchronize()
    after = obuf.cpu()
    keep = torch.ones(after.shape, dtype=torch.bool)
    keep[SLACK:SLACK + M, co:co + N] = False
    label = (c["kind"], M, N, K, sel)
    assert torch.equal(after.view(torch.int16)[keep], _sentinel(*after.shape)[keep]), (label, "guard band written")
    got = after[SLACK:SLACK + M, co:co + N].contiguous()
    fail, share = fails(c, got)
    assert not fail.any(), (label, int(fail.sum()), int(fail.flatten().int().argmax()), share)
    return share, got


@gpu
@pytest.mark.parametrize("M", MS)
def test_linear_w8_rows_coded(M):
    worst = 0.0
    for i, (N, K) in enumerate((N, K) for N in NS for K in KS):
        # M <= M_SKINNY is the kernel through the op; above it the op dequantises, so call the kernel itself
        worst = max(worst, _run(case("coded", M, N, K), i + M, kernel_only=M > ops.M_SKINNY)[0])
    print(f"test_linear_w8_rows_coded[{M}]: worst share of the bound {worst:.3f}")


@gpu
@pytest.mark.parametrize("kind", ["exact", "binades", "nonfinite"])
def test_linear_w8_rows_exact_binades_nonfinite(kind):
    worst = 0.0
    for i, (M, N, K) in enumerate(kind_shapes(kind)):
        if M not in (1, 5, 17, 32) or (kind != "exact" and (N, K) not in ((16, 1152), (48, 384), (272, 128), (272, 1152))):
            continue
        worst = max(worst, _run(case(kind, M, N, K), i, kernel_only=M > ops.M_SKINNY)[0])
    print(f"test_linear_w8_rows_exact_binades_nonfinite[{kind}]: worst share of the bound {worst:.3f}")
    assert kind != "exact" or worst == 0.0


@gpu
@pytest.mark.parametrize("M", sorted({32, ops.M_SKINNY}))
@pytest.mark.parametrize("N,K", [(48, 384), (272, 1152), (16, 128)])
def test_rows_do_not_depend_on_the_batch(M, N, K):
    c = case("coded", M, N, K)
    q, s = c["q"].cuda(), c["s"].cuda()
    x = c["x"].cuda()
    assert ops.linear_w8_supported(M, N, K, x, q, s) and M <= ops.M_SKINNY
    full = ops.linear_w8(x, q, s)
    assert not fails(c, full.cpu())[0].any()
    assert torch.equal(ops.linear_w8(x[:5], q, s), full[:5])
    for m in range(M):
        assert torch.equal(ops.linear_w8(x[m:m + 1], q, s), full[m:m + 1]), m
    assert torch.equal(ops._linear_w8_kernel(torch.cat([x, x, x[:7]]), q, s,
                                             torch.empty(2 * M + 7, N, device="cuda", dtype=torch.bfloat16))[M:2 * M], full)


@gpu
def test_dequant_kernel_is_exact():
    from test_linear_w8_cpu import weight_rows

    for K, seed in ((128, 1), (1152, 2)):
        w = weight_rows(K, seed)
        q, s = ref.quantize_weight_fp8_ref(w)
        qbuf = torch.full((q.numel() + 4096,), 0x7F, dtype=torch.uint8)
        qbuf[:q.numel()] = q.view(torch.uint8).reshape(-1)
        qd, sd = qbuf.cuda()[:q.numel()].view(q.shape), s.cuda()
        assert ops._w8_tensor_ok(qd) and ops._w8_tensor_ok(sd)  # the kernel, not the reference
        obuf = _sentinel(1, q.numel() + 64).view(torch.bfloat16).cuda()
        got = ops.dequant_w8(qd, sd, out=obuf[0, :q.numel()].view(q.shape))
        want = ref.kv_dequantize_fp8_ref(q, s)
        assert torch.equal(got.cpu(), want) and torch.equal(ops.dequant_w8(qd.view(torch.float8_e4m3fn), sd).cpu(), want)
        assert torch.equal(obuf.cpu().view(torch.int16)[0, q.numel():], _sentinel(1, q.numel() + 64)[0, q.numel():])


@gpu
@pytest.mark.parametrize("M", [ops.M_SKINNY + 1, 300])
def test_large_m_path_is_inside_the_bound(M):
    for sel, (N, K) in enumerate([(48, 384), (272, 1152)]):
        c = case("coded", M, N, K)
        assert M > ops.M_SKINNY
        share, got = _run(c, sel)
        x, q, s = c["x"].cuda(), c["q"].cuda(), c["s"].cuda()
        assert torch.equal(ops.linear_w8(x, q, s).cpu(), got)  # workspace reuse, no out=
        print(f"test_large_m_path[{M}, {N}, {K}]: share of the bound {share:.3f}")
    # a larger weight after a smaller one: the workspace grows
    c = case("coded", 5, 48, 384)
    big = case("coded", M, 272, 1152)
    assert not fails(big, ops.linear_w8(big["x"].cuda(), big["q"].cuda(), big["s"].cuda()).cpu())[0].any()
    assert not fails(c, ops.linear_w8(c["x"].cuda(), c["q"].cuda(), c["s"].cuda()).cpu())[0].any()


def _c_entry(x, q, s, out, M, N, K):
    ws = torch.empty(8 * M * N + 4, device="cuda")
    return lib().rca_linear_w8a16(x.data_ptr(), q.data_ptr(), s.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 4, M, N, K, x.stride(0), out.stride(0), stream_ptr(x.device))


@gpu
def test_contract_refusals_take_the_reference_path_and_launch_nothing():
    g = torch.Generator().manual_seed(5)
    for M, N, K, off in ((5, 48, 192, 0), (5, 24, 384, 0), (5, 48, 384, 4)):
        xw = torch.randn(M, K + 8, generator=g).bfloat16()
        w = torch.randn(N, K, generator=g)
        q, s = ref.quantize_weight_fp8_ref(w)
        c = dict(kind="coded", M=M, N=N, K=K, x=xw[:, off:off + K])
        W64, X64 = q.double() * s.double()[:, None], c["x"].double()
        c.update(S=X64 @ W64.t(), P=X64.abs() @ W64.abs().t(), mag=max(X64.abs().max().item(), W64.abs().max().item()))
        xd = xw.cuda()[:, off:off + K]
        qd, sd = q.cuda(), s.cuda()
        assert (xd.data_ptr() % 16 == 8) == (off == 4)
        assert not ops.linear_w8_supported(M, N, K, xd, qd, sd)
        sentinel = _sentinel(M, N).view(torch.bfloat16).cuda()
        out = sentinel.clone()
        rc = _c_entry(xd, qd, sd, out, M, N, K)
        torch.cuda.synchronize()
        untouched = torch.equal(out.view(torch.int16), sentinel.view(torch.int16))  # bit patterns: some are NaN
        assert rc == (-2 if off else -1) and untouched, (M, N, K, off, rc)
        got = ops.linear_w8(xd, qd, sd)  # K = 192, N = 24: the reference; misaligned x: made contiguous first
        assert not fails(c, got.cpu())[0].any(), (M, N, K, off)
    c = case("coded", 5, 48, 384)
    x, q, s = c["x"].cuda(), c["q"].cuda(), c["s"].cuda()
    out = torch.empty(5, 48, device="cuda", dtype=torch.bfloat16)
    assert lib().rca_linear_w8a16(x.data_ptr(), q.data_ptr(), s.data_ptr(), out.data_ptr(), 0, 0, 0, 48, 384, 384, 48,
                                  stream_ptr(x.device)) == -1                       # M = 0
    assert _c_entry(x, q, s, out, 5, 48, 384) == 0 and not fails(c, out.cpu())[0].any()
    big = case("coded", 5, 48, 1152)                                               # splits = 2 and no workspace
    x, q, s = big["x"].cuda(), big["q"].cuda(), big["s"].cuda()
    assert lib().rca_linear_w8a16(x.data_ptr(), q.data_ptr(), s.data_ptr(), out.data_ptr(), 0, 0, 5, 48, 1152, 1152, 48,
                                  stream_ptr(x.device)) == -3
    # a transposed (non-unit inner stride) x is made contiguous and still takes the kernel's bound
    xt = c["x"].t().contiguous().cuda().t()
    assert xt.stride(1) != 1 and not fails(c, ops.linear_w8(xt, c["q"].cuda(), c["s"].cuda()).cpu())[0].any()


# ------------------------------------------------------------------------------------ end to end
@gpu
def test_quantised_model_on_gpu_is_as_accurate_as_its_bf16_fake_quant_twin():
    import copy

    from ray_community_amd.models.kv_cache import PagedKVCache

    torch.manual_seed(0)
    base = build_llama("llama3-tiny", dtype=torch.float32).eval()
    quant32 = copy.deepcopy(base).quantize_weights_("fp8")
    twin32 = copy.deepcopy(base)  # the fp32 CPU reference: ordinary linears holding the dequantised values
    with torch.no_grad():
        for (_, a), (_, b) in zip(quant32.named_modules(), twin32.named_modules()):
            if isinstance(a, QuantLinear):
                b.weight.copy_(a.dequantized(torch.float32))
    twin_gpu = copy.deepcopy(twin32).to("cuda", torch.bfloat16)
    # requantising dequantised values keeps every value (a row whose largest byte became 224 takes the next
    # scale down and other bytes, nothing else changes)
    quant_gpu = copy.deepcopy(twin32).to("cuda", torch.bfloat16).quantize_weights_("fp8")
    for (name, a), (_, b) in zip(quant_gpu.named_modules(), quant32.named_modules()):
        if isinstance(a, QuantLinear):
            assert torch.equal(a.dequantized(torch.float32).cpu(), b.dequantized(torch.float32)), name
    prompts = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]
    forced = torch.randint(0, base.cfg.vocab_size, (6, 3), generator=torch.Generator().manual_seed(1))

    def teacher_forced(model, dtype):
        dev = model.embed.weight.device
        cache = PagedKVCache(model.cfg, 32, 16, device=dev, dtype=dtype)
        ids = [0, 1, 2]
        out = [model.prefill(prompts, None, cache, ids)]
        for step in forced:
            out.append(model.decode_step(step, cache, ids))
        return torch.stack(out).float().cpu()

    want = teacher_forced(twin32, torch.float32)
    e_bf16 = (teacher_forced(twin_gpu, torch.bfloat16) - want).abs().max().item()
    got = teacher_forced(quant_gpu, torch.bfloat16)
    e_fp8 = (got - want).abs().max().item()
    print(f"e_bf16 {e_bf16:.4g}  e_fp8 {e_fp8:.4g}  max|logit| {want.abs().max().item():.4g}")
    assert torch.isfinite(got).all()
    assert e_fp8 <= 2 * e_bf16 + 1e-3 * want.abs().max().item()

    toks = quant_gpu.generate(prompts, 9, kv_cache_dtype="fp8")
    assert [len(t) for t in toks] == [9, 9, 9]
    eng = GenerationEngine(quant_gpu, max_slots=4, num_blocks=48, speculative=3, kv_cache_dtype="fp8")
    rids = [eng.add_request(p, 7 + i) for i, p in enumerate(prompts)]
    out = {r: [] for r in rids}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            out[rid].append(tok)
    assert [len(out[r]) for r in rids] == [7, 8, 9]
