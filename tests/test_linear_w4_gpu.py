"""The W4A16 kernel and the MXFP4 dequantiser (ops/csrc/linear_w4.hip) through ``ops.linear_w4`` against the
float64 oracle and bound of tests/test_linear_w8_cpu.py (``fails``), then a quantised model end to end.

Views: x is ``buf[2 : 2 + M, c0 : c0 + K]`` of a NaN-filled allocation, ``out=`` a view inside a
sentinel-filled allocation that must be bit-identical outside the view; the nibble bytes are followed by
0x77 bytes and the scale bytes by 0xFF (a NaN scale) inside larger allocations, so a read past N or K shows.

Worst share of the bound, measured on one MI355X (the file's 13 tests take 3 s): rows M=1 0.916, 5 0.948,
16 0.976, 17 0.955, 32 0.969; the large-M path (33) 0.966; the exact case, row invariance and the dequantiser
bit for bit. The kernel passed every case at its first device run.
"""
import copy
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, QuantLinear, build_llama
from ray_community_amd.ops import reference as ref
from ray_community_amd.ops._lib import lib, stream_ptr
from test_linear_w8_cpu import PADS, _gen, fails, weight_rows
from test_linear_w8_gpu import SLACK, _sentinel

gpu = pytest.mark.gpu
MS, NS, KS = [1, 5, 16, 17, 32], [16, 48, 272], [256, 768, 2304]
SPLITS = {(N, K): lib().rca_linear_w4_splits(N, K) for N in NS for K in KS}
# both epilogues: direct, and K ranges of unequal length (2304 = 9 chunks of 256 over 2 ranges: 5 + 4)
assert all(SPLITS[N, K] == 1 for N in NS for K in (256, 768)) and all(SPLITS[N, 2304] == 2 for N in NS)


def _oracle(x, q, e, **kw):
    W64, X64 = ref.dequantize_mxfp4_ref(q, e, torch.float64), x.double()
    return dict(kind="coded", M=x.shape[0], N=q.shape[0], K=x.shape[1], x=x, q=q, e=e, S=X64 @ W64.t(),
                P=X64.abs() @ W64.abs().t(), mag=max(X64.abs().max().item(), W64.abs().max().item()), **kw)


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """x [M, K] bf16, q [N, K/2], e [N, K/32] on the CPU plus the float64 oracle: Gaussian rows with a
    per-row offset and a per-row binade, so that the block scales differ along and across rows."""
    g = _gen(4, M, N, K)
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
    x = (torch.randn(M, K, generator=g) + 0.5 * torch.sin(0.37 * m + 0.11 * k)).bfloat16()
    w = (torch.randn(N, K, generator=g) + 0.3 * torch.sin(0.7 * n)) * 2.0 ** (n % 5 - 2) * (1 + (k // 32) % 3)
    return _oracle(x, *ref.quantize_weight_mxfp4_ref(w))


def _padded(t, tail, fill):
    buf = torch.full((t.numel() + tail,), fill, dtype=torch.uint8)
    buf[:t.numel()] = t.reshape(-1)
    return buf.cuda()[:t.numel()].view(t.shape)


def _run(c, sel):
    """One call on the case's views; asserts the guard band and the bound; returns (share, out on the CPU)."""
    M, N, K = c["M"], c["N"], c["K"]
    (px, cx), (po, co) = PADS[sel % 3], PADS[(sel + 1) % 3]
    xbuf = torch.full((M + 2 * SLACK, K + px), float("nan"), dtype=torch.bfloat16)
    xbuf[SLACK:SLACK + M, cx:cx + K] = c["x"]
    x = xbuf.cuda()[SLACK:SLACK + M, cx:cx + K]
    q, e = _padded(c["q"], 4096, 0x77), _padded(c["e"], 64, 0xFF)
    obuf = _sentinel(M + 2 * SLACK, N + po).view(torch.bfloat16).cuda()
    out = obuf[SLACK:SLACK + M, co:co + N]
    # the conditions under which ops.linear_w4 takes the HIP paths and not the reference
    assert ops.linear_w4_supported(M, N, K, x, q, e, out) and ops.kernels_available() and x.stride(0) == K + px
    assert ops.linear_w4(x, q, e, out=out) is out
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
@pytest.mark.parametrize("M", MS + [ops.M_SKINNY_W4 + 1])  # the last one: dequantise + F.linear, the same bound
def test_linear_w4_rows_against_the_oracle(M):
    assert MS[-1] == ops.M_SKINNY_W4
    worst = max(_run(case(M, N, K), i + M)[0] for i, (N, K) in enumerate((N, K) for N in NS for K in KS))
    print(f"test_linear_w4_rows_against_the_oracle[{M}]: worst share of the bound {worst:.3f}")


@gpu
@pytest.mark.parametrize("M", [16, 32])
def test_linear_w4_exact_case_bit_for_bit(M):
    """K = 256; nibble (n, k) is code (k + 3 n) % 16 and block (n, b) has e = 127 + (3 n + 5 b) % 9 - 4, so a
    swapped nibble, a wrong byte select, a neighbour's scale or a lost sign changes the value read. Row m
    of x holds +-2^(m % 7 - 3) at k = (256 / M) m + r and zeros elsewhere, so every S is one weight times a
    power of two, a bf16 number (``fails`` asserts it), and r = 0 .. 256 / M - 1 visits every k."""
    N, K = 48, 256
    n, k, m = torch.arange(N)[:, None], torch.arange(K)[None, :], torch.arange(M)
    code = ((k + 3 * n) % 16).to(torch.uint8).view(N, K // 2, 2)
    q = code[..., 0] | (code[..., 1] << 4)
    e = (127 + (3 * n + 5 * torch.arange(K // 32)[None, :]) % 9 - 4).to(torch.uint8)
    for r in range(K // M):
        x = torch.zeros(M, K)
        x[m, (K // M) * m + r] = (1.0 - 2 * ((m + r) % 2)) * 2.0 ** (m % 7 - 3)
        c = _oracle(x.bfloat16(), q, e)
        c["kind"] = "exact"
        assert (c["S"] != 0).sum() >= M * N * 7 // 8 - N
        _run(c, r)


@gpu
@pytest.mark.parametrize("N,K", [(48, 768), (48, 2304)])
def test_rows_do_not_depend_on_the_batch(N, K):
    M = 32
    c = case(M, N, K)
    x, q, e = c["x"].cuda(), c["q"].cuda(), c["e"].cuda()
    assert ops.linear_w4_supported(M, N, K, x, q, e) and (SPLITS[N, K] > 1) == (K == 2304)
    full = ops.linear_w4(x, q, e)
    assert not fails(c, full.cpu())[0].any()
    assert torch.equal(ops.linear_w4(x[:5], q, e), full[:5])
    for m in (0, 15, 16, 31):
        assert torch.equal(ops.linear_w4(x[m:m + 1], q, e), full[m:m + 1]), m
    longer = torch.empty(2 * M + 7, N, device="cuda", dtype=torch.bfloat16)
    assert torch.equal(ops._linear_w4_kernel(torch.cat([x[:9], x, x, x[:30]])[:2 * M + 7], q, e, longer)[9:9 + M], full)


@gpu
def test_dequant_kernel_is_exact():
    for K, seed in ((256, 1), (2304, 2)):
        q, e = ref.quantize_weight_mxfp4_ref(weight_rows(K, seed))
        e[0, :3] = torch.tensor([2, 252, 127], dtype=torch.uint8)  # the ends of the scale range
        qd, ed = _padded(q, 4096, 0x77), _padded(e, 64, 0xFF)
        numel = 2 * q.numel()
        obuf = _sentinel(1, numel + 64).view(torch.bfloat16).cuda()
        got = ops.dequant_w4(qd, ed, out=obuf[0, :numel].view(q.shape[0], K))
        assert torch.equal(got.cpu(), ref.dequantize_mxfp4_ref(q, e)) and torch.equal(ops.dequant_w4(qd, ed), got)
        assert torch.equal(obuf.cpu().view(torch.int16)[0, numel:], _sentinel(1, numel + 64)[0, numel:])


def _c_entry(x, q, e, out, M, N, K, ws=True):
    ws = torch.empty(8 * M * N + 4, device="cuda") if ws else None
    return lib().rca_linear_w4a16(x.data_ptr(), q.data_ptr(), e.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else 0,
                                  ws.numel() * 4 if ws is not None else 0, M, N, K, x.stride(0), out.stride(0),
                                  stream_ptr(x.device))


@gpu
def test_contract_refusals_take_the_reference_path_and_launch_nothing():
    g = torch.Generator().manual_seed(5)
    for M, N, K, off in ((5, 48, 128, 0), (5, 24, 256, 0), (5, 48, 256, 4)):
        xw = torch.randn(M, K + 8, generator=g).bfloat16()
        c = _oracle(xw[:, off:off + K], *ref.quantize_weight_mxfp4_ref(torch.randn(N, K, generator=g)))
        xd, qd, ed = xw.cuda()[:, off:off + K], c["q"].cuda(), c["e"].cuda()
        assert (xd.data_ptr() % 16 == 8) == (off == 4) and not ops.linear_w4_supported(M, N, K, xd, qd, ed)
        sentinel = _sentinel(M, N).view(torch.bfloat16).cuda()
        out = sentinel.clone()
        rc = _c_entry(xd, qd, ed, out, M, N, K)
        torch.cuda.synchronize()
        assert rc == (-2 if off else -1) and torch.equal(out.view(torch.int16), sentinel.view(torch.int16)), (M, N, K, rc)
        got = ops.linear_w4(xd, qd, ed)  # K = 128, N = 24: the reference; misaligned x: made contiguous first
        assert not fails(c, got.cpu())[0].any(), (M, N, K, off)
    assert lib().rca_linear_w4_splits(48, 128) == 0 and lib().rca_linear_w4_splits(24, 256) == 0
    for K, ws, rc in ((768, False, 0), (2304, True, 0), (2304, False, -3)):  # splits = 2 and no workspace: -3
        c = case(5, 48, K)
        out = torch.zeros(5, 48, device="cuda", dtype=torch.bfloat16)
        assert _c_entry(c["x"].cuda(), c["q"].cuda(), c["e"].cuda(), out, 5, 48, K, ws) == rc
        assert (out == 0).all() if rc else not fails(c, out.cpu())[0].any()


# ------------------------------------------------------------------------------------ end to end
@gpu
def test_quantised_model_on_gpu_is_as_accurate_as_its_bf16_fake_quant_twin():
    from ray_community_amd.models.kv_cache import PagedKVCache

    torch.manual_seed(0)
    base = build_llama("llama3-tiny", dtype=torch.float32).eval()
    quant32 = copy.deepcopy(base).quantize_weights_("mxfp4")
    twin32 = copy.deepcopy(base)  # the fp32 CPU reference: ordinary linears holding the dequantised values
    with torch.no_grad():
        for (_, a), (_, b) in zip(quant32.named_modules(), twin32.named_modules()):
            if isinstance(a, QuantLinear):
                b.weight.copy_(a.dequantized(torch.float32))
    twin_gpu = copy.deepcopy(twin32).to("cuda", torch.bfloat16)
    quant_gpu = copy.deepcopy(quant32).to("cuda", torch.bfloat16)  # the same bytes: the casts leave uint8 alone
    assert quant_gpu.layers[0].mlp.down.qweight.dtype == torch.uint8 and quant_gpu.weight_dtype == "mxfp4"
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
    e_q = (got - want).abs().max().item()
    print(f"e_bf16 {e_bf16:.4g}  e_mxfp4 {e_q:.4g}  max|logit| {want.abs().max().item():.4g}")
    assert torch.isfinite(got).all()
    assert e_q <= 2 * e_bf16 + 1e-3 * want.abs().max().item()

    assert [len(t) for t in quant_gpu.generate(prompts, 9)] == [9, 9, 9]
    eng = GenerationEngine(quant_gpu, max_slots=4, num_blocks=48, graph_decode=True)
    rids = [eng.add_request(p, 7 + i) for i, p in enumerate(prompts)]
    out = {r: [] for r in rids}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            out[rid].append(tok)
    assert [len(out[r]) for r in rids] == [7, 8, 9]
