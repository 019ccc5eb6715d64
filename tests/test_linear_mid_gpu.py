"""The mid-M quantised linears (ops/csrc/linear_mid.h through ``ops.linear_w4`` / ``ops.linear_w8`` with
``kernel="mid"`` and the default dispatch above ``M_SKINNY*``) on the cases, float64 oracle, bound and
poisoned views of tests/test_linear_w4_gpu.py and tests/test_linear_w8_gpu.py; bit for bit against the
skinny kernels; the C entries' refusals; a quantised model at 40 rows.

M: 33 (one row into a third tile), 64 / 65 (the 64-row block's last row, the 128-row block's first use),
128 / 129 and 300 (one row into, and a part of, a further 128-row slab).

Worst share of the bound, measured on one MI355X (the file's 27 GPU tests take 3 s): mxfp4 0.966 .. 0.976, fp8
0.976 .. 0.990, set by the rounding term as in the skinny kernels' files. The kernel passed every case at its
first device run.
"""
import copy

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, QuantLinear, build_llama
from ray_community_amd.ops._lib import lib, stream_ptr
from test_linear_w4_gpu import KS as KS4, NS, _oracle, _padded, case as case_w4
from test_linear_w8_cpu import KS as KS8, PADS, case as case_w8, fails
from test_linear_w8_gpu import SLACK, _device_operands, _sentinel

gpu = pytest.mark.gpu
MS = [33, 64, 65, 128, 129, 300]
FORMATS = ["mxfp4", "fp8"]


def _case(fmt, M, N, K):
    """(linear op, case with its oracle, weight and scale on the CPU)"""
    if fmt == "mxfp4":
        c = case_w4(M, N, K)
        return ops.linear_w4, c, c["q"], c["e"]
    c = case_w8("coded", M, N, K)
    return ops.linear_w8, c, c["q"].view(torch.uint8), c["s"]


def _shapes(fmt):
    return [(N, K) for N in NS for K in (KS4 if fmt == "mxfp4" else KS8)]


@gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_mid_kernel_against_the_oracle(fmt, M):
    worst = 0.0
    for i, (N, K) in enumerate(_shapes(fmt)):
        linear, c, _, _ = _case(fmt, M, N, K)
        sel = i + M
        if fmt == "mxfp4":  # the views of test_linear_w4_gpu._run
            (px, cx), (po, co) = PADS[sel % 3], PADS[(sel + 1) % 3]
            xbuf = torch.full((M + 2 * SLACK, K + px), float("nan"), dtype=torch.bfloat16)
            xbuf[SLACK:SLACK + M, cx:cx + K] = c["x"]
            x = xbuf.cuda()[SLACK:SLACK + M, cx:cx + K]
            q, s = _padded(c["q"], 4096, 0x77), _padded(c["e"], 64, 0xFF)
            obuf = _sentinel(M + 2 * SLACK, N + po).view(torch.bfloat16).cuda()
            out = obuf[SLACK:SLACK + M, co:co + N]
        else:
            x, q, s, obuf, out, co = _device_operands(c, sel)
        assert x.stride(0) > K and out.stride(0) > N
        assert linear(x, q, s, out=out, kernel="mid") is out
        torch.cuda.synchronize()
        after = obuf.cpu()
        keep = torch.ones(after.shape, dtype=torch.bool)
        keep[SLACK:SLACK + M, co:co + N] = False
        assert torch.equal(after.view(torch.int16)[keep], _sentinel(*after.shape)[keep]), (fmt, M, N, K, "guard band")
        fail, share = fails(c, after[SLACK:SLACK + M, co:co + N].contiguous())
        assert not fail.any(), (fmt, M, N, K, int(fail.sum()), int(fail.flatten().int().argmax()), share)
        worst = max(worst, share)
    print(f"test_mid_kernel_against_the_oracle[{fmt}-{M}]: worst share of the bound {worst:.3f}")


@gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_mid_kernel_equals_the_skinny_kernel_bit_for_bit(fmt, M):
    for N, K in _shapes(fmt):
        linear, c, q, s = _case(fmt, M, N, K)
        x, q, s = c["x"].cuda(), q.cuda(), s.cuda()
        mid = linear(x, q, s, kernel="mid")
        assert torch.equal(mid, linear(x, q, s, kernel="skinny")), (fmt, M, N, K)
        if M == 64:  # the default dispatch: a row alone (skinny) against the same row of the batch (mid)
            assert max(ops.M_SKINNY, ops.M_SKINNY_W4) < M <= min(ops.M_MID, ops.M_MID_W4)
            full = linear(x, q, s)
            assert torch.equal(full, mid)
            for m in (0, 31, 32, M - 1):
                assert torch.equal(linear(x[m:m + 1], q, s), full[m:m + 1]), (fmt, N, K, m)


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_mid_entries_refuse_what_the_skinny_entries_refuse(fmt):
    L, M = lib(), 40
    skinny, mid = (L.rca_linear_w4a16, L.rca_linear_w4a16_mid) if fmt == "mxfp4" else (L.rca_linear_w8a16, L.rca_linear_w8a16_mid)
    kq, ks = (256, 2304) if fmt == "mxfp4" else (128, 1152)  # the chunk; a K with two ranges
    # (N, K, x offset in elements, workspace, code): K % chunk, N % 16, a misaligned x, no workspace for 2 ranges
    for N, K, off, ws, want in ((48, kq // 2, 0, True, -1), (24, kq, 0, True, -1), (48, kq, 4, True, -2),
                                (48, ks, 0, False, -3)):
        x = torch.ones(M, K + 8, device="cuda", dtype=torch.bfloat16)[:, off:off + K]
        q = torch.zeros(N * K + 64, device="cuda", dtype=torch.uint8)
        s = torch.ones(N * K // 8 + 64, device="cuda", dtype=torch.float32)
        work = torch.empty(8 * M * N, device="cuda") if ws else None
        for entry in (skinny, mid):
            out = _sentinel(M, N).view(torch.bfloat16).cuda()
            rc = entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), out.data_ptr(), work.data_ptr() if ws else 0,
                       work.numel() * 4 if ws else 0, M, N, K, x.stride(0), out.stride(0), stream_ptr(x.device))
            torch.cuda.synchronize()
            assert rc == want and torch.equal(out.cpu().view(torch.int16), _sentinel(M, N)), (fmt, N, K, off, rc)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_forced_arm_never_falls_back(fmt):
    linear, c, q, s = _case(fmt, 5, 48, 768 if fmt == "mxfp4" else 384)
    for kernel in ("skinny", "mid", "dequant"):
        with pytest.raises(ValueError):
            linear(c["x"], q, s, kernel=kernel)  # CPU tensors: the reference path
    with pytest.raises(ValueError):
        linear(c["x"], q, s, kernel="nope")
    assert not fails(c, linear(c["x"], q, s, kernel="auto"))[0].any()
    assert ops.M_SKINNY < ops.M_MID and ops.M_SKINNY_W4 < ops.M_MID_W4


@gpu
def test_quantised_model_at_40_rows_is_as_accurate_as_its_bf16_fake_quant_twin():
    """tests/test_linear_w4_gpu.py's end-to-end criterion with 40 sequences: every linear of a decode step
    has 40 rows, the mid kernel under the default dispatch."""
    from ray_community_amd.models.kv_cache import PagedKVCache

    B = 40
    assert ops.M_SKINNY_W4 < B <= ops.M_MID_W4
    torch.manual_seed(0)
    base = build_llama("llama3-tiny", dtype=torch.float32).eval()
    quant32 = copy.deepcopy(base).quantize_weights_("mxfp4")
    twin32 = copy.deepcopy(base)
    with torch.no_grad():
        for (_, a), (_, b) in zip(quant32.named_modules(), twin32.named_modules()):
            if isinstance(a, QuantLinear):
                b.weight.copy_(a.dequantized(torch.float32))
    twin_gpu = copy.deepcopy(twin32).to("cuda", torch.bfloat16)
    quant_gpu = copy.deepcopy(quant32).to("cuda", torch.bfloat16)
    prompts = [[(7 * i + 3 * j) % 1000 + 1 for j in range(1 + i % 3)] for i in range(B)]
    forced = torch.randint(0, base.cfg.vocab_size, (3, B), generator=torch.Generator().manual_seed(1))

    def teacher_forced(model, dtype):
        cache = PagedKVCache(model.cfg, 2 * B, 16, device=model.embed.weight.device, dtype=dtype)
        ids = list(range(B))
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

    eng = GenerationEngine(quant_gpu, max_slots=B, num_blocks=2 * B, graph_decode=True)
    rids = [eng.add_request(p, 3 + i % 4) for i, p in enumerate(prompts)]
    out = {r: [] for r in rids}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            out[rid].append(tok)
    assert [len(out[r]) for r in rids] == [3 + i % 4 for i in range(B)]
