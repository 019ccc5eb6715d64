"""The MXFP4 expert FFN kernels (ops/csrc/moe_w4.hip) against the float64 oracle and per-element bound of
tests/test_moe_gpu.py applied to the exactly dequantised weights (the kernels multiply by exactly known bf16
values, so the derivation carries over; splits is rca_moe_w4_down_splits), then a quantised MoE model end to end.

q and the scale bytes are drawn directly: random nibbles, and per-block E8M0 bytes uniform in [115, 122] (8 wide, so
neighbouring blocks differ and a wrong scale byte shows; |w| <= 6 * 2^-5 keeps g, u and d of size 1 at these H and
I). x is a view inside NaN, y a view inside sentinels that must keep their bits, and q and s are each followed by 0xFF
bytes (nibble -6 times an E8M0 NaN), so a read past the end shows.

Worst share of the bound, measured on one MI355X (11 tests, 4 s): ffn rows in FFN_CASES' order 0.259, 0.570, 0.570,
0.380, 0.195 (2 K ranges), 0.293, 0.291, grouped 0.347; rows bit for bit; model e_ref_path 0.008481, e_hip 0.008481
(max |logit| 1.713).
"""
import copy

import pytest
import test_moe_gpu
import torch
from test_moe_gpu import PROMPTS, U8, _case, _check, _teacher_forced

from ray_community_amd import ops
from ray_community_amd.models import DecodeRunner, GenerationEngine, PagedKVCache, build_llama
from ray_community_amd.ops import reference as ref
from ray_community_amd.ops._lib import lib, stream_ptr

gpu = pytest.mark.gpu
QUADS = ("q_gate_up", "s_gate_up", "q_down", "s_down")


@pytest.fixture(autouse=True)
def _w4_splits(monkeypatch):
    """test_moe_gpu._oracle counts the combine's roundings with its lib()'s split rule: give it the W4 rule."""
    class W4:
        rca_moe_down_splits = staticmethod(lambda H, I: lib().rca_moe_w4_down_splits(H, I))
    monkeypatch.setattr(test_moe_gpu, "lib", lambda: W4)


def _w4_case(T, H, I, E, k, pattern, seed=0):
    """test_moe_gpu._case with wgu / wd the dequantised values of random MXFP4 bytes, which it carries too."""
    c = _case(T, H, I, E, k, pattern, seed)
    g = torch.Generator().manual_seed(seed + 1)
    for name, (N, K) in (("gate_up", (2 * I, H)), ("down", (H, I))):
        q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.uint8)
        s = torch.randint(115, 123, (E, N, K // 32), generator=g, dtype=torch.uint8)
        c["q_" + name], c["s_" + name] = q, s
        c["wgu" if name == "gate_up" else "wd"] = ref.dequantize_mxfp4_ref(q.flatten(0, 1), s.flatten(0, 1)).view(E, N, K)
    if pattern == "bad":  # ids outside [0, E): such a pair adds nothing
        c["ids"][0, 0], c["ids"][T - 1, k - 1] = E, -1
    return c


def _w4_operands(c):
    """(x view inside NaN, y allocation of sentinels, y view, ids, weights, the four uint8 tensors followed by 0xFF)."""
    x, ybuf, y, ids, weights, _, _ = test_moe_gpu._operands(c)
    tail = torch.full((4096,), 0xFF, dtype=torch.uint8)
    quads = [torch.cat([c[n].reshape(-1), tail]).cuda()[:c[n].numel()].view(c[n].shape) for n in QUADS]
    return x, ybuf, y, ids, weights, quads


FFN_CASES = [(1, 256, 256, 8, 2, "rand"), (16, 256, 256, 2, 1, "one"), (17, 256, 256, 2, 1, "one"),
             (33, 768, 256, 8, 2, "rand"), (33, 256, 2304, 8, 2, "skip"), (9, 256, 256, 4, 4, "rand"),
             (12, 512, 512, 8, 2, "bad"), (ops.M_MOE_W4 + 1, 256, 256, 8, 2, "grouped")]


@gpu
@pytest.mark.parametrize("T,H,I,E,k,pattern", FFN_CASES)
def test_ffn_rows(T, H, I, E, k, pattern):
    c = _w4_case(T, H, I, E, k, pattern)
    x, ybuf, y, ids, weights, quads = _w4_operands(c)
    assert ops.moe_w4_supported(T, H, I, E, k, x, y, ids, weights, *quads) and ops.kernels_available()
    splits = lib().rca_moe_w4_down_splits(H, I)
    assert I != 2304 or (splits > 1 and (I // 256) % splits)  # ragged K ranges
    grouped = pattern == "grouped"  # the op above M_MOE_W4 rows: dequantise and group, bf16 F.linear
    assert ops.moe_ffn_w4(x, ids, weights, *quads, out=y) is y
    share = _check(c, ybuf, r=U8 if grouped else 0.0)
    print(f"ffn_w4 T={T} H={H} I={I} E={E} k={k} {pattern}: splits {splits}, worst share of the bound {share:.3f}")


@gpu
def test_rows_do_not_depend_on_the_batch():
    c = _w4_case(21, 256, 2304, 8, 2, "rand", seed=3)  # rca_moe_w4_down_splits(256, 2304) > 1: test_ffn_rows asserts it
    x, ids, weights, *quads = (c[n].cuda() for n in ("x", "ids", "weights") + QUADS)

    def run(rows):
        rows = torch.as_tensor(rows, device="cuda")
        out = torch.empty(len(rows), 256, device="cuda", dtype=torch.bfloat16)
        return ops._moe_w4_kernel(x[rows].contiguous(), ids[rows].contiguous(), weights[rows].contiguous(), *quads, out).cpu()
    full = run(range(21))
    assert torch.equal(full.view(torch.int16), run(range(21)).view(torch.int16))  # run to run
    for t in range(21):
        assert torch.equal(run([t]).view(torch.int16), full[t:t + 1].view(torch.int16)), t
    perm = torch.randperm(21, generator=torch.Generator().manual_seed(5)).tolist()
    assert torch.equal(run(perm).view(torch.int16), full[perm].view(torch.int16))
    assert torch.equal(run(list(range(21)) * 3).view(torch.int16), full.repeat(3, 1).view(torch.int16))


@gpu
def test_contract_refusals_launch_nothing_and_the_op_answers_through_the_reference():
    T, H, I, E, k = 5, 256, 512, 4, 2
    c = _w4_case(T, H, I, E, k, "rand")
    x, ybuf, y, ids, weights, quads = _w4_operands(c)
    need = lib().rca_moe_ffn_w4_workspace(T, H, I, E, k)
    ws = torch.full((need // 4 + 4,), float("nan"), device="cuda")
    entry = lambda ws, T=T, H=H, I=I, x_ptr=x.data_ptr(): lib().rca_moe_ffn_w4(  # noqa: E731
        x_ptr, x.stride(0), y.data_ptr(), y.stride(0), ids.data_ptr(), weights.data_ptr(), *(t.data_ptr() for t in quads),
        0 if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, T, H, I, E, k, stream_ptr(x.device))
    for want, kw in [(-1, dict(H=128)), (-1, dict(I=384)), (-1, dict(T=0)), (-2, dict(x_ptr=x.data_ptr() + 2)),
                     (-3, dict(ws=None)), (-3, dict(ws=ws[:need // 4 - 1]))]:
        assert entry(**{"ws": ws, **kw}) == want, kw
        _check(c, ybuf, written=False)
    assert entry(ws) == 0  # the workspace starts as NaN
    _check(c, ybuf)
    c = _w4_case(T, 128, 384, E, k, "rand")  # outside the contract the op answers through the reference, in the same bound
    x, ybuf, y, ids, weights, quads = _w4_operands(c)
    assert not ops.moe_w4_supported(T, 128, 384, E, k, x, y, ids, weights, *quads)
    assert ops.moe_ffn_w4(x, ids, weights, *quads, out=y) is y
    _check(c, ybuf)


@gpu
def test_quantised_model_is_as_accurate_as_its_reference_path_and_decodes_in_a_graph(monkeypatch):
    torch.manual_seed(0)
    base = build_llama("mixtral-tiny", dtype=torch.float32, experts_per_token=4, expert_dtype="mxfp4").eval()
    forced = torch.randint(0, base.cfg.vocab_size, (6, 3), generator=torch.Generator().manual_seed(1))
    want = _teacher_forced(base, torch.float32, forced)  # fp32 on the CPU over the same quantised bytes
    model = copy.deepcopy(base).to("cuda", torch.bfloat16)
    mlp = model.layers[0].mlp
    assert ops.moe_w4_supported(3, 256, 512, 4, 4, *(getattr(mlp, n) for n in QUADS))

    c1 = PagedKVCache(model.cfg, 32, 16, device="cuda")  # before M_MOE_W4 is patched: as the model is served
    toks = [int(t) for t in model.prefill(PROMPTS, None, c1, ["a", "b", "c"]).argmax(-1)]
    graphed, plain = DecodeRunner(model, c1, 3), DecodeRunner(model, copy.deepcopy(c1), 3, capture=False)
    for step in range(5):
        got, ref_step = graphed.step(toks, ["a", "b", "c"]).clone(), plain.step(toks, ["a", "b", "c"])
        assert torch.equal(got.view(torch.int16), ref_step.view(torch.int16)), step
        toks = [int(t) for t in ref_step.argmax(-1)]
    assert graphed.stats["graphs"] >= 1 and graphed.stats["replays"] >= 3
    eng = GenerationEngine(model, max_slots=4, num_blocks=48, graph_decode=True, speculative=3)
    rids = {eng.add_request(p, 7 + i): 7 + i for i, p in enumerate(PROMPTS)}
    out = {r: 0 for r in rids}
    while eng.has_work():
        for rid, _, _ in eng.step():
            out[rid] += 1
    assert out == rids

    monkeypatch.setattr(ops, "M_MOE_W4", 1 << 30)  # the prefill rows through the kernels too
    got = _teacher_forced(model, torch.bfloat16, forced)
    monkeypatch.setattr(ops, "moe_ffn_w4", lambda x, ids, w, *quads, out=None: ref.moe_ffn_w4_ref(x, ids, w, *quads))
    via_ref = _teacher_forced(model, torch.bfloat16, forced)
    e_hip, e_ref = (got - want).abs().max().item(), (via_ref - want).abs().max().item()
    print(f"w4 model: e_ref_path {e_ref:.4g}  e_hip {e_hip:.4g}  max|logit| {want.abs().max().item():.4g}")
    assert torch.isfinite(got).all() and e_hip <= 2 * e_ref + 1e-3 * want.abs().max().item()
