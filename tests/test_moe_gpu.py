"""The mixture-of-experts kernels (ops/csrc/moe.hip) against float64 oracles with derived per-element bounds,
then MoE models end to end. x is a view inside a NaN-filled allocation, y a view inside a sentinel-filled one
that must keep its bits outside the view, and the expert weights are followed by NaN, so a read past them shows.

Worst share of the bound, measured on one MI355X (18 tests, 3.3 s): route 0.000, 0.000, 0.001, 0.001 with 64, 64,
63, 64 of 64 rows kept; exact logits 0.000 (k = 2, bit for bit) and 0.345 (k = 8) of the softmax bound; ffn rows in
FFN_CASES' order 0.221, 0.326, 0.314, 0.239, 0.139, 0.324, 0.403, grouped 0.216; rows bit for bit; model e_ref_path
0.008686, e_hip 0.008686 (max |logit| 1.723).
"""
import copy
import math

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import DecodeRunner, GenerationEngine, PagedKVCache, build_llama
from ray_community_amd.ops import reference as ref
from ray_community_amd.ops._lib import lib, stream_ptr

gpu = pytest.mark.gpu
U32, U8 = 2.0 ** -24, 2.0 ** -8  # fp32 accumulation unit per term; the bf16 rounding of the bound
SENTINEL = -7.75  # what y's allocation holds around (and, before the call, inside) the view


@gpu
@pytest.mark.parametrize("H,E,k", [(128, 2, 1), (384, 8, 2), (384, 64, 8), (256, 4, 4)])
def test_route_matches_the_fp64_router_where_fp32_can_decide(H, E, k):
    """eps = H 2^-24 max_e sum_h |x_h| |w_eh| bounds the error of an fp32 sum of a logit, so a row whose top
    min(k + 1, E) fp64 logits are b = 2 eps apart keeps its order: ids are exact. Each exp(l_i - m) then moves
    by a factor within e^(+-eps), and so does their sum: a weight moves by at most (e^(2 eps) - 1) w; the fp32
    softmax itself adds (k + 4 + 2 s) 2^-24 relative, s the spread of the row's top k logits: the subtraction
    l_i - m rounds by s 2^-24 at most, expf is within 1 ulp (2 units), both on a numerator and on the sum's
    terms, then k - 1 adds of positive terms and a division."""
    g = torch.Generator().manual_seed(H + E + k)
    x = torch.randn(64, H, generator=g).bfloat16()
    w = (torch.randn(E, H, generator=g) / math.sqrt(H)).bfloat16()
    logits = x.double() @ w.double().t()
    eps = H * U32 * (x.double().abs() @ w.double().abs().t()).max(dim=1).values
    top = logits.sort(dim=1, descending=True).values[:, :min(k + 1, E)]
    keep = ((top[:, :-1] - top[:, 1:]) >= 2 * eps[:, None]).all(dim=1)
    assert keep.sum().item() >= 56  # 7/8 of the rows: a condition on the reference alone
    want_ids, want_w = ref.moe_route_ref(x.double(), w.double(), k)
    assert ops.moe_supported(64, H, 128, E, k, x.cuda()) and ops.kernels_available()
    ids, weights = ops.moe_route(x.cuda(), w.cuda(), k)
    assert ids.dtype == torch.int32 and weights.dtype == torch.float32 and torch.equal(ids.cpu()[keep], want_ids[keep])
    bound = (torch.expm1(2 * eps) + (k + 4 + 2 * (top[:, 0] - top[:, k - 1] + 2 * eps)) * U32)[:, None] * want_w.double()
    share = ((weights.cpu().double() - want_w.double()).abs() / bound)[keep].max().item()
    print(f"route H={H} E={E} k={k}: kept {int(keep.sum())}/64, worst share of the bound {share:.3f}")
    assert share <= 1


@gpu
@pytest.mark.parametrize("k", [2, 8])
def test_route_orders_equal_logits_by_expert(k):
    """Every logit is an exact small integer, so the ids are the reference's, ties included, and only the fp32
    softmax is left: expf within 1 ulp (2 units of 2^-24) on a numerator and on the terms of the sum, k - 1 adds
    of positive terms and one division, (k + 4) 2^-24 relative against the fp64 softmax. k = 2 is bit for bit."""
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (40, 128), generator=g).bfloat16()
    w = torch.randint(-2, 3, (4, 128), generator=g).bfloat16().repeat_interleave(2, dim=0)  # rows 2i and 2i + 1 are equal
    want_ids, want_w = ref.moe_route_ref(x, w, k)
    ids, weights = ops.moe_route(x.cuda(), w.cuda(), k)
    assert torch.equal(ids.cpu(), want_ids) and (want_ids[:, 1] == want_ids[:, 0] + 1).all()
    exact = torch.softmax((x.double() @ w.double().t()).gather(1, want_ids.long()), dim=1)
    share = ((weights.cpu().double() - exact).abs() / ((k + 4) * U32 * exact + 2.0 ** -126)).max().item()  # + below normal
    print(f"route ties k={k}: worst share of the softmax bound {share:.3f}")
    assert share <= 1 and (k != 2 or torch.equal(weights.cpu().view(torch.int32), want_w.view(torch.int32)))


def _case(T, H, I, E, k, pattern, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    c = dict(T=T, H=H, I=I, E=E, k=k, x=rnd(T, H).bfloat16(), wgu=(rnd(E, 2 * I, H) / math.sqrt(H)).bfloat16(),
             wd=(rnd(E, H, I) / math.sqrt(I)).bfloat16(), weights=torch.softmax(rnd(T, k), dim=1))
    if pattern == "one":  # every pair on the last expert
        ids = torch.full((T, k), E - 1)
    else:  # k distinct experts per row; "skip": none of them is expert 1
        pool = [e for e in range(E) if not (pattern == "skip" and e == 1)]
        ids = torch.stack([torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:k]] for _ in range(T)])
    return dict(c, ids=ids.to(torch.int32))


def _oracle(c, r=0.0):
    """(y, bound) in float64. Per pair: dg = H 2^-24 |W_g| |x| (fp32 accumulation; du alike) goes through
    act = silu(g) u as |u silu'(g)| dg + |silu(g)| du (+ 0.5 |u| dg^2 + 1.1 dg du: |silu''| <= 0.5, |silu'| <=
    1.1) plus the rounding 2^-8 |act|; through the down product as |W_d| dact + I 2^-24 |W_d| |act|; through the
    combine as sum_j |w_j| dd_j plus (k + splits) fp32 roundings; the final rounding is 2^-8 |y|. r = 2^-8 for the
    grouped torch form: its bf16 F.linear (fp32 sums in any order) rounds g, u and d too, r (|v| + dv) more each."""
    T, H, I, E, k = (c[n] for n in "THIEk")
    x, wgu, wd, w = c["x"].double(), c["wgu"].double(), c["wd"].double(), c["weights"].double()
    y, err, mag = torch.zeros(3, T, H, dtype=torch.float64)
    for t in range(T):
        for j in range(k):
            e = int(c["ids"][t, j])
            if not 0 <= e < E:  # adds nothing
                continue
            gate, up = wgu[e, :I] @ x[t], wgu[e, I:] @ x[t]
            dg, du = H * U32 * (wgu[e, :I].abs() @ x[t].abs()), H * U32 * (wgu[e, I:].abs() @ x[t].abs())
            dg, du = (1 + r) * dg + r * gate.abs(), (1 + r) * du + r * up.abs()
            sig = torch.sigmoid(gate)
            act = gate * sig * up
            dact = ((up * sig * (1 + gate * (1 - sig))).abs() * dg + (gate * sig).abs() * du + 0.5 * up.abs() * dg * dg
                    + 1.1 * dg * du + U8 * act.abs())
            d = wd[e] @ act
            dd = (1 + r) * (wd[e].abs() @ dact + I * U32 * (wd[e].abs() @ act.abs())) + r * d.abs()
            y[t] += w[t, j] * d
            err[t] += w[t, j].abs() * dd
            mag[t] += w[t, j].abs() * (d.abs() + dd)
    splits = lib().rca_moe_down_splits(H, I) or 1
    return y, err + (k + splits) * U32 * mag + U8 * y.abs()


def _operands(c):
    """(x view inside NaN, y allocation of sentinels, y view, ids, weights, w_gate_up and w_down followed by NaN)."""
    T, H = c["T"], c["H"]
    xbuf = torch.full((T + 4, H + 16), float("nan"), dtype=torch.bfloat16)
    xbuf[2:2 + T, 8:8 + H] = c["x"]
    ybuf = torch.full((T + 4, H + 16), SENTINEL, dtype=torch.bfloat16).cuda()
    tail = torch.full((4096,), float("nan"), dtype=torch.bfloat16)
    wgu, wd = (torch.cat([c[n].reshape(-1), tail]).cuda()[:c[n].numel()].view(c[n].shape) for n in ("wgu", "wd"))
    return xbuf.cuda()[2:2 + T, 8:8 + H], ybuf, ybuf[2:2 + T, 8:8 + H], c["ids"].cuda(), c["weights"].cuda(), wgu, wd


def _check(c, ybuf, written=True, r=0.0):
    """The guard band (all of y when nothing may be written) keeps the sentinel; the view is within the bound."""
    (T, H), after = (c["T"], c["H"]), ybuf.cpu()
    keep = torch.ones(after.shape, dtype=torch.bool)
    keep[2:2 + T, 8:8 + H] = not written
    assert (after[keep] == SENTINEL).all(), "guard band written"
    if written:
        (want, bound), got = _oracle(c, r), after[2:2 + T, 8:8 + H].double()
        bad = ~((got - want).abs() <= bound)  # a NaN fails
        assert not bad.any(), (int(bad.sum()), int(bad.flatten().int().argmax()))
        return ((got - want).abs() / bound).max().item()


FFN_CASES = [(1, 128, 128, 8, 2, "rand"), (16, 128, 128, 2, 1, "one"), (17, 128, 128, 2, 1, "one"),
             (33, 384, 256, 8, 2, "rand"), (33, 128, 1152, 8, 2, "skip"), (9, 256, 128, 4, 4, "rand"),
             (40, 128, 128, 8, 2, "one"), (65, 128, 128, 8, 2, "grouped")]


@gpu
@pytest.mark.parametrize("T,H,I,E,k,pattern", FFN_CASES)
def test_ffn_rows(T, H, I, E, k, pattern):
    c = _case(T, H, I, E, k, pattern)
    x, ybuf, y, ids, weights, wgu, wd = _operands(c)
    assert ops.moe_supported(T, H, I, E, k, x, y, ids, weights, wgu, wd) and ops.kernels_available()
    assert I != 1152 or (lib().rca_moe_down_splits(H, I) > 1 and (I // 128) % lib().rca_moe_down_splits(H, I))  # ragged
    grouped = pattern == "grouped" and T > ops.M_MOE  # the op above M_MOE rows: reference.moe_ffn_grouped in bf16
    run = ops.moe_ffn if grouped or T <= ops.M_MOE else ops._moe_kernel  # more rows: the kernel entry itself
    assert run(x, ids, weights, wgu, wd, y) is y
    share = _check(c, ybuf, r=U8 if grouped else 0.0)
    print(f"ffn T={T} H={H} I={I} E={E} k={k} {pattern}: worst share of the bound {share:.3f}")


@gpu
def test_rows_do_not_depend_on_the_batch():
    c = _case(21, 128, 1152, 8, 2, "rand", seed=3)  # rca_moe_down_splits(128, 1152) > 1: test_ffn_rows asserts it
    x, ids, weights, wgu, wd = (c[n].cuda() for n in ("x", "ids", "weights", "wgu", "wd"))

    def run(rows):
        rows = torch.as_tensor(rows, device="cuda")
        out = torch.empty(len(rows), 128, device="cuda", dtype=torch.bfloat16)
        return ops._moe_kernel(x[rows].contiguous(), ids[rows].contiguous(), weights[rows].contiguous(), wgu, wd, out).cpu()
    full = run(range(21))
    assert torch.equal(full.view(torch.int16), run(range(21)).view(torch.int16))  # run to run
    for t in range(21):
        assert torch.equal(run([t]).view(torch.int16), full[t:t + 1].view(torch.int16)), t
    perm = torch.randperm(21, generator=torch.Generator().manual_seed(5)).tolist()
    assert torch.equal(run(perm).view(torch.int16), full[perm].view(torch.int16))
    assert torch.equal(run(list(range(21)) * 3).view(torch.int16), full.repeat(3, 1).view(torch.int16))


@gpu
def test_contract_refusals_launch_nothing_and_the_op_answers_through_the_reference():
    T, H, I, E, k = 5, 128, 256, 4, 2
    c = _case(T, H, I, E, k, "rand")
    x, ybuf, y, ids, weights, wgu, wd = _operands(c)
    need = lib().rca_moe_ffn_workspace(T, H, I, E, k)
    ws = torch.full((need // 4 + 4,), float("nan"), device="cuda")
    entry = lambda ws, ids=ids, T=T, H=H, I=I, x_ptr=x.data_ptr(): lib().rca_moe_ffn(  # noqa: E731
        x_ptr, x.stride(0), y.data_ptr(), y.stride(0), ids.data_ptr(), weights.data_ptr(), wgu.data_ptr(), wd.data_ptr(),
        0 if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, T, H, I, E, k, stream_ptr(x.device))
    for want, kw in [(-1, dict(H=192)), (-1, dict(I=192)), (-1, dict(T=0)), (-2, dict(x_ptr=x.data_ptr() + 2)),
                     (-3, dict(ws=None)), (-3, dict(ws=ws[:need // 4 - 1]))]:
        assert entry(**{"ws": ws, **kw}) == want, kw
        _check(c, ybuf, written=False)
    c["ids"][1, 0] = c["ids"][3, 1] = E  # nothing is computed for such a pair: the workspace and past the weights is NaN
    assert entry(ws, ids=c["ids"].cuda()) == 0
    _check(c, ybuf)
    for xs, gu, d in [(x.float(), wgu.float(), wd.float()), (x.float(), wgu, wd)]:  # fp32 within the shapes: the reference
        assert torch.equal(ops.moe_ffn(xs, ids, weights, gu, d), ref.moe_ffn_ref(xs, ids, weights, gu, d))
        assert all(torch.equal(a, b) for a, b in zip(ops.moe_route(xs, gu[:, 0], k), ref.moe_route_ref(xs, gu[:, 0], k)))
    c = _case(T, 192, 192, E, k, "rand")  # outside the contract the op answers through the reference, in the same bound
    x, ybuf, y, ids, weights, wgu, wd = _operands(c)
    assert not ops.moe_supported(T, 192, 192, E, k, x, y, ids, weights, wgu, wd) and ops.moe_ffn(x, ids, weights, wgu, wd, out=y) is y
    _check(c, ybuf)


PROMPTS = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]


def _teacher_forced(model, dtype, forced):
    cache = PagedKVCache(model.cfg, 32, 16, device=model.embed.weight.device, dtype=dtype)
    out = [model.prefill(PROMPTS, None, cache, [0, 1, 2])]
    for step in forced:
        out.append(model.decode_step(step, cache, [0, 1, 2]))
    return torch.stack(out).float().cpu()


@gpu
def test_all_expert_model_on_gpu_is_as_accurate_as_its_reference_path(monkeypatch):
    torch.manual_seed(0)
    base = build_llama("mixtral-tiny", dtype=torch.float32, experts_per_token=4).eval()  # every expert: no routing flips
    forced = torch.randint(0, base.cfg.vocab_size, (6, 3), generator=torch.Generator().manual_seed(1))
    want = _teacher_forced(base, torch.float32, forced)
    model = copy.deepcopy(base).to("cuda", torch.bfloat16)
    monkeypatch.setattr(ops, "M_MOE", 1 << 30)  # the prefill rows through the kernels too
    got = _teacher_forced(model, torch.bfloat16, forced)
    monkeypatch.setattr(ops, "moe_ffn", lambda x, ids, w, gu, d, out=None: ref.moe_ffn_ref(x, ids, w, gu, d))
    via_ref = _teacher_forced(model, torch.bfloat16, forced)
    e_hip, e_ref = (got - want).abs().max().item(), (via_ref - want).abs().max().item()
    print(f"e_ref_path {e_ref:.4g}  e_hip {e_hip:.4g}  max|logit| {want.abs().max().item():.4g}")
    assert torch.isfinite(got).all() and e_hip <= 2 * e_ref + 1e-3 * want.abs().max().item()


@gpu
def test_stock_model_decodes_in_a_graph_and_serves_speculatively():
    torch.manual_seed(0)
    model = build_llama("mixtral-tiny", device="cuda").eval()
    mlp, c1 = model.layers[0].mlp, PagedKVCache(model.cfg, 32, 16, device="cuda")
    assert ops.moe_supported(3, 256, 512, 4, 2, mlp.w_gate_up, mlp.w_down)
    toks = [int(t) for t in model.prefill(PROMPTS, None, c1, ["a", "b", "c"]).argmax(-1)]
    graphed, plain = DecodeRunner(model, c1, 3), DecodeRunner(model, copy.deepcopy(c1), 3, capture=False)
    for step in range(8):
        got, want = graphed.step(toks, ["a", "b", "c"]).clone(), plain.step(toks, ["a", "b", "c"])
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), step
        toks = [int(t) for t in want.argmax(-1)]
    assert graphed.stats["graphs"] >= 1 and graphed.stats["replays"] >= 6
    eng = GenerationEngine(model, max_slots=4, num_blocks=48, graph_decode=True, speculative=3)
    rids = {eng.add_request(p, 7 + i): 7 + i for i, p in enumerate(PROMPTS)}
    out = {r: 0 for r in rids}
    while eng.has_work():
        for rid, _, _ in eng.step():
            out[rid] += 1
    assert out == rids
