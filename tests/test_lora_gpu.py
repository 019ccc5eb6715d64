"""The multi-LoRA kernels (ops/csrc/lora.hip) through ``ops.lora_add_`` on the cases, float64 oracle and bound
of tests/test_lora_cpu.py (its CPU tests guard the checker), then LoRA models end to end.

Views: x is ``buf[2 : 2 + M, c0 : c0 + K]`` of a NaN-filled allocation, y a view inside a sentinel-filled
allocation that must be bit-identical outside the view, both with the (row stride - cols, c0) pairs of
tests/test_linear_w8_cpu.py; A, B and the scales are followed by poison (NaN) inside larger allocations, so
a read past a bank shows. Slot 3 of every case is NaN and never named.

Worst share of the bound per GPU test, measured on one MI355X (the file's 10 tests take 4 s; the slowest,
the contract test, 0.6 s):
    test_lora_rows[coded]      0.676 over 65 cases
    test_lora_rows[exact]      bit for bit, 47 cases
    test_lora_rows[binades]    0.731 over 65 cases
    test_rows_do_not_depend_on_the_batch   bit for bit
    test_lora_model_on_gpu_is_as_accurate_as_its_bf16_merged_twin   bf16: e_merged 0.009975, e_lora 0.009909;
                               fp8 weights and cache: e_merged 0.03444, e_lora 0.03083 (max |logit| 1.46)
The shares equal those of the fp32 emulation of tests/test_lora_cpu.py. The kernels passed every case at their
first device run.
"""
import copy

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, LoraAdapter, PagedKVCache, build_llama
from ray_community_amd.ops._lib import lib, stream_ptr
from test_lora_cpu import KINDS, PADS, case, fails, gpu_cases, splits

gpu = pytest.mark.gpu
SLACK = 2


def _sentinel(rows, width):
    idx = torch.arange(rows * width, dtype=torch.int64)
    bits = (idx * 40503 + 0x1234) & 0xFFFF
    return (bits - ((bits >> 15) << 16)).to(torch.int16).view(rows, width)


def _poisoned(t):
    """``t`` on the GPU at the head of a larger NaN-filled allocation."""
    buf = torch.full((t.numel() + 4096,), float("nan"), dtype=t.dtype)
    buf[:t.numel()] = t.reshape(-1)
    return buf.cuda()[:t.numel()].view(t.shape)


def _device_operands(c, sel):
    """(x view, y allocation, y view, its first column, A, B, scale) on the GPU, padded and poisoned."""
    M, N, K = c["M"], c["N"], c["K"]
    (px, cx), (po, co) = PADS[sel % 3], PADS[(sel + 1) % 3]
    xbuf = torch.full((M + 2 * SLACK, K + px), float("nan"), dtype=torch.bfloat16)
    xbuf[SLACK:SLACK + M, cx:cx + K] = c["x"]
    x = xbuf.cuda()[SLACK:SLACK + M, cx:cx + K]
    ybuf = _sentinel(M + 2 * SLACK, N + po).view(torch.bfloat16).clone()
    ybuf[SLACK:SLACK + M, co:co + N] = c["y0"]
    ybuf = ybuf.cuda()
    y = ybuf[SLACK:SLACK + M, co:co + N]
    assert x.stride(0) == K + px and y.stride(0) == N + po and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    return x, ybuf, y, co, _poisoned(c["A"]), _poisoned(c["B"]), _poisoned(c["scale"])


def _run(c, sel):
    """One call on the case's views; asserts the guard band and the bound; returns (share, y on the CPU)."""
    M, N, K, R = c["M"], c["N"], c["K"], c["R"]
    x, ybuf, y, co, A, B, scale = _device_operands(c, sel)
    routing = ops.lora_routing(c["idx"], "cuda")
    # the conditions under which ops.lora_add_ takes the HIP path and not the reference
    assert ops.lora_supported(M, N, K, R, y, x, A, B, scale) and ops.kernels_available()
    assert lib().rca_lora_splits(K, R) == splits(K, R)
    assert ops.lora_add_(y, x, A, B, scale, routing) is y
    torch.cuda.synchronize()
    after = ybuf.cpu()
    keep = torch.ones(after.shape, dtype=torch.bool)
    keep[SLACK:SLACK + M, co:co + N] = False
    label = (c["kind"], M, N, K, R, c["pattern"], sel)
    assert torch.equal(after.view(torch.int16)[keep], _sentinel(*after.shape)[keep]), (label, "guard band written")
    got = after[SLACK:SLACK + M, co:co + N].contiguous()
    fail, share = fails(c, got)
    assert not fail.any(), (label, int(fail.sum()), int(fail.flatten().int().argmax()), share)
    return share, got


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_lora_rows(kind):
    worst = 0.0
    for i, args in enumerate(gpu_cases(kind)):
        worst = max(worst, _run(case(kind, *args), i)[0])
    print(f"test_lora_rows[{kind}]: worst share of the bound {worst:.3f} over {len(gpu_cases(kind))} cases")
    assert kind != "exact" or worst == 0.0


@gpu
@pytest.mark.parametrize("N,K,R", [(48, 384, 32), (272, 1152, 16), (16, 128, 64)])
def test_rows_do_not_depend_on_the_batch(N, K, R):
    M = 33
    c = case("coded", M, N, K, R, "cycle")
    x, y0, A, B, scale = (c[k].cuda() for k in ("x", "y0", "A", "B", "scale"))
    idx = c["idx"]

    def run(xs, ys, ids):
        y = ys.clone()
        assert ops.lora_supported(len(ids), N, K, R, y, xs, A, B, scale)
        return ops.lora_add_(y, xs, A, B, scale, ops.lora_routing(ids, "cuda"))

    full = run(x, y0, idx)
    assert not fails(c, full.cpu())[0].any()
    for m in range(M):  # each row alone
        assert torch.equal(run(x[m:m + 1], y0[m:m + 1], idx[m:m + 1]), full[m:m + 1]), m
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(4))
    got = run(x[perm.cuda()].contiguous(), y0[perm.cuda()].contiguous(), [idx[p] for p in perm.tolist()])
    assert torch.equal(got, full[perm.cuda()])
    three = run(torch.cat([x, x, x]), torch.cat([y0, y0, y0]), idx * 3)
    assert torch.equal(three[M:2 * M], full) and torch.equal(three[:M], full)
    assert torch.equal(run(x, y0, idx), full)  # and run to run


def _c_entry(x, y, A, B, scale, routing, M, N, K, R, ws="make", n_tiles=None):
    n = routing.n_tiles if n_tiles is None else n_tiles
    if ws == "make":
        ws = torch.empty(16 * max(n, 1) * 16 * R + 4, device="cuda")
    return lib().rca_lora_add(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), A.data_ptr(), B.data_ptr(),
                              scale.data_ptr(), routing.tile_slot.data_ptr(), routing.tile_rows.data_ptr(), n,
                              0 if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, M, N, K, R,
                              A.shape[0], stream_ptr(x.device))


@gpu
def test_all_base_rows_and_zero_tiles_launch_nothing(monkeypatch):
    c = case("coded", 17, 48, 384, 32, "none")
    share, got = _run(c, 1)
    assert share == 0.0 and torch.equal(got.view(torch.int16), c["y0"].view(torch.int16))
    x, y0, A, B, scale = (c[k].cuda() for k in ("x", "y0", "A", "B", "scale"))
    routing = ops.lora_routing(c["idx"], "cuda")
    assert not routing.any and routing.n_tiles == 0
    monkeypatch.setattr(ops, "_lora_kernel", lambda *a: pytest.fail("the C entry was reached"))
    y = y0.clone()
    assert ops.lora_add_(y, x, A, B, scale, routing) is y and torch.equal(y.view(torch.int16), y0.view(torch.int16))
    monkeypatch.undo()
    # a direct call with n_tiles = 0: returns 0 and writes nothing, even with tiles in the arrays
    busy = ops.lora_routing(case("coded", 17, 48, 384, 32, "cycle")["idx"], "cuda")
    sentinel = _sentinel(17, 48).view(torch.bfloat16).cuda()
    y = sentinel.clone()
    assert _c_entry(x, y, A, B, scale, busy, 17, 48, 384, 32, n_tiles=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), sentinel.view(torch.int16))


@gpu
def test_contract_refusals_take_the_reference_path_and_launch_nothing():
    g = torch.Generator().manual_seed(5)
    S = 4
    for M, N, K, R, off, want_rc in ((5, 48, 192, 32, 0, -1), (5, 24, 384, 32, 0, -1), (5, 48, 384, 24, 0, -1),
                                     (5, 48, 384, 32, 4, -2)):
        xw = torch.randn(M, K + 8, generator=g).bfloat16()
        y0 = torch.randn(M, N, generator=g).bfloat16()
        A = (torch.randn(S, R, K, generator=g) / K ** 0.5).bfloat16()
        B = (torch.randn(S, N, R, generator=g) * 0.25).bfloat16()
        scale = torch.tensor([0.5, 2.0, -1.25, 1.0])
        idx = [m % 3 for m in range(M)]
        xs = xw[:, off:off + K]
        c = dict(kind="coded", M=M, N=N, K=K, R=R, y0=y0, base=torch.zeros(M, dtype=torch.bool))
        S64, bound = y0.double().clone(), torch.zeros(M, N, dtype=torch.float64)
        for m, a in enumerate(idx):  # the oracle and bound of tests/test_lora_cpu.py, row by row
            X, A64, B64, sc = xs[m].double(), A[a].double(), B[a].double(), scale[a].double()
            T = A64 @ X
            S64[m] = y0[m].double() + sc * (B64 @ T)
            t_err = 2.0 ** -8 * T.abs() + K * 2.0 ** -24 * (A64.abs() @ X.abs())
            bound[m] = sc.abs() * (B64.abs() @ t_err) + R * 2.0 ** -24 * sc.abs() * (B64.abs() @ T.abs())
        c.update(S=S64, bound=bound + 2.0 ** -8 * S64.abs() + 2.0 ** -126)
        xd = xw.cuda()[:, off:off + K]
        Ad, Bd, sd = A.cuda(), B.cuda(), scale.cuda()
        routing = ops.lora_routing(idx, "cuda")
        assert (xd.data_ptr() % 16 == 8) == (off == 4)
        sentinel = _sentinel(M, N).view(torch.bfloat16).cuda()
        y = sentinel.clone()
        assert not ops.lora_supported(M, N, K, R, y, xd, Ad, Bd, sd)
        rc = _c_entry(xd, y, Ad, Bd, sd, routing, M, N, K, R)
        torch.cuda.synchronize()
        untouched = torch.equal(y.view(torch.int16), sentinel.view(torch.int16))  # bit patterns: some are NaN
        assert rc == want_rc and untouched, (M, N, K, R, off, rc)
        got = ops.lora_add_(y0.cuda(), xd, Ad, Bd, sd, routing)  # the reference answers
        assert not fails(c, got.cpu())[0].any(), (M, N, K, R, off)
    c = case("coded", 5, 48, 384, 32, "cycle")
    x, y0, A, B, scale = (c[k].cuda() for k in ("x", "y0", "A", "B", "scale"))
    routing = ops.lora_routing(c["idx"], "cuda")
    sentinel = _sentinel(5, 48).view(torch.bfloat16).cuda()
    y = sentinel.clone()
    assert _c_entry(x, y, A, B, scale, routing, 5, 48, 384, 32, ws=None) == -3            # no workspace
    assert _c_entry(x, y, A, B, scale, routing, 5, 48, 384, 32, ws=torch.empty(16, device="cuda")) == -3  # too small
    assert _c_entry(x, y, A, B, scale, routing, 0, 48, 384, 32) == -1                     # M = 0
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), sentinel.view(torch.int16))
    y = y0.clone()
    assert _c_entry(x, y, A, B, scale, routing, 5, 48, 384, 32) == 0 and not fails(c, y.cpu())[0].any()


# ------------------------------------------------------------------------------------ end to end
PROMPTS = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]
NAMES = ["a", None, "b"]


def _teacher_forced(model, dtype, forced, kv=None, **kw):
    dev = model.embed.weight.device
    cache = PagedKVCache(model.cfg, 32, 16, device=dev, dtype=dtype, kv_dtype=kv)
    ids = [0, 1, 2]
    out = [model.prefill(PROMPTS, None, cache, ids, **kw)]
    for step in forced:
        out.append(model.decode_step(step, cache, ids, **kw))
    return torch.stack(out).float().cpu()


def _merged(base, ads, name):
    """A plain model whose weights hold ``W + scale * B @ A`` of adapter ``name`` (``None``: the base)."""
    from ray_community_amd.models import lora as lora_mod

    twin = copy.deepcopy(base)
    if name is not None:
        with torch.no_grad():
            for (parent, t), lay in zip(lora_mod._targets(twin), (lay for lay in ads[name].layers for _ in lora_mod.TARGETS)):
                A, B, scale = lay[t]
                getattr(parent, t).weight.add_(scale * (B @ A))
    return twin


@gpu
@pytest.mark.parametrize("fp8", [False, True])
def test_lora_model_on_gpu_is_as_accurate_as_its_bf16_merged_twin(fp8):
    torch.manual_seed(0)
    base = build_llama("llama3-tiny", dtype=torch.float32).eval()
    if fp8:  # fp8 weights underneath: start from a base whose weights are the dequantised values
        from ray_community_amd.models import QuantLinear

        q = copy.deepcopy(base).quantize_weights_("fp8")
        with torch.no_grad():
            for (_, a), (_, b) in zip(q.named_modules(), base.named_modules()):
                if isinstance(a, QuantLinear):
                    b.weight.copy_(a.dequantized(torch.float32))
    ads = {"a": LoraAdapter.random(base.cfg, 4, seed=1), "b": LoraAdapter.random(base.cfg, 2, seed=2, alpha=8)}
    # bf16 adapters everywhere, so that the twins and the bank hold the same values
    for ad in ads.values():
        ad.layers = [{t: (A.bfloat16().float(), B.bfloat16().float(), s) for t, (A, B, s) in lay.items()} for lay in ad.layers]
    forced = torch.randint(0, base.cfg.vocab_size, (6, 3), generator=torch.Generator().manual_seed(1))
    kv = "fp8" if fp8 else None
    # the fp32 CPU reference and the bf16 GPU twin: one merged-weight model per sequence, one row each
    want, twin_gpu = [], []
    for b, name in enumerate(NAMES):
        m32 = _merged(base, ads, name)
        want.append(_teacher_forced(m32, torch.float32, forced)[:, b])
        twin_gpu.append(_teacher_forced(copy.deepcopy(m32).to("cuda", torch.bfloat16), torch.bfloat16, forced, kv)[:, b])
    want, twin_gpu = torch.stack(want, 1), torch.stack(twin_gpu, 1)
    model = copy.deepcopy(base).to("cuda", torch.bfloat16)
    if fp8:
        model.quantize_weights_("fp8")
    plain = _teacher_forced(model, torch.bfloat16, forced, kv)
    model.enable_lora_(max_adapters=3, max_rank=4)
    assert torch.equal(_teacher_forced(model, torch.bfloat16, forced, kv), plain)  # enabled, unused: no bit moves
    for name, ad in ads.items():
        model.load_adapter(name, ad)
    lin = model.layers[0].attn.qkv
    assert ops.lora_supported(3, lin.out_features, lin.in_features, lin.lora_A.shape[1], lin.lora_A, lin.lora_B, lin.lora_scale)
    got = _teacher_forced(model, torch.bfloat16, forced, kv, adapters=NAMES)
    e_twin, e_lora = (twin_gpu - want).abs().max().item(), (got - want).abs().max().item()
    print(f"fp8={fp8}: e_bf16_merged {e_twin:.4g}  e_lora {e_lora:.4g}  max|logit| {want.abs().max().item():.4g}")
    assert torch.isfinite(got).all()
    assert e_lora <= 2 * e_twin + 1e-3 * want.abs().max().item()
    assert torch.equal(got[:, 1], plain[:, 1]) or (got[:, 1] - plain[:, 1]).abs().max() <= 2 * e_twin  # the base row
    assert (got[:, 0] - plain[:, 0]).abs().max().item() > 4 * e_twin  # the adapter does something

    eng = GenerationEngine(model, max_slots=4, num_blocks=48, speculative=3, kv_cache_dtype=kv)
    rids = [eng.add_request(p, 7 + i, **({} if a is None else {"adapter": a})) for i, (p, a) in enumerate(zip(PROMPTS, NAMES))]
    out = {r: [] for r in rids}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            out[rid].append(tok)
    assert [len(out[r]) for r in rids] == [7, 8, 9]
