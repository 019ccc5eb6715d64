"""Multi-LoRA (ops.lora_add_, ops.lora_routing, models.lora, the engine's per-request adapters) without a
GPU, and the cases, float64 oracle, bound checker and fp32 emulation that tests/test_lora_gpu.py runs the
kernels through.

Contract (ops/reference.py, lora_add_ref): with a = idx[m] >= 0 the slot of row m,
    t[m, :] = bf16(sum_k A[a, :, k] x[m, k])        y[m, n] = bf16(y0[m, n] + scale[a] sum_r B[a, n, r] t[m, r])
both sums in fp32; a row with idx[m] < 0 keeps its bits.

Oracle and bound. From the bf16 inputs in float64: T = A x, S = y0 + scale B T (t unrounded), and per element
    |got - S| <= 2**-8 |S|                                           the final bf16 rounding
               + |scale| |B| @ (2**-8 |T| + K 2**-24 |A| |x|)        t: its bf16 rounding and fp32 accumulation over K
               + R 2**-24 |scale| |B| @ |T|                          the fp32 accumulation over R
               + TINY max(1, magnitude)
Nothing in it is taken from a kernel. On the ``exact`` kind every fp32 sum is exact (small integers times
powers of two), so the two roundings are the only inexact steps and the oracle applies them itself: the
comparison is bit for bit, and it sees whether t was rounded. Base rows are compared bit for bit on every kind.

Every case has S = 4 slots; slot 3 is never named and is NaN in A, B and scale; slot 1 holds a rank-8 adapter
inside capacity R (the rest zero).

The emulation follows ops/csrc/lora.hip: K is cut into ``splits(K, R)`` ranges of 128-deep blocks (a mirror of
the kernel's rule, compared with the library's on the GPU), every range is summed in fp32 in 32-deep groups
(one MFMA each), the partials are added in range order and rounded to bf16 (t), the expand step sums over R
in 32-deep groups, multiplies by scale, adds y0 and rounds once. Worst share of the bound over every GPU
case: printed by ``test_fp32_emulation_passes_every_gpu_case`` (coded 0.676, binades 0.731; ``exact`` is bit
for bit).
"""
import copy
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import (AdapterSlotsFull, GenerationEngine, LoraAdapter, LoraLinear, PagedKVCache,
                                      build_llama, weight_bytes)
from ray_community_amd.models import lora as lora_mod
from ray_community_amd.ops import reference as ref
from test_linear_w8_cpu import PADS, TINY, _gen  # noqa: F401  (PADS: for the GPU file)

S = 4
NAN_SLOT, LOW_RANK_SLOT, LOW_RANK = 3, 1, 8
MS = [1, 2, 5, 16, 17, 32, 33, 70]
NKS = [(16, 128), (48, 384), (272, 1152)]
RS = [16, 32, 64]
KINDS = ["coded", "exact", "binades"]
PATTERNS = ["one", "cycle", "base_mixed", "none", "big_and_single"]


def splits(K, R):
    """Mirror of lora_splits (ops/csrc/lora.hip): a function of K and R only."""
    kblocks, most, ks = K // 128, 16 if R <= 64 else 8, 1
    while ks < most and ks * 2 * 4 <= kblocks:
        ks *= 2
    return ks


def pattern_idx(pattern, M):
    if pattern == "one":
        return [2] * M
    if pattern == "cycle":  # the rows of a slot are not contiguous
        return [m % 3 for m in range(M)]
    if pattern == "base_mixed":
        return [-1 if m % 2 == 0 else (m // 2) % 3 for m in range(M)]
    if pattern == "none":
        return [-1] * M
    idx = [0] * M  # more than 16 rows on slot 0 (from M = 18), exactly one on slot 1
    idx[min(3, M - 1)] = 1
    return idx


def gpu_cases(kind):
    """(M, N, K, R, pattern): every M and pattern at one (N, K, R); every (N, K, R) at three M with the
    patterns in turn (rows are independent); R = 192 once."""
    out, turn = [], 0
    for N, K in NKS:
        if kind == "exact" and K > 256:
            continue
        for R in RS:
            for M in MS:
                if (N, K, R) == ((48, 384, 32) if kind != "exact" else (16, 128, 32)):
                    out += [(M, N, K, R, p) for p in PATTERNS]
                elif M in (5, 33, 70):
                    out.append((M, N, K, R, PATTERNS[turn % 5]))
                    turn += 1
    out.append((33, 16, 128, 192, "cycle") if kind == "exact" else (33, 48, 384, 192, "cycle"))
    return out


# ------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def case(kind, M, N, K, R, pattern):
    """x [M, K], y0 [M, N], A [S, R, K], B [S, N, R] bf16, scale [S] fp32, idx (list) on the CPU, plus the
    float64 oracle and the terms of the bound."""
    g = _gen(KINDS.index(kind), M, N, K, R, PATTERNS.index(pattern))
    m = torch.arange(M, dtype=torch.float64)[:, None]
    s = torch.arange(S, dtype=torch.float64)[:, None, None]
    if kind == "exact":
        assert K <= 256
        # integers times a power of two per row: T = A x needs up to 14 bits (so its bf16 rounding is visible)
        # and every partial sum of both products stays below 2**24 units, i.e. exact in fp32
        x = torch.randint(-3, 4, (M, K), generator=g).double() * 2.0 ** (m % 7 - 3)
        y0 = torch.randint(-1, 2, (M, N), generator=g).double() * 2.0 ** (m % 7 - 3)
        A = torch.randint(-31, 32, (S, R, K), generator=g).double()
        B = torch.randint(-1, 2, (S, N, R), generator=g).double()
        scale = torch.tensor([0.5, 2.0, 1.0, 1.0], dtype=torch.float64)
    else:
        x, y0 = torch.randn(M, K, generator=g).double(), torch.randn(M, N, generator=g).double()
        A = torch.randn(S, R, K, generator=g).double() / K ** 0.5
        B = torch.randn(S, N, R, generator=g).double() * 0.25
        scale = torch.tensor([0.5, 2.0, -1.25, 1.0], dtype=torch.float64)
        if kind == "binades":  # rows and slots over 2^-6 .. 2^6
            x, y0 = x * 2.0 ** (m % 13 - 6), y0 * 2.0 ** (m % 13 - 6)
            A, scale = A * 2.0 ** (3 * s - 3), scale * 2.0 ** (3 - 3 * s[:, 0, 0])
    A[LOW_RANK_SLOT, LOW_RANK:] = 0  # a rank-8 adapter inside capacity R
    B[LOW_RANK_SLOT, :, LOW_RANK:] = 0
    x, y0, A, B, scale = x.bfloat16(), y0.bfloat16(), A.bfloat16(), B.bfloat16(), scale.float()
    A[NAN_SLOT], B[NAN_SLOT], scale[NAN_SLOT] = float("nan"), float("nan"), float("nan")
    idx = pattern_idx(pattern, M)
    assert NAN_SLOT not in idx
    c = dict(kind=kind, M=M, N=N, K=K, R=R, pattern=pattern, x=x, y0=y0, A=A, B=B, scale=scale, idx=idx)
    S64, bound = y0.double().clone(), torch.zeros(M, N, dtype=torch.float64)
    want = y0.clone()
    mag = max(x.double().abs().max().item(), y0.double().abs().max().item())
    for a in sorted(set(idx) - {-1}):
        rows = torch.tensor([i for i, v in enumerate(idx) if v == a])
        X, A64, B64, sc = x[rows].double(), A[a].double(), B[a].double(), scale[a].double()
        T = X @ A64.t()
        S64[rows] = y0[rows].double() + sc * (T @ B64.t())
        t_err = 2.0 ** -8 * T.abs() + K * 2.0 ** -24 * (X.abs() @ A64.abs().t())
        bound[rows] = sc.abs() * (t_err @ B64.abs().t()) + R * 2.0 ** -24 * sc.abs() * (T.abs() @ B64.abs().t())
        mag = max(mag, A64.abs().max().item(), B64.abs().max().item(), sc.abs().item())
        if kind == "exact":
            assert torch.equal(T.float().double(), T)
            t = T.float().bfloat16().double()
            full = y0[rows].double() + sc * (t @ B64.t())
            assert torch.equal(full.float().double(), full)  # every fp32 sum on the way is exact
            want[rows] = full.float().bfloat16()
    bound = bound + 2.0 ** -8 * S64.abs() + TINY * max(1.0, mag)
    c.update(S=S64, bound=bound, want=want, base=torch.tensor([v < 0 for v in idx]))
    return c


def fails(c, got):
    """[M][N] bool, True where ``got`` (bf16, CPU) is rejected, and the worst share of the bound. No
    element is left out: adapter rows against the bound (``exact``: bit for bit), base rows bit for bit."""
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (c["M"], c["N"])
    bits = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    same_base = bits(got) == bits(c["y0"])
    if c["kind"] == "exact":
        fail = bits(got) != bits(c["want"])
        fail[c["base"]] = ~same_base[c["base"]]
        return fail, float(fail.any())
    diff = (got.double() - c["S"]).abs()
    fail = ~(diff <= c["bound"])
    ratio = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff / c["bound"])
    fail[c["base"]] = ~same_base[c["base"]]
    ratio[c["base"]] = torch.where(same_base[c["base"]], 0.0, float("inf")).double()
    return fail, float(ratio.max())


def emulate(c, slip=None):
    """The kernels' arithmetic in fp32 on the CPU (see the module docstring); ``slip`` plants one of the
    mistakes the checker must reject."""
    x, K, R = c["x"].float(), c["K"], c["R"]
    idx = list(c["idx"])
    if slip == "neighbour_slot":
        idx[0] = idx[1]
    if slip == "touch_base":
        idx[c["base"].nonzero()[0, 0].item()] = 0
    y = c["y0"].clone()
    kblocks, ks = K // 128, splits(K, R)
    per = -(-kblocks // ks)
    for a in sorted(set(idx) - {-1}):
        rows = torch.tensor([i for i, v in enumerate(idx) if v == a])
        Aa, Ba, sc = c["A"][a].float(), c["B"][a].float(), c["scale"][a]
        total = None
        for z in range(ks):
            acc = torch.zeros(len(rows), R, dtype=torch.float32)
            for kb in range(min(z * per, kblocks), min(z * per + per, kblocks)):
                for j in range(4):  # MFMA j of a chunk: k = 128 kb + 32 g + 8 j + i, g < 4, i < 8
                    k = torch.tensor([128 * kb + 32 * g + 8 * j + i for g in range(4) for i in range(8)])
                    acc = acc + x[rows][:, k] @ Aa[:, k].t()
            if slip == "drop_range" and z == ks - 1:
                continue
            total = acc if total is None else total + acc
        t = total if slip == "t_unrounded" else total.bfloat16().float()
        acc = torch.zeros(len(rows), c["N"], dtype=torch.float32)
        for r0 in range(0, R, 32):
            acc = acc + t[:, r0:r0 + 32] @ Ba[:, r0:r0 + 32].t()
        y[rows] = (c["y0"][rows].float() + (acc if slip == "no_scale" else sc * acc)).bfloat16()
    return y


# ------------------------------------------------------------------------------- checker, reference
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_emulation_passes_every_gpu_case(kind):
    worst = 0.0
    for args in gpu_cases(kind):
        c = case(kind, *args)
        fail, share = fails(c, emulate(c))
        assert not fail.any(), (kind, args, int(fail.sum()), share)
        worst = max(worst, share)
    print(f"lora emulation {kind}: worst share of the bound {worst:.3f}")
    assert kind != "exact" or worst == 0.0


def test_gpu_cases_cover_the_shapes_patterns_and_both_split_counts():
    for kind in KINDS:
        cs = gpu_cases(kind)
        assert {c[0] for c in cs} == set(MS) and {c[4] for c in cs} == set(PATTERNS) and {c[3] for c in cs} == {*RS, 192}
        assert {(c[1], c[2]) for c in cs} == ({(16, 128)} if kind == "exact" else set(NKS))
    assert [splits(K, 16) for _, K in NKS] == [1, 1, 2] and splits(1152, 192) == 2
    assert splits(4096, 16) == 8 and splits(14336, 48) == 16 and splits(14336, 128) == 8  # R enters above 64
    idx = pattern_idx("big_and_single", 70)
    assert idx.count(0) == 69 and idx.count(1) == 1


@pytest.mark.parametrize("slip", ["drop_range", "no_scale", "t_unrounded", "neighbour_slot", "touch_base"])
def test_checker_rejects(slip):
    c = {"drop_range": case("coded", 5, 272, 1152, 32, "cycle"), "no_scale": case("coded", 5, 48, 384, 32, "cycle"),
         "t_unrounded": case("exact", 5, 16, 128, 32, "cycle"), "neighbour_slot": case("coded", 5, 48, 384, 32, "cycle"),
         "touch_base": case("coded", 5, 48, 384, 32, "base_mixed")}[slip]
    assert not fails(c, emulate(c))[0].any()
    fail, _ = fails(c, emulate(c, slip))
    assert fail.any(), slip
    if slip == "neighbour_slot":
        assert fail[0].any() and not fail[1:].any()
    if slip == "touch_base":
        assert fail[0].any() and not fail[1:].any()  # row 0 is the first base row


@pytest.mark.parametrize("kind", KINDS)
def test_reference_passes_the_bound_and_is_the_cpu_path_of_the_op(kind):
    for args in gpu_cases(kind)[::3]:
        c = case(kind, *args)
        routing = ops.lora_routing(c["idx"])
        y = c["y0"].clone()
        assert ops.lora_add_(y, c["x"], c["A"], c["B"], c["scale"], routing) is y
        assert not fails(c, y)[0].any(), (kind, args)
        y2 = c["y0"].clone()
        ref.lora_add_ref(y2, c["x"], c["A"], c["B"], c["scale"], routing.idx)
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
        assert not ops.lora_supported(c["M"], c["N"], c["K"], c["R"], y, c["x"], c["A"], c["B"], c["scale"])  # CPU
    c = case("coded", 5, 48, 384, 32, "cycle")
    with pytest.raises(ValueError):
        ops.lora_add_(c["y0"].clone(), c["x"][:, :128], c["A"], c["B"], c["scale"], ops.lora_routing(c["idx"]))
    with pytest.raises(ValueError):
        ops.lora_add_(c["y0"].clone(), c["x"], c["A"], c["B"], c["scale"], ops.lora_routing(c["idx"][:4]))


def test_routing_tiles():
    for M in MS + [200]:
        for pattern in PATTERNS:
            idx = pattern_idx(pattern, M)
            idx = [None if v < 0 and i % 3 == 0 else v for i, v in enumerate(idx)]  # None and -1 both mean base
            r = ops.lora_routing(idx)
            want = [-1 if v is None else v for v in idx]
            assert r.idx.dtype == torch.int32 and r.idx.tolist() == want and r.num_rows == M
            assert r.tile_slot.dtype == r.tile_rows.dtype == torch.int32 and tuple(r.tile_rows.shape) == (r.n_tiles, 16)
            seen = []
            for slot, rows in zip(r.tile_slot.tolist(), r.tile_rows.tolist()):
                real = [m for m in rows if m >= 0]
                assert 1 <= len(real) <= 16 and all(want[m] == slot for m in real) and slot >= 0
                assert rows[len(real):] == [-1] * (16 - len(real))
                seen += real
            assert sorted(seen) == [m for m, v in enumerate(want) if v >= 0]  # once each; base rows nowhere
            assert r.any == any(v >= 0 for v in want) == (r.n_tiles > 0)
    assert ops.lora_routing([0] * 33).n_tiles == 3 and ops.lora_routing([]).n_tiles == 0
    with pytest.raises(ValueError):
        ops.lora_routing([0, -2])


# ---------------------------------------------------------------------------------------- models
PROMPTS = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]
RANK = 4


class _RoundedTwin(torch.nn.Module):
    """One adapter applied by hand around a plain linear, with the contract's rounding of t."""

    def __init__(self, base, A, B, scale):
        super().__init__()
        self.base, self.A, self.B, self.scale = base, A, B, scale

    def forward(self, x):
        t = (x @ self.A.t()).bfloat16().float()
        return self.base(x) + self.scale * (t @ self.B.t())


@functools.lru_cache(maxsize=None)
def tiny():
    """fp32 llama3-tiny: the plain model, the LoRA-enabled copy with adapters ``a`` and ``b`` loaded, and
    the adapters."""
    torch.manual_seed(3)
    base = build_llama("llama3-tiny", dtype=torch.float32).eval()
    model = copy.deepcopy(base).enable_lora_(max_adapters=3, max_rank=RANK)
    ads = {"a": LoraAdapter.random(base.cfg, RANK, seed=1), "b": LoraAdapter.random(base.cfg, 2, seed=2, alpha=8)}
    for name, ad in ads.items():
        model.load_adapter(name, ad)
    return base, model, ads


def _twin(base, adapter):
    twin = copy.deepcopy(base)
    for (parent, t), lay in zip(lora_mod._targets(twin), (lay for lay in adapter.layers for _ in lora_mod.TARGETS)):
        setattr(parent, t, _RoundedTwin(getattr(parent, t), *lay[t]))
    # the twin's MLP takes down(swiglu(.)) as a LoRA model does
    for blk in twin.layers:
        blk.mlp.forward = (lambda mlp: lambda x: mlp.down(ops.swiglu(mlp.gate_up(x))))(blk.mlp)
    return twin


def _three_calls(model, prompts, **kw):
    cache = PagedKVCache(model.cfg, 32, 16, dtype=torch.float32)
    ids = list(range(len(prompts)))
    out = [model.prefill(prompts, None, cache, ids, **kw)]
    out.append(model.extend([[8, 2, 6], [1], [77, 78]][:len(prompts)], cache, ids, all_logits=True, **kw))
    out.append(model.decode_step([4, 5, 6][:len(prompts)], cache, ids, **kw))
    return out


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-4, atol=1e-4 * max(1.0, b.abs().max().item()))


def test_lora_model_equals_the_hand_applied_twin():
    base, model, ads = tiny()
    for name in ("a", "b"):
        twin = _twin(base, ads[name])
        got, want = _three_calls(model, PROMPTS, adapters=[name] * 3), _three_calls(twin, PROMPTS)
        plain = _three_calls(base, PROMPTS)
        for g, w, p in zip(got, want, plain):
            assert _close(g, w), (name, (g - w).abs().max().item())
            assert (g - p).abs().max().item() > 100 * (g - w).abs().max().item() + 1e-3  # the adapter does something


def test_mixed_batch_equals_single_sequence_runs():
    _, model, _ = tiny()
    names = ["a", None, "b"]
    mixed = _three_calls(model, PROMPTS, adapters=names)
    at = [0, 3, 4, 6]  # rows of the three sequences in the packed extend output
    for b, name in enumerate(names):
        kw = {} if name is None else {"adapters": [name]}
        cache = PagedKVCache(model.cfg, 32, 16, dtype=torch.float32)
        solo = [model.prefill([PROMPTS[b]], None, cache, [0], **kw),
                model.extend([[[8, 2, 6], [1], [77, 78]][b]], cache, [0], all_logits=True, **kw),
                model.decode_step([[4, 5, 6][b]], cache, [0], **kw)]
        assert _close(mixed[0][b:b + 1], solo[0]) and _close(mixed[2][b:b + 1], solo[2]), name
        assert _close(mixed[1][at[b]:at[b + 1]], solo[1]), name
    assert not _close(mixed[0][0:1], _three_calls(model, PROMPTS)[0][0:1])


def test_enabled_but_unused_is_the_plain_model_bit_for_bit():
    base, model, _ = tiny()
    assert isinstance(model.layers[0].attn.qkv, LoraLinear) and isinstance(model.layers[1].mlp.down, LoraLinear)
    assert model.lm_head is not None and not isinstance(model.lm_head, LoraLinear)
    for kw in ({}, {"adapters": [None] * 3}):
        for a, b in zip(_three_calls(model, PROMPTS, **kw), _three_calls(base, PROMPTS)):
            assert torch.equal(a, b)
    assert model.generate(PROMPTS, 6) == base.generate(PROMPTS, 6)
    assert model.generate(PROMPTS, 6, adapters=[None] * 3, prefill_chunk=4) == base.generate(PROMPTS, 6, prefill_chunk=4)
    with pytest.raises(RuntimeError, match="inference-only"):
        model(torch.tensor([[1, 2, 3]]))
    with pytest.raises(ValueError, match="not enabled"):
        base.generate(PROMPTS, 2, adapters=["a", None, None])
    assert base.loaded_adapters() == [] and not hasattr(base, "lora")
    # the bank is buffers: counted by weight_bytes, fp32 scale through casts
    cfg = base.cfg
    per_slot = sum((i + o) * model.lora.capacity(t) for t, (i, o) in lora_mod.target_dims(cfg).items())
    assert weight_bytes(model) - weight_bytes(base) == lora_mod.bank_bytes(model) == cfg.num_layers * 3 * (4 * per_slot + 16)
    assert model.lora.capacity("qkv") == 16 and copy.deepcopy(model).bfloat16().layers[0].attn.o.lora_scale.dtype == torch.float32


def test_quantise_and_enable_in_either_order():
    from ray_community_amd.models import QuantLinear

    base, _, ads = tiny()
    first = copy.deepcopy(base).quantize_weights_("fp8").enable_lora_(2, RANK)
    second = copy.deepcopy(base).enable_lora_(2, RANK).quantize_weights_("fp8")
    for m in (first, second):
        assert isinstance(m.layers[0].attn.qkv, LoraLinear) and isinstance(m.layers[0].attn.qkv.base, QuantLinear)
        m.load_adapter("a", ads["a"])
    for a, b in zip(_three_calls(first, PROMPTS, adapters=["a", None, "a"]), _three_calls(second, PROMPTS, adapters=["a", None, "a"])):
        assert torch.equal(a, b)


def test_from_peft_state_dict_places_q_k_v_block_diagonally(tmp_path):
    base, _, _ = tiny()
    cfg, r, alpha = base.cfg, 3, 6.0
    dims = lora_mod.part_dims(cfg)
    g = torch.Generator().manual_seed(9)
    sd, hand = {}, {}
    for i in range(cfg.num_layers):
        for p, mod in lora_mod._PEFT.items():
            if (i, p) in ((0, "k"), (1, "gate"), (1, "o")):
                continue  # missing projections contribute zeros
            a, b = torch.randn(r, dims[p][0], generator=g), torch.randn(dims[p][1], r, generator=g)
            prefix = "base_model.model.model." if i == 0 else ""
            sd[f"{prefix}layers.{i}.{mod}.lora_A.weight"], sd[f"{prefix}layers.{i}.{mod}.lora_B.weight"] = a, b
            hand[(i, p)] = (alpha / r) * (b @ a)
    ad = LoraAdapter.from_peft_state_dict(sd, cfg, alpha)
    for i, lay in enumerate(ad.layers):
        for t, parts in lora_mod.PARTS.items():
            A, B, scale = lay[t]
            assert A.shape[0] == r * len(parts) and scale == alpha / r
            delta, row = scale * (B @ A), 0
            for p in parts:  # q, k and v separately: each block of output rows sees its own projection only
                want = hand.get((i, p), torch.zeros(dims[p][1], dims[p][0]))
                assert torch.allclose(delta[row: row + dims[p][1]], want, rtol=1e-5, atol=1e-6), (i, p)
                row += dims[p][1]
    assert ad.layers[0]["qkv"][0].shape[0] == 3 * r and ad.layers[0]["gate_up"][0].shape[0] == 2 * r
    path = tmp_path / "ad.pt"
    ad.save(path)
    back = LoraAdapter.load(path)
    assert all(torch.equal(x, y) for la, lb in zip(ad.layers, back.layers) for t in la for x, y in zip(la[t][:2], lb[t][:2]))
    model = copy.deepcopy(base).enable_lora_(1, r)
    model.load_adapter("p", back)
    with pytest.raises(ValueError):
        LoraAdapter.from_peft_state_dict({"layers.0.self_attn.q_proj.weight": torch.zeros(2, 2)}, cfg, 1.0)
    with pytest.raises(ValueError):
        LoraAdapter.from_peft_state_dict({**sd, "layers.0.mlp.up_proj.lora_A.weight": torch.zeros(r + 1, 256)}, cfg, 1.0)


def test_load_and_unload_errors():
    base, _, ads = tiny()
    model = copy.deepcopy(base).enable_lora_(max_adapters=2, max_rank=RANK)
    assert model.load_adapter("a", ads["a"]) == 0 and model.load_adapter("b", ads["b"]) == 1
    assert model.loaded_adapters() == ["a", "b"]
    with pytest.raises(AdapterSlotsFull):
        model.load_adapter("c", ads["a"])
    with pytest.raises(ValueError, match="already loaded"):
        model.load_adapter("a", ads["a"])
    model.unload_adapter("a")
    assert model.loaded_adapters() == ["b"] and not model.layers[0].attn.qkv.lora_A[0].any()
    with pytest.raises(ValueError, match="rank"):
        model.load_adapter("big", LoraAdapter.random(base.cfg, RANK + 1))
    other = LoraAdapter.random(build_llama("llama3-tiny", dtype=torch.float32, intermediate_size=256).cfg, RANK)
    with pytest.raises(ValueError, match="do not fit"):
        model.load_adapter("other", other)
    with pytest.raises(ValueError, match="unknown adapter"):
        model.unload_adapter("a")
    with pytest.raises(ValueError, match="unknown adapter"):
        model.generate(PROMPTS, 2, adapters=["zzz", None, None])
    assert model.load_adapter("a2", ads["b"]) == 0  # the freed slot, its old rank zeroed
    assert torch.equal(model.layers[1].mlp.down.lora_A[0], model.layers[1].mlp.down.lora_A[1])
    with pytest.raises(ValueError, match="already enabled"):
        model.enable_lora_(2, 2)
    with pytest.raises(ValueError):
        model.prefill(PROMPTS, None, PagedKVCache(model.cfg, 32, 16, dtype=torch.float32), [0, 1, 2], adapters=["b"])


# ---------------------------------------------------------------------------------------- engine
def _engine_run(model, adapters, prefixes=None, **kw):
    eng = GenerationEngine(model, max_slots=4, num_blocks=64, **kw)
    rids = [eng.add_request(p, 8, **({} if a is None else {"adapter": a})) for p, a in zip(PROMPTS, adapters)]
    out = {r: [] for r in rids}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            out[rid].append(tok)
    assert eng.cache.num_free_blocks == 64
    return [out[r] for r in rids]


@pytest.mark.parametrize("kw", [{}, {"speculative": 3}, {"prefill_chunk": 5}, {"prefill_chunk": 5, "speculative": 3}])
def test_engine_per_request_adapters_give_the_generate_streams(kw):
    _, model, _ = tiny()
    names = ["a", None, "b"]
    gkw = {k: v for k, v in kw.items()}
    if "speculative" in kw:
        gkw["fused_sampling"] = True
    want = model.generate(PROMPTS, 8, adapters=names, **gkw)
    assert _engine_run(model, names, **kw) == want and all(len(t) == 8 for t in want)
    solo = [model.generate([p], 8, **({} if a is None else {"adapters": [a]}), **gkw)[0] for p, a in zip(PROMPTS, names)]
    assert want == solo
    assert want[0] != model.generate(PROMPTS, 8, **gkw)[0]  # adapter a changes the first stream


def test_engine_prefix_adapter_rules_and_unload_refusal():
    _, model, ads = tiny()
    model = copy.deepcopy(model)
    eng = GenerationEngine(model, max_slots=4, num_blocks=64, prefill_chunk=6)
    with pytest.raises(ValueError, match="unknown adapter"):
        eng.add_request([1, 2, 3], 2, adapter="zzz")
    with pytest.raises(ValueError, match="unknown adapter"):
        eng.register_prefix([1, 2, 3], adapter="zzz")
    head = [7] * 20
    h_a, h_none = eng.register_prefix(head, adapter="a"), eng.register_prefix(head)
    for handle, bad in ((h_a, None), (h_a, "b"), (h_none, "a")):
        with pytest.raises(ValueError, match="prefix"):
            eng.add_request([1, 2, 3], 2, prefix=handle, **({} if bad is None else {"adapter": bad}))
    assert not eng.has_work()
    r_a = eng.add_request([1, 2, 3], 5, prefix=h_a, adapter="a")
    r_n = eng.add_request([1, 2, 3], 5, prefix=h_none)
    r_b = eng.add_request([9, 9], 5, adapter="b")
    assert eng.adapter_users("a") == 2 and eng.adapter_users("b") == 1
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("b")
    out = {}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            out.setdefault(rid, []).append(tok)
    assert out[r_a] == model.generate([head + [1, 2, 3]], 5, adapters=["a"])[0]
    assert out[r_n] == model.generate([head + [1, 2, 3]], 5)[0] != out[r_a]
    assert out[r_b] == model.generate([[9, 9]], 5, adapters=["b"])[0]
    eng.unload_adapter("b")  # its request is over
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("a")  # the registered prefix still uses it
    eng.release_prefix(h_a)
    eng.unload_adapter("a")
    assert model.loaded_adapters() == []
    eng.load_adapter("c", ads["b"])
    assert eng.add_request([9, 9], 1, adapter="c") is not None


def test_requests_without_an_adapter_make_todays_calls(monkeypatch):
    base, model, _ = tiny()
    trace = {}

    def spy(key, name, real):
        def wrapper(self, *a, **kw):
            trace[key].append((name, len(a), sorted(kw)))
            return real(self, *a, **kw)
        return wrapper

    def run(key, m):
        trace[key] = []
        with monkeypatch.context() as patch:
            for name in ("prefill", "decode_step", "extend"):
                patch.setattr(type(m), name, spy(key, name, getattr(type(m), name)))
            return _engine_run(m, [None] * 3, speculative=3), _engine_run(m, [None] * 3, prefill_chunk=5)

    assert run("lora", model) == run("plain", base)
    assert trace["lora"] == trace["plain"] and not any("adapters" in kw for _, _, kw in trace["lora"])
    trace["named"] = []
    with monkeypatch.context() as patch:
        for name in ("prefill", "decode_step", "extend"):
            patch.setattr(type(model), name, spy("named", name, getattr(type(model), name)))
        _engine_run(model, ["a", None, None], speculative=3)
    assert all("adapters" in kw for _, _, kw in trace["named"])
