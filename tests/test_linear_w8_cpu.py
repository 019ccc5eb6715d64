"""FP8 weights (ops.linear_w8, models.QuantLinear, Llama.quantize_weights_) without a GPU: the weight
quantiser, the module, quantised tiny models against fake-quant twins, and the cases, float64 oracle,
bound checker and fp32 emulation that tests/test_linear_w8_gpu.py runs the kernel through.

Oracle and bound (the ``plain`` bound of tests/test_gemm_rows_gpu.py, same derivation): with X64 the
bf16 activations and W64 = Q64 * s the exactly known weight values (an e4m3 byte times a power of two),
S = X64 W64^T and P = |X64| |W64|^T in float64, and per element
    |got - S| <= 2**-8 |S| + K 2**-24 P + TINY max(1, magnitude)
2**-8 |S| is half a bf16 ulp of the one rounding, K 2**-24 P the fp32 accumulation bound, TINY = 2**-126;
the power-of-two scale adds no rounding. Nothing in it is taken from a kernel.

The emulation follows ops/csrc/linear_w8.hip: K is cut into ``splits(N, K)`` ranges of 128-deep blocks
(a mirror of the kernel's rule, compared with the library's on the GPU), every range is summed in fp32
in 32-deep groups (one MFMA each), the partials are added in range order, multiplied by s[n] and rounded
once to bf16. Worst share of the bound over every GPU case: printed by
``test_fp32_emulation_passes_every_gpu_case`` (coded 0.976, binades 0.958, nonfinite 0.959, set by the
rounding term; ``exact`` is bit for bit; M=5, N=48, K=384 coded: 0.896).
"""
import copy
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import GenerationEngine, QuantLinear, build_llama, quantize_weights_, weight_bytes
from ray_community_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn
TINY = 2.0 ** -126
NAN = float("nan")
PADS = [(8, 0), (72, 8), (264, 64)]  # (row stride - cols, c0), as tests/test_gemm_rows_gpu.py
MS = sorted({1, 2, 5, 16, 17, 32, 33, ops.M_SKINNY})
NS = [16, 48, 272]
KS = [128, 384, 1152]
KINDS = ["coded", "exact", "binades", "nonfinite"]


def kind_shapes(kind):
    return [(M, N, K) for M in MS for N in NS for K in KS if kind != "exact" or K <= 256]


def splits(N, K):
    """Mirror of w8_splits (ops/csrc/linear_w8.hip): a function of N and K only."""
    blocks, kblocks, ks = (N + 63) // 64, K // 128, 1
    while ks < 8 and blocks * ks < 512 and ks * 2 * 4 <= kblocks:
        ks *= 2
    return ks


def _gen(*ints):
    seed = 0
    for v in ints:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def case(kind, M, N, K):
    """x [M, K] bf16, q [N, K] e4m3, s [N] fp32 on the CPU, plus the float64 oracle."""
    g = _gen(KINDS.index(kind), M, N, K)
    m = torch.arange(M, dtype=torch.float64)[:, None]
    n = torch.arange(N, dtype=torch.float64)[:, None]
    k = torch.arange(K, dtype=torch.float64)[None, :]
    if kind == "exact":
        assert K <= 256
        x = torch.randint(-1, 2, (M, K), generator=g).double() * 2.0 ** (m % 7 - 3)
        w = torch.randint(-1, 2, (N, K), generator=g).double() * 2.0 ** (n % 5)
    else:
        x, w = torch.randn(M, K, generator=g).double(), torch.randn(N, K, generator=g).double()
        if kind == "binades":
            w = w / w.abs().amax(-1, keepdim=True) * 3.0  # one amax for every row: the scales follow 2^e alone
            x, w = x * 2.0 ** (m % 13 - 6), w * 2.0 ** (n % 41 - 20)
        else:
            x = x + 0.5 * torch.sin(0.37 * m + 0.11 * k)
            w = w - 0.4 * torch.cos(0.23 * n + 0.05 * k) + 0.3 * torch.sin(0.7 * n)
    x = x.bfloat16()
    q, s = ref.quantize_weight_fp8_ref(w.float())
    c = dict(kind=kind, M=M, N=N, K=K)
    if kind == "exact":
        assert torch.equal(ref.kv_dequantize_fp8_ref(q, s, torch.float64), w) and torch.equal(x.double(), x.double())
    if kind == "nonfinite":
        qb = q.view(torch.uint8)
        qb[(qb & 0x7F) == 0] = 0x08  # no zero weight: inf * 0 is out of the picture
        x[x == 0] = 1.0
        c.update(mi=M - 1, ki=K - 5, mn=0, kn=3)
        x[c["mi"], c["ki"]] = float("inf")
        x[c["mn"], c["kn"]] = NAN  # M = 1: the same row holds both and is all NaN
    W64 = q.double() * s.double()[:, None]
    assert torch.isfinite(W64).all()
    X64 = x.double()
    clean = torch.where(torch.isfinite(X64), X64, torch.ones_like(X64))
    c.update(x=x, q=q, s=s, W64=W64, S=clean @ W64.t(), P=clean.abs() @ W64.abs().t(),
             mag=max(clean.abs().max().item(), W64.abs().max().item()))
    if kind == "nonfinite":
        c["S_nf"] = (X64[:, None, :] * W64[None, :, :]).sum(-1)  # elementwise: no BLAS shortcuts around inf / NaN
        bad = ~torch.isfinite(c["S_nf"])
        rows = sorted({c["mi"], c["mn"]})
        assert bad[rows].all() and not bad[[r for r in range(M) if r not in rows]].any()
    if kind == "binades":
        assert len(set(s[:41].tolist())) == min(N, 41)
    return c


def fails(c, got):
    """[M][N] bool, True where ``got`` (bf16, CPU) is rejected, and the worst share of the bound."""
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (c["M"], c["N"])
    S, g64 = c["S"], got.double()
    if c["kind"] == "exact":
        assert torch.equal(S.bfloat16().double(), S)
        fail = got.contiguous().view(torch.int16) != S.bfloat16().view(torch.int16)
        return fail, float(fail.any())
    bound = 2.0 ** -8 * S.abs() + c["K"] * 2.0 ** -24 * c["P"] + TINY * max(1.0, c["mag"])
    diff = (g64 - S).abs()
    fail = ~(diff <= bound)
    ratio = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff / bound)
    if c["kind"] == "nonfinite":
        want = c["S_nf"]
        bad = ~torch.isfinite(want)
        same = (torch.isnan(want) & torch.isnan(g64)) | (torch.isinf(want) & (g64 == want))
        fail = torch.where(bad, ~same, fail)
        ratio = torch.where(bad, torch.zeros_like(ratio), ratio)
    return fail, float(ratio.max())


def emulate(c, slip=None):
    """The kernel's arithmetic in fp32 on the CPU (see the module docstring); ``slip`` plants one
    of the mistakes the checker must reject."""
    x, q, s, N, K = c["x"].float(), c["q"], c["s"], c["N"], c["K"]
    w = q.float()
    if slip == "fnuz":
        w = torch.nan_to_num(q.view(torch.uint8).view(torch.float8_e4m3fnuz).float(), nan=0.0)
    if slip == "drop_last_block":
        K -= 128
    if slip == "row_from_next":
        x = torch.cat([x[1:2], x[1:]])  # row 0 computed from row 1's activations
    kblocks, ks = K // 128, splits(N, c["K"])
    per = -(-(c["K"] // 128) // ks)
    total = None
    for z in range(ks):
        acc = torch.zeros(x.shape[0], N, dtype=torch.float32)
        for kb in range(min(z * per, kblocks), min(z * per + per, kblocks)):
            for j in range(4):  # MFMA j of a chunk: k = 128 kb + 32 g + 8 j + i, g < 4, i < 8
                idx = torch.tensor([128 * kb + 32 * g + 8 * j + i for g in range(4) for i in range(8)])
                acc = acc + x[:, idx] @ w[:, idx].t()
        if slip == "double_rounding":
            acc = acc.bfloat16().float()
        total = acc if total is None else total + acc
    if slip == "scale_of_neighbour":
        s = torch.roll(s, 1)
    return (total * s[None, :]).bfloat16()


# ------------------------------------------------------------------------------------- quantiser
def weight_rows(K, seed=0):
    """fp32 rows [R, K]: N(0, 1) times 2^e for e in -20..20, a zero row, rows whose amax is exactly
    448 * 2^k and rows whose amax is the next bf16 above it (450 * 2^k)."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(K, generator=g) * 2.0 ** e for e in range(-20, 21)]
    rows.append(torch.zeros(K))
    for k in (-20, -3, 0, 7):
        for top in (448.0, 450.0):
            r = (torch.rand(K, generator=g) * 2 - 1) * 440.0
            r[int(torch.randint(K, (1,), generator=g))] = -top if k % 2 else top
            rows.append(r * 2.0 ** k)
    return torch.stack(rows).bfloat16().float()


def test_weight_quantiser_properties():
    w = weight_rows(128)
    q, s = ref.quantize_weight_fp8_ref(w)
    assert q.dtype == FP8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (w.shape[0],)
    amax = w.abs().amax(-1)
    mant, _ = torch.frexp(s)
    assert (mant == 0.5).all(), "scales are powers of two"
    zero = amax == 0
    assert int(zero.sum()) == 1 and (s[zero] == 1).all() and (q.float()[zero] == 0).all()
    ratio = amax[~zero] / s[~zero]
    assert (ratio > 224).all() and (ratio <= 448).all()
    qmax = q.float().abs().amax(-1) * s
    # the largest element is rounded to 4 significant bits: half an e4m3 ulp, 2**-4 relative
    assert ((qmax - amax).abs() <= 2.0 ** -4 * amax).all()
    for dt in (torch.bfloat16, torch.float32):
        d = ref.kv_dequantize_fp8_ref(q, s, dt)
        assert d.dtype == dt and torch.equal(d.double(), q.double() * s.double()[:, None]), dt
    with pytest.raises(ValueError):
        ref.quantize_weight_fp8_ref(torch.zeros(4))


def test_linear_w8_reference_path_and_contract_predicate():
    c = case("coded", 5, 48, 384)
    y = ops.linear_w8(c["x"], c["q"], c["s"])
    assert y.dtype == torch.bfloat16 and torch.equal(y, ref.linear_w8_ref(c["x"], c["q"], c["s"]))
    assert torch.equal(ops.linear_w8(c["x"], c["q"].view(torch.uint8), c["s"]), y)
    assert torch.equal(ops.linear_w8(c["x"].view(1, 5, 384), c["q"], c["s"]), y.view(1, 5, 48))
    out = torch.zeros(5, 48, dtype=torch.bfloat16)
    assert ops.linear_w8(c["x"], c["q"], c["s"], out=out) is out and torch.equal(out, y)
    assert not ops.linear_w8_supported(5, 48, 384, c["x"], c["q"], c["s"])  # CPU tensors
    assert torch.equal(ops.dequant_w8(c["q"], c["s"]), ref.kv_dequantize_fp8_ref(c["q"], c["s"]))
    with pytest.raises(ValueError):
        ops.linear_w8(c["x"][:, :128], c["q"], c["s"])
    assert not fails(c, y)[0].any()


# ------------------------------------------------------------------------------------- emulation
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_emulation_passes_every_gpu_case(kind):
    worst = 0.0
    for M, N, K in kind_shapes(kind):
        if M not in (1, 5, 33) and (N, K) != (48, 384):
            continue  # rows are independent: every (N, K) at three M, every M at one (N, K)
        c = case(kind, M, N, K)
        fail, share = fails(c, emulate(c))
        assert not fail.any(), (kind, M, N, K, int(fail.sum()), share)
        worst = max(worst, share)
    print(f"linear_w8 emulation {kind}: worst share of the bound {worst:.3f}")
    assert kind != "exact" or worst == 0.0
    c = case("coded", 5, 48, 384)
    print(f"coded M=5 N=48 K=384: {fails(c, emulate(c))[1]:.3f}")


def test_splits_cover_both_epilogues_and_a_multi_tile_loop():
    assert [splits(N, K) for N in NS for K in KS] == [1, 1, 2] * 3  # direct and split, 1 to 3 LDS tiles a range
    assert splits(4096, 4096) == 8 and splits(4096, 14336) == 8 and splits(28672, 4096) == 2
    assert splits(128256, 4096) == 1 and splits(2048, 2048) == 4


@pytest.mark.parametrize("slip", ["scale_of_neighbour", "drop_last_block", "fnuz", "row_from_next", "double_rounding"])
def test_checker_rejects(slip):
    kind = "binades" if slip == "scale_of_neighbour" else "coded"
    c = case(kind, 5, 48, 1152 if slip == "double_rounding" else 384)
    assert not fails(c, emulate(c))[0].any()
    fail, _ = fails(c, emulate(c, slip))
    assert fail.any(), slip
    if slip == "scale_of_neighbour":
        assert fail.all()  # every s[n] differs from its neighbour's by a factor of two or more
    if slip == "row_from_next":
        assert fail[0].any() and not fail[1:].any()


def test_nonfinite_checker_wants_the_exact_pattern():
    c = case("nonfinite", 5, 48, 384)
    good = emulate(c)
    assert not fails(c, good)[0].any()
    assert torch.isnan(good[c["mn"]]).all() and torch.isinf(good[c["mi"]]).all()
    for row, value in ((c["mi"], NAN), (c["mn"], float("inf")), (c["mi"], 1.0), (1, NAN)):
        bad = good.clone()
        bad[row, 7] = value
        assert fails(c, bad)[0][row, 7]
    flipped = good.clone()
    flipped[c["mi"]] = -flipped[c["mi"]]
    assert fails(c, flipped)[0][c["mi"]].all()
    one = case("nonfinite", 1, 48, 384)
    assert torch.isnan(one["S_nf"]).all() and not fails(one, emulate(one))[0].any()


# ---------------------------------------------------------------------------------------- module
def test_quant_linear_survives_casts_and_moves():
    torch.manual_seed(0)
    w = weight_rows(128)[:48]
    lin = QuantLinear.from_weight(w)
    assert lin.qweight.dtype == torch.uint8 and lin.scale.dtype == torch.float32 and not list(lin.parameters())
    assert torch.equal(lin.dequantized(torch.float32), ref.kv_dequantize_fp8_ref(*ref.quantize_weight_fp8_ref(w),
                                                                                 torch.float32))
    x = torch.randn(5, 128).bfloat16()
    with torch.no_grad():
        want = lin(x)
        q0, s0 = lin.qweight.clone(), lin.scale.clone()
        for move in (lambda m: m.to(torch.float32), lambda m: m.bfloat16(), lambda m: m.half(), lambda m: m.to("cpu"),
                     lambda m: m.to(dtype=torch.bfloat16)):
            lin = move(lin)
            assert lin.qweight.dtype == torch.uint8 and lin.scale.dtype == torch.float32
            assert torch.equal(lin.qweight, q0) and torch.equal(lin.scale, s0) and torch.equal(lin(x), want)
    with pytest.raises(RuntimeError, match="inference-only"):
        lin(x)


# ---------------------------------------------------------------------------------------- models
@functools.lru_cache(maxsize=None)
def tiny_pair(tied):
    """(bf16-free) fp32 llama3-tiny: the quantised model, its fake-quant twin (ordinary linears holding
    the dequantised values, exact in fp32) and the unquantised original's weight bytes."""
    torch.manual_seed(3)
    base = build_llama("llama3-tiny", dtype=torch.float32, tie_embeddings=tied).eval()
    quant = copy.deepcopy(base).quantize_weights_("fp8")
    twin = copy.deepcopy(base)
    with torch.no_grad():
        for (name, a), (_, b) in zip(quant.named_modules(), twin.named_modules()):
            if isinstance(a, QuantLinear) and name != "lm_head":
                b.weight.copy_(a.dequantized(torch.float32))
        if tied:  # the twin's head is the dequantised fp8 copy of the embedding; its lookup stays as it was
            twin.logits = lambda h: torch.nn.functional.linear(h, quant.lm_head.dequantized(torch.float32))
        else:
            twin.lm_head.weight.copy_(quant.lm_head.dequantized(torch.float32))
    return quant, twin, weight_bytes(base)


PROMPTS = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]


@pytest.mark.parametrize("tied", [False, True])
def test_quantised_tiny_model_equals_its_fake_quant_twin(tied):
    from ray_community_amd.models.kv_cache import PagedKVCache

    quant, twin, _ = tiny_pair(tied)
    assert isinstance(quant.lm_head, QuantLinear) and isinstance(quant.layers[1].mlp.down, QuantLinear)
    assert quant.embed.weight.dtype == torch.float32 and torch.equal(quant.embed.weight, twin.embed.weight)
    outs = []
    for model in (quant, twin):
        cache = PagedKVCache(model.cfg, 32, 16, dtype=torch.float32)
        ids = ["a", "b", "c"]
        got = [model.prefill(PROMPTS, None, cache, ids)]
        got.append(model.extend([[8, 2, 6], [1], [77, 78]], cache, ids, all_logits=True))
        got.append(model.decode_step([4, 5, 6], cache, ids))
        got.append(model.generate(PROMPTS, 6))
        got.append(model.generate(PROMPTS, 6, temperature=0.8, top_k=20, seed=5, prefill_chunk=4))
        outs.append(got)
    for a, b in zip(*outs):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert torch.isfinite(outs[0][0]).all()


@pytest.mark.parametrize("tied", [False, True])
def test_quantised_engine_streams_and_speculation(tied):
    quant, twin, _ = tiny_pair(tied)

    def run(model, **kw):
        eng = GenerationEngine(model, max_slots=4, num_blocks=48, **kw)
        rids = [eng.add_request(p, 8, temperature=0.7, top_p=0.9, seed=11 + i) for i, p in enumerate(PROMPTS)]
        out = {r: [] for r in rids}
        while eng.has_work():
            for rid, tok, _ in eng.step():
                out[rid].append(tok)
        return [out[r] for r in rids]

    fused = run(quant, fused_sampling=True)
    assert fused == run(twin, fused_sampling=True) and all(len(t) == 8 for t in fused)
    assert run(quant, fused_sampling=True, speculative=3) == fused
    assert quant.generate(PROMPTS, 8, fused_sampling=True, speculative=3) == quant.generate(PROMPTS, 8,
                                                                                            fused_sampling=True)


@pytest.mark.parametrize("tied", [False, True])
def test_weight_bytes_state_dict_and_gradients(tied):
    quant, twin, before = tiny_pair(tied)
    cfg = quant.cfg
    H, I, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_layers
    rows = L * ((cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim + H + 2 * I + H)  # output rows of the layers' linears
    elems = L * (H * (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim + H * H + 2 * I * H + I * H)
    if tied:  # the fp8 copy of the embedding is added, nothing leaves
        want = before - 4 * elems + (elems + V * H) + 4 * (rows + V)
    else:
        want = before - 4 * (elems + V * H) + (elems + V * H) + 4 * (rows + V)
    assert weight_bytes(quant) == want
    sd = quant.state_dict()
    assert sd["layers.0.attn.qkv.qweight"].dtype == torch.uint8 and sd["lm_head.scale"].dtype == torch.float32
    assert not any(k.endswith("qkv.weight") or k.endswith("down.weight") for k in sd)
    torch.manual_seed(99)
    other = build_llama("llama3-tiny", dtype=torch.float32, tie_embeddings=tied, weight_dtype="fp8").eval()
    assert not torch.equal(other.layers[0].attn.qkv.qweight, quant.layers[0].attn.qkv.qweight)
    other.load_state_dict(sd)
    assert other.generate(PROMPTS, 4) == quant.generate(PROMPTS, 4)
    assert quantize_weights_(other, "fp8") is other and other.quantize_weights_("fp8") is other  # idempotent
    assert weight_bytes(other) == want
    for bad in ("int8", "fp4", "bf16"):
        with pytest.raises(ValueError):
            other.quantize_weights_(bad)
    assert weight_bytes(copy.deepcopy(twin).quantize_weights_(None)) == before
    with pytest.raises(RuntimeError, match="inference-only"):
        quant(torch.tensor([[1, 2, 3]]))
