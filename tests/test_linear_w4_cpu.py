"""MXFP4 weights (ops.linear_w4, models.QuantLinear("mxfp4"), Llama.quantize_weights_("mxfp4")) without a
GPU: the quantiser's rule, the op's reference path, the module, quantised tiny models against fake-quant
twins, the byte count and the Serve knob. The kernel's tests are in tests/test_linear_w4_gpu.py."""
import asyncio
import copy

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import QuantLinear, build_llama, weight_bytes
from ray_community_amd.ops import reference as ref
from test_linear_w8_cpu import PROMPTS, fails, weight_rows

GRID = torch.tensor(ref.MXFP4_VALUES)


def test_quantiser_properties():
    # grid values times a power of two round-trip exactly: every code in every block, scales from the clamp up
    c = torch.arange(64)
    exps = torch.cat([torch.arange(-125, 125, 6), torch.tensor([0, 1, -1])])[:, None] + c[None, :] // 32
    w = (GRID[c % 8] * (1 - 2 * ((c // 8) % 2))).double()[None, :] * 2.0 ** exps.double()
    q, e = ref.quantize_weight_mxfp4_ref(w.float())
    assert q.dtype == e.dtype == torch.uint8 and q.shape == (45, 32) and e.shape == (45, 2)
    assert torch.equal(e.long(), exps[:, ::32] + 127) and e.min() == 2  # a block's amax is 6 * 2^exps
    for dt in (torch.bfloat16, torch.float32, torch.float64):
        assert torch.equal(ref.dequantize_mxfp4_ref(q, e, dt).double(), w), dt
    assert q[0, :6].tolist() == [0x10, 0x32, 0x54, 0x76, 0x90, 0xBA]  # low nibble first; -0 is stored as +0

    w = weight_rows(128)
    w[3, 32:64] = 0
    q, e = ref.quantize_weight_mxfp4_ref(w)
    blocks, s = w.view(-1, 4, 32), 2.0 ** (e.float() - 127)
    amax, d = blocks.abs().amax(-1), ref.dequantize_mxfp4_ref(q, e, torch.float32).view(-1, 4, 32)
    zero = amax == 0
    assert e[3, 1] == 127 and (e[zero] == 127).all() and (d[zero] == 0).all() and int(zero.sum()) == 5
    assert ((amax / s)[~zero] <= 6).all() and ((amax / s)[~zero] > 3).all()  # the smallest such power of two
    assert ((blocks - d).abs() <= s[..., None]).all()  # half the widest e2m1 gap (2) times the scale
    assert ((d.abs() / s[..., None]).amax(-1)[~zero] >= 3).all()  # amax / s in (3, 6] rounds to 3, 4 or 6
    for bad in (torch.zeros(4, 48), torch.zeros(64)):
        with pytest.raises(ValueError):
            ref.quantize_weight_mxfp4_ref(bad)
    # ties go to the even code
    q, _ = ref.quantize_weight_mxfp4_ref(torch.tensor([[6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -5.0] + [0.0] * 23]))
    assert ref.dequantize_mxfp4_ref(q, torch.tensor([[127]], dtype=torch.uint8), torch.float32)[0, :9].tolist() == \
        [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -4.0]


def test_linear_w4_reference_path_and_contract_predicate():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 256, generator=g).bfloat16()
    q, e = ref.quantize_weight_mxfp4_ref(torch.randn(48, 256, generator=g))
    y = ops.linear_w4(x, q, e)
    assert y.dtype == torch.bfloat16 and torch.equal(y, ref.linear_w4_ref(x, q, e))
    assert torch.equal(ops.linear_w4(x.view(1, 5, 256), q, e), y.view(1, 5, 48))
    out = torch.zeros(5, 48, dtype=torch.bfloat16)
    assert ops.linear_w4(x, q, e, out=out) is out and torch.equal(out, y)
    assert not ops.linear_w4_supported(5, 48, 256, x, q, e)  # CPU tensors
    assert torch.equal(ops.dequant_w4(q, e), ref.dequantize_mxfp4_ref(q, e))
    for bad in (lambda: ops.linear_w4(x[:, :128], q, e), lambda: ops.linear_w4(x, q, e[:, :4]),
                lambda: ops.linear_w4(x, q, e.float())):
        with pytest.raises(ValueError):
            bad()
    W64, X64 = ref.dequantize_mxfp4_ref(q, e, torch.float64), x.double()
    c = dict(kind="coded", M=5, N=48, K=256, S=X64 @ W64.t(), P=X64.abs() @ W64.abs().t(), mag=6.0)
    assert not fails(c, y)[0].any()


def test_quant_linear_mxfp4_survives_casts_copies_and_state_dicts():
    w = weight_rows(128)[:48]
    lin = QuantLinear.from_weight(w, "mxfp4")
    assert lin.qweight.dtype == lin.scale.dtype == torch.uint8 and not list(lin.parameters())
    assert lin.qweight.shape == (48, 64) and lin.scale.shape == (48, 4) and "mxfp4" in repr(lin)
    want_w = ref.dequantize_mxfp4_ref(*ref.quantize_weight_mxfp4_ref(w), torch.float32)
    x = torch.randn(5, 128, generator=torch.Generator().manual_seed(1)).bfloat16()
    with torch.no_grad():
        want = lin(x)
        for move in (lambda m: m.to(torch.bfloat16), lambda m: m.half(), copy.deepcopy, lambda m: m.to(torch.float32)):
            lin = move(lin)
            assert lin.qweight.dtype == lin.scale.dtype == torch.uint8 and lin.weight_format == "mxfp4"
            assert torch.equal(lin.dequantized(torch.float32), want_w) and torch.equal(lin(x), want)
        other = QuantLinear(128, 48, weight_format="mxfp4")
        assert (other.dequantized(torch.float32) == 0).all()
        other.load_state_dict(lin.state_dict())
        assert torch.equal(other(x), want)
    with pytest.raises(RuntimeError, match="inference-only"):
        lin(x)
    with pytest.raises(ValueError):
        QuantLinear(128, 48, weight_format="fp4")


@pytest.mark.parametrize("tied", [False, True])
def test_quantised_tiny_model_generates_its_fake_quant_twins_tokens_and_counts_its_bytes(tied):
    torch.manual_seed(3)
    base = build_llama("llama3-tiny", dtype=torch.float32, tie_embeddings=tied).eval()
    quant = copy.deepcopy(base)
    epoch = quant.module_epoch
    assert quant.quantize_weights_("mxfp4") is quant and quant.weight_dtype == "mxfp4" and quant.module_epoch > epoch
    twin = copy.deepcopy(base)
    with torch.no_grad():
        for (name, a), (_, b) in zip(quant.named_modules(), twin.named_modules()):
            if isinstance(a, QuantLinear) and name != "lm_head":
                assert a.weight_format == "mxfp4"
                b.weight.copy_(a.dequantized(torch.float32))
        head = quant.lm_head.dequantized(torch.float32)
        if tied:  # the twin's head is the dequantised copy of the embedding; its lookup stays as it was
            twin.logits = lambda h: torch.nn.functional.linear(h, head)
        else:
            twin.lm_head.weight.copy_(head)
    assert torch.equal(quant.embed.weight, base.embed.weight)
    assert quant.generate(PROMPTS, 6) == twin.generate(PROMPTS, 6)
    kw = dict(temperature=0.8, top_k=20, seed=5, prefill_chunk=4)
    assert quant.generate(PROMPTS, 6, **kw) == twin.generate(PROMPTS, 6, **kw)

    cfg = quant.cfg
    H, I, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_layers
    elems = L * (H * (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim + H * H + 2 * I * H + I * H)
    quantised = elems + V * H
    gone = 4 * (elems if tied else quantised)  # tied: the fp32 embedding stays for the lookup
    assert weight_bytes(quant) == weight_bytes(base) - gone + quantised // 2 + quantised // 32
    assert quant.quantize_weights_("mxfp4") is quant and weight_bytes(quant) == weight_bytes(base) - gone + quantised * 17 // 32
    with pytest.raises(RuntimeError, match="already mxfp4"):
        quant.quantize_weights_("fp8")
    with pytest.raises(RuntimeError, match="already fp8"):
        copy.deepcopy(base).quantize_weights_("fp8").quantize_weights_("mxfp4")
    with pytest.raises(ValueError):
        copy.deepcopy(base).quantize_weights_("fp4")
    built = build_llama("llama3-tiny", dtype=torch.float32, tie_embeddings=tied, weight_dtype="mxfp4").eval()
    built.load_state_dict(quant.state_dict())
    assert built.state_dict()["layers.0.attn.qkv.scale"].dtype == torch.uint8
    assert built.generate(PROMPTS, 4) == quant.generate(PROMPTS, 4)


def test_serve_status_reports_mxfp4_weights():
    from ray_community_amd.serve.llm import LlamaDeployment

    dep = LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", max_slots=2, num_blocks=16, weight_dtype="mxfp4")
    st = asyncio.run(dep.status())
    assert dep.model.lm_head.weight_format == "mxfp4"
    assert st["weight_dtype"] == "mxfp4" and st["weight_bytes"] == weight_bytes(dep.model)
