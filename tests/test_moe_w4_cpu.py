"""MXFP4 expert weights without a GPU: ``mixtral-tiny`` in fp32 on the reference (ops/reference.py), and Serve."""
import asyncio
import copy

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import build_llama, weight_bytes
from ray_community_amd.ops import reference as ref
from ray_community_amd.serve.llm import LlamaDeployment

PROMPTS = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]
L, E, H, I = 2, 4, 256, 512  # mixtral-tiny


@pytest.fixture(scope="module")
def pair():
    """(the model with its experts' weights replaced by their dequantised values, the quantised model)."""
    torch.manual_seed(0)
    deq = build_llama("mixtral-tiny", dtype=torch.float32).eval()
    quant = copy.deepcopy(deq).quantize_experts_("mxfp4")
    with torch.no_grad():
        for blk in deq.layers:
            for w in (blk.mlp.w_gate_up, blk.mlp.w_down):
                q, s = ref.quantize_experts_mxfp4_ref(w)
                w.copy_(ref.dequantize_mxfp4_ref(q.flatten(0, 1), s.flatten(0, 1), torch.float32).view_as(w))
    return deq, quant


def test_quantize_experts_replaces_the_parameters_and_keeps_the_logits(pair):
    deq, quant = pair
    mlp = quant.layers[0].mlp
    shapes = {"q_gate_up": (E, 2 * I, H // 2), "s_gate_up": (E, 2 * I, H // 32), "q_down": (E, H, I // 2), "s_down": (E, H, I // 32)}
    assert {n: tuple(b.shape) for n, b in mlp.named_buffers()} == shapes and all(b.dtype == torch.uint8 for b in mlp.buffers())
    assert [n for n, _ in mlp.named_parameters()] == ["router.weight"] and quant.expert_dtype == "mxfp4"
    epoch = quant.module_epoch
    assert quant.quantize_experts_("mxfp4") is quant and quant.quantize_experts_(None) is quant  # idempotent
    assert quant.module_epoch == epoch + 1 and {n: tuple(b.shape) for n, b in mlp.named_buffers()} == shapes
    tokens = torch.tensor([p[:4] for p in PROMPTS])
    with torch.no_grad():
        assert torch.equal(quant(tokens), deq(tokens))
    with pytest.raises(RuntimeError, match="inference-only"):
        quant(tokens)
    want = quant.generate(PROMPTS, 6)
    assert want == deq.generate(PROMPTS, 6) == quant.generate(PROMPTS, 6, prefill_chunk=5)
    fresh = build_llama("mixtral-tiny", dtype=torch.float32, expert_dtype="mxfp4").eval()  # other weights
    fresh.load_state_dict(quant.state_dict())
    assert fresh.generate(PROMPTS, 6) == want


def test_weight_bytes_and_what_is_still_refused(pair):
    bf16 = build_llama("mixtral-tiny")
    before = weight_bytes(bf16)
    assert 32 * (before - weight_bytes(bf16.quantize_experts_("mxfp4"))) == L * E * 3 * H * I * (64 - 17)  # 2 - 17/32 bytes
    quant = pair[1]
    for dtype in ("fp8", "mxfp4"):
        with pytest.raises(NotImplementedError, match="MoE"):
            quant.quantize_weights_(dtype)
    with pytest.raises(NotImplementedError, match="MoE"):
        quant.enable_lora_(2, 4)
    with pytest.raises(ValueError, match="expert dtype"):
        quant.quantize_experts_("fp8")
    with pytest.raises(ValueError, match="MoE"):
        build_llama("llama3-tiny", dtype=torch.float32).quantize_experts_("mxfp4")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_forms_agree(pair, dtype):
    deq, quant = (m.layers[1].mlp for m in pair)
    quads = (quant.q_gate_up, quant.s_gate_up, quant.q_down, quant.s_down)
    x = torch.randn(9, H, generator=torch.Generator().manual_seed(1)).to(dtype)
    ids, weights = ops.moe_route(x, deq.router.weight.to(dtype), 2)
    ids[4, 1] = E  # adds nothing
    with torch.no_grad():
        want = ref.moe_ffn_ref(x, ids, weights, deq.w_gate_up.to(dtype), deq.w_down.to(dtype))  # exact in bf16 too
    assert torch.equal(ref.moe_ffn_w4_ref(x, ids, weights, *quads), want)
    assert torch.equal(ops.moe_ffn_w4(x, ids, weights, *quads), want) and not ops.moe_w4_supported(9, H, I, E, 2, x)
    if dtype == torch.float32:  # the grouped dequantising form: the same sums per row in another order
        assert torch.allclose(ref.moe_ffn_w4_grouped(x, ids, weights, *quads), want, rtol=1e-4, atol=1e-6)


def test_expert_dtype_deployment_streams_tokens():
    dep = LlamaDeployment.func_or_class("mixtral-tiny", dtype="float32", max_slots=4, num_blocks=64, expert_dtype="mxfp4")

    async def run():
        async def one(p):
            return [tok async for tok in dep.generate(p, max_new_tokens=5)]
        out = await asyncio.gather(*(one(p) for p in PROMPTS))
        while dep._driver is not None:
            await asyncio.sleep(0.002)
        return out, await dep.status()
    got, idle = asyncio.run(run())
    assert idle["expert_dtype"] == "mxfp4" and idle["weight_bytes"] == weight_bytes(dep.model) and "weight_dtype" not in idle
    assert idle["active"] == 0 and got == dep.model.generate(PROMPTS, 5)
    plain = LlamaDeployment.func_or_class("mixtral-tiny", dtype="float32", max_slots=2, num_blocks=16)
    assert not {"expert_dtype", "weight_bytes"} & set(asyncio.run(plain.status()))
