"""Mixture of experts without a GPU: the ``mixtral-tiny`` model in fp32 on the reference (ops/reference.py)."""
import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import LLAMA_PRESETS, MoEMLP, build_llama
from ray_community_amd.ops import reference as ref


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return build_llama("mixtral-tiny", dtype=torch.float32).eval()


def test_mixtral_tiny_counts_its_parameters_and_refuses_quantisation_and_lora(tiny):
    assert all(isinstance(b.mlp, MoEMLP) for b in tiny.layers)
    assert tiny.cfg.num_params() == sum(p.numel() for p in tiny.parameters())
    assert LLAMA_PRESETS["mixtral-8x7b"].num_params() == 46_702_792_704
    active = tiny.cfg.num_params() - 2 * (4 - 2) * 3 * 256 * 512  # two of the four experts of each of the two layers
    assert tiny.cfg.flops_per_token(128) == 6 * (active - 1024 * 256 - 5 * 256) + 6 * 2 * 256 * 128
    w = tiny.layers[0].mlp
    assert tuple(w.router.weight.shape) == (4, 256) and tuple(w.w_gate_up.shape) == (4, 1024, 256)
    assert tuple(w.w_down.shape) == (4, 256, 512) and w.w_down.std() < 0.6 * w.w_gate_up.std()  # out_std
    for dtype in ("fp8", "mxfp4"):  # quantised experts and LoRA on experts are refused
        with pytest.raises(NotImplementedError, match="MoE"):
            tiny.quantize_weights_(dtype)
    with pytest.raises(NotImplementedError, match="MoE"):
        tiny.enable_lora_(2, 4)


def test_mixtral_tiny_generates_the_same_tokens_chunked_and_grouped_rows_agree(tiny):
    w = tiny.layers[0].mlp
    with torch.no_grad():  # the grouped form of the reference (fp32 here: the same sums per row)
        x = torch.randn(9, 256)
        ids, weights = ops.moe_route(x, w.router.weight, 2)
        assert ids.dtype == torch.int32 and torch.allclose(weights.sum(1), torch.ones(9))
        assert torch.allclose(ref.moe_ffn_grouped(x, ids, weights, w.w_gate_up, w.w_down),
                              ops.moe_ffn(x, ids, weights, w.w_gate_up, w.w_down), rtol=1e-4, atol=1e-6)
    prompts = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]
    want = tiny.generate(prompts, 6)
    assert want == tiny.generate(prompts, 6, prefill_chunk=5) and [len(r) for r in want] == [6, 6, 6]


def test_the_dense_model_keeps_its_keys_and_logits():
    models = []
    for over in ({}, dict(num_experts=0, experts_per_token=7)):
        torch.manual_seed(0)
        models.append(build_llama("llama3-tiny", dtype=torch.float32, **over).eval())
    a, b = models
    assert {k.split(".", 2)[2] for k in a.state_dict() if k.startswith("layers.0.mlp.")} == {"mlp.gate_up.weight", "mlp.down.weight"}
    assert list(a.state_dict()) == list(b.state_dict()) and not any("router" in k or "w_" in k for k in a.state_dict())
    with torch.no_grad():
        assert torch.equal(a(torch.arange(40).view(2, 20)), b(torch.arange(40).view(2, 20)))
