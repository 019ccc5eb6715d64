"""``ops.lora_routing`` and ``ops.lora_add_(kernel=...)`` without a GPU: a tensor of slots is for the device
path only, and a forced arm never falls back to the reference."""
import pytest
import torch

from ray_community_amd import ops
from test_lora_cpu import case


def test_cpu_tensors_and_forced_arms_are_refused():
    c = case("coded", 5, 48, 384, 32, "cycle")
    with pytest.raises(ValueError, match="CUDA int32"):
        ops.lora_routing(torch.tensor(c["idx"], dtype=torch.int32), slots=4)
    routing = ops.lora_routing(c["idx"])  # the list path is what it was
    y = c["y0"].clone()
    for kernel in ("fused", "two_pass", "triton"):
        with pytest.raises(ValueError, match="kernel"):
            ops.lora_add_(y, c["x"], c["A"], c["B"], c["scale"], routing, kernel=kernel)
    assert torch.equal(y.view(torch.int16), c["y0"].view(torch.int16))
    assert ops.lora_add_(y, c["x"], c["A"], c["B"], c["scale"], routing, kernel="auto") is y
    assert ops.M_LORA_FUSED >= 0
