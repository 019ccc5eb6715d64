"""LlamaDeployment with ``weight_dtype="fp8"``: the replica quantises its linears after loading the
state dict, streams the tokens a ``GenerationEngine`` over an equally quantised model gives, and
``status()`` carries ``weight_dtype`` / ``weight_bytes`` only when the knob is set."""
import asyncio

import torch

from ray_community_amd.models import GenerationEngine, QuantLinear, build_llama, weight_bytes
from ray_community_amd.serve.llm import LlamaDeployment

PROMPTS = [[5, 9, 200, 31, 7, 7, 12], [100, 3, 3, 900], [44] * 19]
N_NEW = 10


def _stream_all(dep, prompts, n):
    async def one(p):
        return [tok async for tok in dep.generate(p, max_new_tokens=n)]

    async def run():
        out = await asyncio.gather(*(one(p) for p in prompts))
        while dep._driver is not None:
            await asyncio.sleep(0.002)
        return out, await dep.status()

    return asyncio.run(run())


def test_fp8_weight_deployment_streams_the_engines_tokens(tmp_path):
    torch.manual_seed(7)
    src = build_llama("llama3-tiny", dtype=torch.float32)
    path = tmp_path / "model.pt"
    torch.save(src.state_dict(), path)
    dep = LlamaDeployment.func_or_class("llama3-tiny", state_dict_path=str(path), dtype="float32", max_slots=4,
                                        num_blocks=64, weight_dtype="fp8")
    assert isinstance(dep.model.lm_head, QuantLinear) and isinstance(dep.model.layers[0].attn.qkv, QuantLinear)
    got, idle = _stream_all(dep, PROMPTS, N_NEW)
    assert idle["weight_dtype"] == "fp8" and idle["weight_bytes"] == weight_bytes(dep.model) < weight_bytes(src)
    assert idle["active"] == 0 and all(len(t) == N_NEW for t in got)

    eng = GenerationEngine(src.eval().quantize_weights_("fp8"), max_slots=4, num_blocks=64)
    rids = [eng.add_request(p, N_NEW) for p in PROMPTS]
    want = {r: [] for r in rids}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            want[rid].append(tok)
    assert got == [want[r] for r in rids]


def test_status_omits_weight_dtype_when_off():
    for knob in (None, "auto"):
        dep = LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", max_slots=2, num_blocks=16, weight_dtype=knob)
        assert not isinstance(dep.model.lm_head, QuantLinear)
        st = asyncio.run(dep.status())
        assert "weight_dtype" not in st and "weight_bytes" not in st
