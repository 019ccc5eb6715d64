"""LlamaDeployment with ``speculative``: the replica-side generator driven in-process streams the
same tokens as the plain deployment for greedy requests, and ``status()`` carries the
``"speculative"`` entry only when the knob is set.

Stream equality holds under the margin condition of test_speculative_cpu.py: every greedy step of
the plain streams has a top-2 logit gap >= 1e-3 (checked here), against about 1e-6 between the
logits of ``extend`` and ``decode_step`` in fp32. The lm_head is scaled as there, so that the gaps
of the random llama3-tiny are wide."""
import asyncio

import torch

from ray_community_amd.serve.llm import LlamaDeployment

SEED = 0
MARGIN = 1e-3
N_NEW = 16


def _prompt(n, seed, span=5):
    g = torch.Generator().manual_seed(seed)
    spans = torch.randint(0, 1024, (3, span), generator=g).tolist()
    order = torch.randint(0, 3, (n // span + 1,), generator=g).tolist()
    return [t for o in order for t in spans[o]][:n]


PROMPTS = [_prompt(12, 1), _prompt(70, 2), _prompt(41, 3)]


def _deployment(**kw):
    dep = LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", seed=SEED, max_slots=4, num_blocks=64, **kw)
    with torch.no_grad():
        dep.model.lm_head.weight.mul_(12.0)
    return dep


def _stream_all(dep, prompts, n):
    async def one(p):
        return [tok async for tok in dep.generate(p, max_new_tokens=n)]

    async def run():
        out = await asyncio.gather(*(one(p) for p in prompts))
        while dep._driver is not None:
            await asyncio.sleep(0.002)
        return out, await dep.status()

    return asyncio.run(run())


def test_speculative_deployment_streams_the_same_tokens():
    plain = _deployment(fused_sampling=True)
    want, idle = _stream_all(plain, PROMPTS, N_NEW)
    assert "speculative" not in idle
    for p, stream in zip(PROMPTS, want):  # the margin condition
        with torch.no_grad():
            logits = plain.model(torch.tensor([p + stream]))[0]
        for i, tok in enumerate(stream):
            top = logits[len(p) - 1 + i].topk(2)
            assert int(top.indices[0]) == tok and (top.values[0] - top.values[1]).item() >= MARGIN
    dep = _deployment(speculative=4)
    got, idle = _stream_all(dep, PROMPTS, N_NEW)
    assert got == want and all(len(t) == N_NEW for t in got)
    spec = idle["speculative"]
    assert set(spec) == {"num_draft", "verify_steps", "drafted", "accepted", "emitted"} and spec["num_draft"] == 4
    assert spec["verify_steps"] > 0 and spec["accepted"] <= spec["drafted"]
    assert idle["fused_sampling"] is True and idle["active"] == 0
    assert dep.engine.cache.num_free_blocks == 64


def test_status_omits_speculative_when_off():
    dep = _deployment()

    async def run():
        return await dep.status()

    assert asyncio.run(run()) == {"active": 0, "waiting": 0, "streams": [], "cancelled": 0}
