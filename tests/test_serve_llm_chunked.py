"""LlamaDeployment with chunked prefill (``prefill_chunk``): the replica-side generator driven
in-process streams the same tokens as a deployment without it, and ``status()`` shows the setting
and the requests still in their prompt."""
import asyncio

import torch

from ray_community_amd.serve.llm import LlamaDeployment

SEED = 0


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (n,), generator=g).tolist()


def _deployment(**kw):
    return LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", seed=SEED, max_slots=4, num_blocks=64, **kw)


def _stream_all(dep, prompts, n):
    async def one(p):
        return [tok async for tok in dep.generate(p, max_new_tokens=n)]

    async def run():
        out = await asyncio.gather(*(one(p) for p in prompts))
        while dep._driver is not None:
            await asyncio.sleep(0.002)
        return out, await dep.status()

    return asyncio.run(run())


def test_chunked_deployment_streams_the_same_tokens():
    prompts = [_prompt(5, 1), _prompt(70, 2), _prompt(40, 3)]
    want, idle = _stream_all(_deployment(), prompts, 8)
    assert idle == {"active": 0, "waiting": 0, "streams": [], "cancelled": 0}
    dep = _deployment(prefill_chunk=16)
    got, idle = _stream_all(dep, prompts, 8)
    assert got == want and all(len(t) == 8 for t in got)
    assert idle == {"active": 0, "waiting": 0, "streams": [], "cancelled": 0, "prefill_chunk": 16, "prefilling": 0}
    assert dep.engine.cache.num_free_blocks == 64


def test_status_counts_prefilling_requests():
    dep = _deployment(prefill_chunk=16)

    async def run():
        agen = dep.generate(_prompt(150, 2), max_new_tokens=4)
        task = asyncio.ensure_future(agen.__anext__())
        seen = []
        while not task.done():
            seen.append((await dep.status())["prefilling"])
            await asyncio.sleep(0.0005)
        rest = [tok async for tok in agen]
        return seen, [task.result()] + rest, await dep.status()

    seen, toks, after = asyncio.run(run())
    assert 1 in seen and len(toks) == 4
    assert after["prefill_chunk"] == 16 and after["prefilling"] == 0
