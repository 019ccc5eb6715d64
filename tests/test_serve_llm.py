"""LlamaDeployment (serve/llm.py): concurrent token streams over one continuous-batching engine,
through deployment handles and over HTTP. CPU, llama3-tiny in fp32."""
import json
import threading
import urllib.request

import pytest
import torch

import ray_community_amd as ray
from ray_community_amd import serve
from ray_community_amd.models import build_llama
from ray_community_amd.serve.llm import LlamaDeployment

PORT = 18147
MARGIN = 1e-3
SEED = 0


@pytest.fixture(scope="module")
def llm_handle():
    ray.init(num_cpus=4, log_to_driver=False)
    serve.start(http_options={"port": PORT})
    app = LlamaDeployment.bind("llama3-tiny", dtype="float32", seed=SEED, max_slots=4, num_blocks=64)
    yield serve.run(app, name="llm", route_prefix="/llm")
    serve.shutdown()
    ray.shutdown()


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(SEED)  # the replica seeds its weights the same way
    return build_llama("llama3-tiny", dtype=torch.float32).eval()


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (n,), generator=g).tolist()


def _safe_steps(model, prompt, toks):
    """Steps comparable under the margin rule: up to the first step at which the no-cache
    forward's top-2 logit margin is below MARGIN."""
    seq = list(prompt)
    with torch.no_grad():
        for step, t in enumerate(toks):
            top = model(torch.tensor([seq]))[0, -1].topk(2).values
            if (top[0] - top[1]).item() < MARGIN:
                return step
            seq.append(t)
    return len(toks)


def test_concurrent_streams_and_http(llm_handle, model):
    # long enough that a generation is far from done when its first token has reached the caller
    cases = [(_prompt(4, 1), 60), (_prompt(19, 2), 90), (_prompt(33, 3), 120)]
    gens = [llm_handle.options(method_name="generate", stream=True).remote(p, max_new_tokens=n) for p, n in cases]
    got = [[] for _ in cases]
    seen = [None] * len(cases)

    def pull(i):
        for tok in gens[i]:
            got[i].append(tok)
            if len(got[i]) == 1:  # first token in hand: what does the replica say about this stream?
                seen[i] = llm_handle.status.remote().result()

    threads = [threading.Thread(target=pull, args=(i,)) for i in range(len(cases))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads)
    want = model.generate([p for p, _ in cases], max(n for _, n in cases))
    compared = total = 0
    for (p, n), toks, ref, st in zip(cases, got, want, seen):
        assert len(toks) == n and all(isinstance(t, int) for t in toks)
        # incremental: when the caller held its first token the replica was still generating this
        # request (a deployment or transport that buffered the whole stream would have finished it)
        mine = [e for e in st["streams"] if e["max_new_tokens"] == n]
        assert len(mine) == 1 and 1 <= mine[0]["produced"] < n, st
        assert st["active"] >= 1
        safe = _safe_steps(model, p, ref[:n])
        assert toks[:safe] == ref[:safe]
        compared += safe
        total += n
    assert compared * 4 >= total * 3
    idle = llm_handle.status.remote().result()
    assert idle == {"active": 0, "waiting": 0, "streams": [], "cancelled": 0}

    p, n = cases[0][0], 9
    solo = list(llm_handle.options(method_name="generate", stream=True).remote(p, max_new_tokens=n))
    req = urllib.request.Request(f"http://127.0.0.1:{PORT}/llm", method="POST",
                                 data=json.dumps({"prompt_tokens": p, "max_new_tokens": n}).encode(),
                                 headers={"content-type": "application/json"})
    with urllib.request.urlopen(req, timeout=60) as r:
        text = r.read().decode()
    assert text.endswith("\n")
    assert [int(x) for x in text.split()] == solo  # both ran alone: the same batch, the same tokens
    assert len(solo) == n


def test_closed_stream_gives_its_slot_back():
    """The replica-side generator, driven in-process: closing it mid-stream cancels the request in
    the engine (slot and cache blocks free at once) instead of decoding 200 tokens into the void."""
    import asyncio

    dep = LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", seed=SEED, max_slots=2, num_blocks=32)

    async def run():
        agen = dep.generate(_prompt(5, 7), max_new_tokens=200)
        first = await agen.__anext__()
        busy = await dep.status()
        await agen.aclose()  # the consumer goes away
        while dep._driver is not None:  # the driver stops once the engine is empty
            await asyncio.sleep(0.005)
        return first, busy, await dep.status(), dep.engine.cache.num_free_blocks

    first, busy, after, free = asyncio.run(run())
    assert isinstance(first, int)
    assert busy["active"] == 1 and busy["streams"][0]["produced"] < 200 and busy["cancelled"] == 0
    assert after == {"active": 0, "waiting": 0, "streams": [], "cancelled": 1}
    assert free == 32
    assert not dep.engine.has_work()
