"""LlamaDeployment with ``lora=``: a request selects its adapter through the HTTP body key ``"adapter"``,
the handle keyword or ``multiplexed_model_id``; the streams equal direct ``generate(adapters=...)``;
``status()`` carries ``"lora"`` only when enabled; adapters load and unload at run time; an unknown adapter
fails its own request only. CPU, llama3-tiny in fp32."""
import asyncio
import json
import urllib.request

import pytest
import torch

import ray_community_amd as ray
from ray_community_amd import serve
from ray_community_amd.models import LoraAdapter, build_llama
from ray_community_amd.models.lora import bank_bytes
from ray_community_amd.serve.llm import LlamaDeployment

PORT = 18153
SEED = 0
PROMPT = [5, 9, 200, 31, 7, 7, 12]
N_NEW = 8
LORA = {"max_adapters": 2, "max_rank": 4}


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    cfg = build_llama("llama3-tiny", dtype=torch.float32).cfg
    root = tmp_path_factory.mktemp("adapters")
    ads = {"a": LoraAdapter.random(cfg, 4, seed=1), "b": LoraAdapter.random(cfg, 2, seed=2, alpha=8)}
    paths = {}
    for name, ad in ads.items():
        paths[name] = str(root / f"{name}.pt")
        ad.save(paths[name])
    return ads, paths


@pytest.fixture(scope="module")
def want(adapters):
    """The streams of direct ``generate(adapters=...)`` calls on the model the replica builds."""
    torch.manual_seed(SEED)
    model = build_llama("llama3-tiny", dtype=torch.float32).eval().enable_lora_(**LORA)
    for name, ad in adapters[0].items():
        model.load_adapter(name, ad)
    out = {name: model.generate([PROMPT], N_NEW, adapters=[name])[0] for name in ("a", "b")}
    out[None] = model.generate([PROMPT], N_NEW)[0]
    assert out["a"] != out[None] and out["b"] != out[None] and out["a"] != out["b"]
    return out


@pytest.fixture(scope="module")
def llm_handle(adapters):
    ray.init(num_cpus=4, log_to_driver=False)
    serve.start(http_options={"port": PORT})
    app = LlamaDeployment.bind("llama3-tiny", dtype="float32", seed=SEED, max_slots=4, num_blocks=64, lora=LORA,
                               adapters={"a": adapters[1]["a"]})
    yield serve.run(app, name="llm-lora", route_prefix="/lora")
    serve.shutdown()
    ray.shutdown()


def _http(body):
    req = urllib.request.Request(f"http://127.0.0.1:{PORT}/lora", method="POST", data=json.dumps(body).encode(),
                                 headers={"content-type": "application/json"})
    with urllib.request.urlopen(req, timeout=60) as r:
        return [int(x) for x in r.read().decode().split()]


def test_body_key_handle_keyword_and_multiplexed_id_select_the_adapter(llm_handle, adapters, want):
    gen = llm_handle.options(method_name="generate", stream=True)
    assert list(gen.remote(PROMPT, max_new_tokens=N_NEW)) == want[None]
    assert list(gen.remote(PROMPT, max_new_tokens=N_NEW, adapter="a")) == want["a"]
    assert list(gen.options(multiplexed_model_id="a").remote(PROMPT, max_new_tokens=N_NEW)) == want["a"]
    assert _http({"prompt_tokens": PROMPT, "max_new_tokens": N_NEW, "adapter": "a"}) == want["a"]
    assert _http({"prompt_tokens": PROMPT, "max_new_tokens": N_NEW}) == want[None]

    st = llm_handle.status.remote().result()
    assert st["lora"]["loaded"] == ["a"] and st["lora"]["max_adapters"] == 2 and st["lora"]["max_rank"] == 4
    assert st["lora"]["bank_bytes"] > 0

    # b is not loaded yet: its request fails, the others do not
    with pytest.raises(Exception):
        list(gen.remote(PROMPT, max_new_tokens=N_NEW, adapter="b"))
    assert list(gen.remote(PROMPT, max_new_tokens=N_NEW, adapter="a")) == want["a"]
    assert llm_handle.load_adapter.remote("b", adapters[1]["b"]).result() == ["a", "b"]
    assert list(gen.remote(PROMPT, max_new_tokens=N_NEW, adapter="b")) == want["b"]
    assert list(gen.options(multiplexed_model_id="b").remote(PROMPT, max_new_tokens=N_NEW, adapter="a")) == want["a"]
    assert llm_handle.unload_adapter.remote("a").result() == ["b"]
    with pytest.raises(Exception):
        list(gen.remote(PROMPT, max_new_tokens=N_NEW, adapter="a"))
    assert list(gen.remote(PROMPT, max_new_tokens=N_NEW)) == want[None]
    idle = llm_handle.status.remote().result()
    assert idle["active"] == 0 and idle["waiting"] == 0 and idle["lora"]["loaded"] == ["b"]


def test_concurrent_mixed_requests_in_process(adapters, want):
    dep = LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", seed=SEED, max_slots=4, num_blocks=64, lora=LORA,
                                        adapters=adapters[1])

    async def one(name):
        try:
            return [tok async for tok in dep.generate(PROMPT, max_new_tokens=N_NEW, adapter=name)]
        except ValueError as e:
            return e

    async def run():
        out = await asyncio.gather(*(one(n) for n in ("a", None, "zzz", "b")))
        while dep._driver is not None:
            await asyncio.sleep(0.002)
        return out, await dep.status()

    (a, none, bad, b), st = asyncio.run(run())
    assert isinstance(bad, ValueError) and "unknown adapter" in str(bad)  # fails alone
    # each stream ran in a mixed batch: equal to its solo stream up to a near-tie in fp32, none seen here
    assert a == want["a"] and none == want[None] and b == want["b"]
    assert st["active"] == 0 and st["lora"] == {**LORA, "loaded": ["a", "b"], "bank_bytes": bank_bytes(dep.model)}


def test_status_omits_lora_when_off_and_adapters_need_the_knob(adapters):
    dep = LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", max_slots=2, num_blocks=16)
    assert "lora" not in asyncio.run(dep.status())
    with pytest.raises(ValueError, match="lora="):
        LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", max_slots=2, num_blocks=16, adapters=adapters[1])
    quant = LlamaDeployment.func_or_class("llama3-tiny", dtype="float32", max_slots=2, num_blocks=16, weight_dtype="fp8",
                                          lora=LORA)
    from ray_community_amd.models import LoraLinear, QuantLinear

    assert isinstance(quant.model.layers[0].attn.qkv, LoraLinear) and isinstance(quant.model.layers[0].attn.qkv.base, QuantLinear)
