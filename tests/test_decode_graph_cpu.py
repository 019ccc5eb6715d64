"""Graphed decode on the CPU: the op's definition, and ``DecodeRunner`` without capture.

``ops.rope_kv_append_decode_`` on CPU tensors is ``rope_ref`` + ``kv_cache_append_ref`` on positions
and slots derived from ``context_lens`` and ``block_table``. ``DecodeRunner(capture=False)`` runs the
body the captured graph records, on the static buffers: the CPU reference attention has no splits, so
its logits equal ``Llama.decode_step``'s bit for bit whatever the block table's width, and every
stream with ``graph_decode=True`` equals the stream without.
"""
import copy
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import (DecodeRunner, GenerationEngine, KVCacheFull, LoraAdapter, PagedKVCache,
                                      build_llama)
from ray_community_amd.ops import reference as ref

V = 1024


def _rand(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (n,), generator=g).tolist()


@functools.lru_cache(maxsize=None)
def _model(max_seq_len=256):
    torch.manual_seed(0)
    return build_llama("llama3-tiny", dtype=torch.float32, max_seq_len=max_seq_len).eval()


# --------------------------------------------------------------------------------- op definition
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16cache", "fp8cache"])
def test_op_is_rope_then_append_on_derived_positions_and_slots(fp8):
    Hq, Hk, D, page, num_blocks, W = 4, 2, 64, 16, 6, 3
    g = torch.Generator().manual_seed(3)
    # row 0 inactive; row 1 at the first slot of a fresh page (n - 1 = 16); row 2 at n = 1; row 3 mid-page
    lens = [0, page + 1, 1, 2 * page + 7]
    table = torch.tensor([[5, 5, 5], [3, 1, 0], [4, 0, 0], [0, 2, 5]], dtype=torch.int32)
    B = len(lens)
    qkv = torch.randn(B, (Hq + 2 * Hk) * D, generator=g)
    cs = ops.rope_cos_sin(64, D)
    cdt = torch.float8_e4m3fn if fp8 else torch.float32

    def caches():
        kv = [torch.full((num_blocks, page, Hk, D), float("nan")).to(cdt) for _ in range(2)]
        sc = [torch.full((num_blocks, page, Hk), float("nan")) for _ in range(2)] if fp8 else [None, None]
        return kv, sc

    (k1, v1), (ks1, vs1) = caches()
    (k2, v2), (ks2, vs2) = caches()
    positions = torch.tensor([0, page, 0, 2 * page + 6])
    slots = torch.tensor([-1, 1 * page + 0, 4 * page + 0, 5 * page + 6], dtype=torch.int32)
    want = qkv.clone()
    n_rot = (Hq + Hk) * D
    rot = ref.rope_ref(qkv[:, :n_rot].reshape(B, Hq + Hk, D), cs, positions).reshape(B, n_rot)
    want[1:, :n_rot] = rot[1:]
    ref.kv_cache_append_ref(k1, v1, want, slots, Hq, Hk, D, ks1, vs1)

    got = ops.rope_kv_append_decode_(qkv.clone(), cs, k2, v2, table, torch.tensor(lens, dtype=torch.int32), Hq, Hk, D,
                                     k_scale=ks2, v_scale=vs2)
    assert torch.equal(got, want)
    assert torch.equal(got[0], qkv[0])  # the inactive row is untouched
    written = sorted(int(s) for s in slots if s >= 0)
    for a, b in ((k1, k2), (v1, v2)) + (((ks1, ks2), (vs1, vs2)) if fp8 else ()):
        a, b = (a.float(), b.float())
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
        flat = b.reshape(num_blocks * page, -1)
        alive = (~torch.isnan(flat).any(dim=1)).nonzero().flatten().tolist()
        assert alive == written  # NaN everywhere except the written slots, which hold no NaN


def test_op_rows_past_the_table_or_the_cache_are_inactive():
    Hq, Hk, D, page, num_blocks = 2, 2, 64, 16, 2
    qkv = torch.randn(3, (Hq + 2 * Hk) * D)
    k = torch.full((num_blocks, page, Hk, D), float("nan"))
    v = k.clone()
    table = torch.tensor([[0], [7], [1]], dtype=torch.int32)  # row 1 names no block of the cache
    lens = torch.tensor([page + 1, 3, 200], dtype=torch.int32)  # rows 0 and 2 lie past the one-column table
    got = ops.rope_kv_append_decode_(qkv.clone(), ops.rope_cos_sin(64, D), k, v, table, lens, Hq, Hk, D)
    assert torch.equal(got, qkv) and torch.isnan(k).all() and torch.isnan(v).all()


# ------------------------------------------------------------------------ runner == decode_step
def _prefilled(model, prompts, ids, num_blocks=64, **kw):
    cache = PagedKVCache(model.cfg, num_blocks, 16, dtype=torch.float32, **kw)
    logits = model.prefill([list(p) for p in prompts], None, cache, ids)
    return cache, logits


def test_runner_equals_decode_step_across_page_and_bucket_boundaries():
    model = _model(1024)
    prompts = [_rand(250, 1), _rand(14, 2), _rand(37, 3)]  # 250: into block 17 (bucket 16 -> 32) at step 7
    ids = ["a", "b", "c"]
    c1, lg = _prefilled(model, prompts, ids)
    c2, _ = _prefilled(model, prompts, ids)
    runner = DecodeRunner(model, c2, 4, capture=False)
    seq = ["a", None, "b", "c"]
    toks = [int(t) for t in lg.argmax(-1)]
    toks = [toks[0], 0, toks[1], toks[2]]
    widths = set()
    for step in range(44):
        want = model.decode_step(toks, c1, seq)
        got = runner.step(toks, seq)
        assert torch.equal(want, got), f"step {step}"
        widths.add(runner.width_for(max(c2.blocks_held(s) for s in ids)))
        toks = [int(t) for t in want.argmax(-1)]
        toks[1] = 0
    assert widths == {16, 32}
    assert c2.length("b") == 14 + 44 and c2.blocks_held("b") == 4  # crossed page boundaries
    assert all(c1.length(s) == c2.length(s) for s in ids)
    for i in range(model.cfg.num_layers):  # the caches agree wherever a sequence lives
        for s in ids:
            for blk1, blk2 in zip(c1._blocks[s], c2._blocks[s]):
                assert blk1 == blk2
        n = c1._lens["a"]
        b = c1._blocks["a"]
        assert torch.equal(c1.k[i][b].reshape(-1, 2, 64)[:n], c2.k[i][b].reshape(-1, 2, 64)[:n])
        assert torch.equal(c1.v[i][b].reshape(-1, 2, 64)[:n], c2.v[i][b].reshape(-1, 2, 64)[:n])
    assert runner.stats == {"graphs": 0, "replays": 0, "eager_warm": 0, "eager_fallback": 0}


def test_runner_fp8_cache_equals_decode_step():
    model = _model()
    prompts, ids = [_rand(9, 4), _rand(20, 5)], ["a", "b"]
    c1, lg = _prefilled(model, prompts, ids, kv_dtype="fp8")
    c2, _ = _prefilled(model, prompts, ids, kv_dtype="fp8")
    runner = DecodeRunner(model, c2, 2, capture=False)
    toks = [int(t) for t in lg.argmax(-1)]
    for step in range(10):
        want = model.decode_step(toks, c1, ids)
        assert torch.equal(want, runner.step(toks, ids)), f"step {step}"
        toks = [int(t) for t in want.argmax(-1)]


def test_cache_full_leaves_the_cache_as_it_was():
    model = _model()
    cache = PagedKVCache(model.cfg, 3, 16, dtype=torch.float32)
    model.prefill([_rand(16, 6), _rand(16, 7), _rand(5, 8)], None, cache, ["a", "b", "c"])
    runner = DecodeRunner(model, cache, 3, capture=False)
    before = (dict(cache._lens), {s: list(b) for s, b in cache._blocks.items()}, cache.num_free_blocks, list(cache._free))
    with pytest.raises(KVCacheFull):
        runner.step([1, 2, 3], ["c", "a", "b"])  # "c" fits its page; "a" and "b" each need a block, none is free
    after = (dict(cache._lens), {s: list(b) for s, b in cache._blocks.items()}, cache.num_free_blocks, list(cache._free))
    assert before == after
    with pytest.raises(ValueError):
        runner.step([1, 2], ["a", "b"])  # not the runner's batch size


def test_max_seq_len_is_checked_before_anything_is_allocated():
    model = _model()
    cache = PagedKVCache(model.cfg, 20, 16, dtype=torch.float32)
    cache.allocate("a", 256)
    runner = DecodeRunner(model, cache, 1, capture=False)
    with pytest.raises(ValueError, match="max_seq_len"):
        runner.step([1], ["a"])
    assert cache.length("a") == 256


# -------------------------------------------------------------------- streams, knob on and off
PROMPTS = (tuple(_rand(7, 11)), tuple(_rand(40, 12)), tuple(_rand(23, 13)))
MODES = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.9, top_p=0.9, seed=8, fused_sampling=True),
         "penalties_logprobs": dict(temperature=0.8, seed=3, repetition_penalty=1.3, presence_penalty=0.2,
                                    frequency_penalty=0.1, logprobs=2)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_generate_streams_do_not_depend_on_the_knob(mode):
    model = _model()
    off = model.generate([list(p) for p in PROMPTS], 20, **MODES[mode])
    on = model.generate([list(p) for p in PROMPTS], 20, graph_decode=True, **MODES[mode])
    assert on == off


def _serve(engine, requests):
    for prompt, n, kw in requests:
        engine.add_request(list(prompt), n, **kw)
    events = []
    while engine.has_work():
        events.extend(engine.step())
    return events


def test_engine_streams_do_not_depend_on_the_knob():
    model = _model()
    requests = [(PROMPTS[0], 12, {}), (PROMPTS[1], 5, dict(temperature=0.9, top_p=0.8, seed=4)),
                (PROMPTS[2], 9, dict(temperature=0.7, seed=2, repetition_penalty=1.2, frequency_penalty=0.3, logprobs=2)),
                (PROMPTS[0][:3], 14, {}), (PROMPTS[1][:9], 3, dict(temperature=1.0, min_p=0.05, seed=9))]
    off = GenerationEngine(model, max_slots=2, num_blocks=32, fused_sampling=True)
    on = GenerationEngine(model, max_slots=2, num_blocks=32, fused_sampling=True, graph_decode=True)
    assert off.runner is None and on.runner is not None and not on.runner.capture
    want = _serve(off, requests)
    assert _serve(on, requests) == want
    assert len(want) == sum(n for _, n, _ in requests)
    assert on.pop_logprobs(2) == off.pop_logprobs(2) != []


# ------------------------------------------------------------------------------------ fallbacks
def test_lora_rounds_run_decode_step_and_are_counted():
    model = copy.deepcopy(_model()).enable_lora_(max_adapters=1, max_rank=4)
    model.load_adapter("a", LoraAdapter.random(model.cfg, 4, seed=1))
    prompts, adapters = [list(PROMPTS[0]), list(PROMPTS[2])], ["a", None]
    off = model.generate(prompts, 8, adapters=adapters)
    cache = PagedKVCache(model.cfg, 16, 16, dtype=torch.float32)
    on = model.generate(prompts, 8, adapters=adapters, graph_decode=True, cache=cache)
    assert on == off
    (runner,) = cache._decode_runners.values()
    assert runner.stats["eager_fallback"] == 7  # every decode round: the first token comes from the prefill
    # the same model with no adapter named runs the body
    assert model.generate(prompts, 8, graph_decode=True, cache=cache) == model.generate(prompts, 8)
    assert runner.stats["eager_fallback"] == 7


def test_verify_rounds_are_counted_and_streams_equal():
    model = _model()
    prompt = list(PROMPTS[0]) * 4  # repeats: the prompt-lookup proposer has drafts
    off = model.generate([prompt], 16, speculative=3)
    verify = model.spec_stats["verify_steps"]
    cache = PagedKVCache(model.cfg, 16, 16, dtype=torch.float32)
    on = model.generate([prompt], 16, speculative=3, graph_decode=True, cache=cache)
    assert on == off and model.spec_stats["verify_steps"] == verify > 0
    (runner,) = cache._decode_runners.values()
    assert runner.stats["eager_fallback"] == verify


# ------------------------------------------------------------------------------------ staleness
def test_a_stepped_runner_follows_quantize_weights():
    model = copy.deepcopy(_model())
    prompts, ids = [_rand(12, 21), _rand(5, 22)], ["a", "b"]
    c1, lg = _prefilled(model, prompts, ids)
    c2, _ = _prefilled(model, prompts, ids)
    runner = DecodeRunner(model, c2, 2, capture=False)
    toks = [int(t) for t in lg.argmax(-1)]
    old = model.decode_step(toks, c1, ids).clone()
    assert torch.equal(runner.step(toks, ids), old)
    epoch = model.module_epoch
    model.quantize_weights_("fp8")
    assert model.module_epoch > epoch
    want = model.decode_step(toks, c1, ids)
    got = runner.step(toks, ids)
    assert torch.equal(got, want) and not torch.equal(got, old)
    assert runner._epoch == model.module_epoch
