"""Graphed decode on the GPU: the fused RoPE + cache-append kernel against the two kernels it
replaces, and ``DecodeRunner``'s replay against the uncaptured body and against ``decode_step``.

Every comparison is bitwise. The fused kernel evaluates ``rope_kernel``'s rotation (one shared
helper) and the append kernels' copy / quantisation on the same values; a replayed graph launches
the kernels the uncaptured body launches, on the same shapes. llama3-tiny at ``max_seq_len = 256``
and page 16 has a decode split count of 1 at every block-table width, so there the runner's bucketed
table and ``decode_step``'s tight one run identical kernels too.

No test here passes a context length beyond the block table or the cache: the kernel's out-of-range
guard is read from the code (``ops/csrc/decode_step.hip``), not exercised on the device.
"""
import asyncio
import copy
import functools

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import DecodeRunner, GenerationEngine, PagedKVCache, build_llama
from ray_community_amd.ops._lib import lib
from test_linear_w8_cpu import PADS

pytestmark = pytest.mark.gpu
V = 1024
SLACK = 2


def _rand(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (n,), generator=g).tolist()


def _raw(t):
    """The tensor as integers of its element size (NaN-safe equality; fp8 tensors index this way)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _bits(t):
    """The tensor's bytes on the CPU."""
    return _raw(t).contiguous().view(torch.uint8).cpu()


# ------------------------------------------------------------------------- fused kernel, bit for bit
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16cache", "fp8cache"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("page", [16, 32])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_fused_kernel_equals_rope_then_append(D, G, page, B, fp8):
    Hk, W = 2, 3
    Hq = G * Hk
    cols = (Hq + 2 * Hk) * D
    assert ops.paged_decode_supported(page, D, Hq, Hk)
    g = torch.Generator().manual_seed(D + G + page + B)
    # inactive, the first token, a full first page, the first slot of a fresh page, the last slot of
    # the last table column
    lens = [0, 1, page, page + 1, W * page][:B] if B > 1 else [page + 1]
    num_blocks = B * W + 2
    table = torch.randperm(num_blocks, generator=g)[: B * W].to(torch.int32).view(B, W)
    pad, c0 = PADS[(G + B) % 3]
    buf = torch.full((B + 2 * SLACK, cols + pad), float("nan"), dtype=torch.bfloat16)
    buf[SLACK:SLACK + B, c0:c0 + cols] = torch.randn(B, cols, generator=g).to(torch.bfloat16)
    cs = ops.rope_cos_sin(W * page, D).cuda()

    def operands():
        whole = buf.cuda()
        view = whole[SLACK:SLACK + B, c0:c0 + cols]
        assert view.stride(0) == cols + pad and view.data_ptr() % 16 == 0
        shape = (num_blocks, page, Hk, D)
        if fp8:
            kv = [torch.full(shape, 0x5A, dtype=torch.uint8).cuda().view(torch.float8_e4m3fn) for _ in range(2)]
            sc = [torch.full(shape[:3], -12345.0).cuda() for _ in range(2)]
        else:
            kv = [torch.full(shape, 0x5A5A, dtype=torch.int16).cuda().view(torch.bfloat16) for _ in range(2)]
            sc = [None, None]
        return whole, view, kv, sc

    # the composition, on host-computed positions and slots
    whole1, view1, (k1, v1), (ks1, vs1) = operands()
    positions = torch.tensor([max(n - 1, 0) for n in lens], dtype=torch.int32).cuda()
    slots = [int(table[b, (n - 1) // page]) * page + (n - 1) % page if n > 0 else -1 for b, n in enumerate(lens)]
    ops.apply_rope_(view1, cs, 1, Hq, Hk, D, positions)
    ops.kv_cache_append_(k1, v1, view1, torch.tensor(slots, dtype=torch.int32).cuda(), Hq, Hk, D, k_scale=ks1,
                         v_scale=vs1)
    # the fused kernel
    whole2, view2, (k2, v2), (ks2, vs2) = operands()
    out = ops.rope_kv_append_decode_(view2, cs, k2, v2, table.cuda(), torch.tensor(lens, dtype=torch.int32).cuda(),
                                     Hq, Hk, D, k_scale=ks2, v_scale=vs2)
    torch.cuda.synchronize()
    assert out.data_ptr() == view2.data_ptr()
    assert torch.equal(_bits(whole1), _bits(whole2))  # the rows, and the NaN guard band around them
    outside = torch.ones(B + 2 * SLACK, cols + pad, dtype=torch.bool)
    outside[SLACK:SLACK + B, c0:c0 + cols] = False
    assert torch.equal(_bits(whole2).view(torch.int16)[outside], _bits(buf).view(torch.int16)[outside])
    if 0 in lens:
        assert torch.equal(_bits(view2[0]), _bits(buf[SLACK, c0:c0 + cols]))  # the inactive row
    live = torch.zeros(num_blocks * page, dtype=torch.bool)
    live[[s for s in slots if s >= 0]] = True
    _, _, (fresh_kv, _), (fresh_sc, _) = operands()
    for a, b in ((k1, k2), (v1, v2)) + (((ks1, ks2), (vs1, vs2)) if fp8 else ()):
        assert torch.equal(_bits(a), _bits(b))
        rows = _bits(b).view(num_blocks * page, -1)
        fresh = _bits(fresh_kv if b.dim() == 4 else fresh_sc).view(num_blocks * page, -1)
        assert torch.equal(rows[~live], fresh[~live])  # every byte outside the written slots
        assert not (rows[live] == fresh[live]).all(dim=1).any()  # and the written slots were written


# -------------------------------------------------------------------------------------- the runner
@functools.lru_cache(maxsize=None)
def _model(max_seq_len=256, weights=None):
    torch.manual_seed(0)
    return build_llama("llama3-tiny", device="cuda", max_seq_len=max_seq_len, weight_dtype=weights).eval()


def _prefilled(model, prompts, ids, num_blocks, **kw):
    cache = PagedKVCache(model.cfg, num_blocks, 16, device="cuda", **kw)
    logits = model.prefill([list(p) for p in prompts], None, cache, ids)
    return cache, [int(t) for t in logits.argmax(-1)]


def test_replay_equals_the_uncaptured_body_with_split_attention():
    model = _model(2048)
    c1, toks = _prefilled(model, [_rand(600, 1)], ["a"], 64)
    c2 = copy.deepcopy(c1)
    graphed, plain = DecodeRunner(model, c1, 1), DecodeRunner(model, c2, 1, capture=False)
    assert graphed.capture and not plain.capture
    width = graphed.width_for(c1.blocks_held("a"))
    assert width == 64 and lib().rca_attn_decode_num_splits(1, model.cfg.num_kv_heads, width * 16, 16) > 1
    for step in range(20):
        got = graphed.step(toks, ["a"]).clone()
        want = plain.step(toks, ["a"])
        assert torch.equal(_bits(got), _bits(want)), f"step {step}"
        toks = [int(want.argmax(-1))]
    assert graphed.stats["eager_warm"] == 1 and graphed.stats["graphs"] == 1 and graphed.stats["replays"] >= 18
    assert plain.stats["replays"] == 0


@pytest.mark.parametrize("variant", ["bf16", "fp8_kv", "fp8_weights"])
def test_replay_equals_eager_decode_step(variant):
    model = _model(256, "fp8" if variant == "fp8_weights" else None)
    kw = {"kv_dtype": "fp8"} if variant == "fp8_kv" else {}
    prompts, ids = [_rand(5, 2), _rand(17, 3), _rand(40, 4)], ["a", "b", "c"]
    c1, first = _prefilled(model, prompts, ids, 32, **kw)
    c2 = copy.deepcopy(c1)
    runner = DecodeRunner(model, c2, 4)
    seq = ["a", "b", None, "c"]
    toks = [first[0], first[1], 0, first[2]]
    for step in range(30):
        want = model.decode_step(toks, c1, seq)
        got = runner.step(toks, seq)
        assert torch.equal(_bits(want), _bits(got)), f"step {step}"
        toks = [int(t) for t in want.argmax(-1)]
        toks[2] = 0
    assert runner.stats == {"graphs": 1, "replays": 29, "eager_warm": 1, "eager_fallback": 0}
    for i in range(model.cfg.num_layers):  # both caches hold the same bytes where the sequences live
        for s in ids:
            blocks, n = c1._blocks[s], c1.length(s)
            assert blocks == c2._blocks[s] and n == c2.length(s)
            for t1, t2 in zip((c1.k[i], c1.v[i]) + (c1.scales(i) if c1.fp8 else ()),
                              (c2.k[i], c2.v[i]) + (c2.scales(i) if c2.fp8 else ())):
                r1, r2 = (_bits(_raw(t)[blocks]).view(len(blocks) * 16, -1)[:n] for t in (t1, t2))
                assert torch.equal(r1, r2)


def test_the_graph_reads_only_the_runners_buffers():
    model = _model()
    c1, first = _prefilled(model, [_rand(9, 5), _rand(30, 6)], ["a", "b"], 16)
    c2 = copy.deepcopy(c1)
    runner = DecodeRunner(model, c1, 2)
    eager_toks = list(first)
    toks = torch.tensor(first, dtype=torch.long, device="cuda")
    for _ in range(3):  # warm, capture, replay
        want = model.decode_step(eager_toks, c2, ["a", "b"])
        got = runner.step(toks, ["a", "b"])
        assert torch.equal(_bits(want), _bits(got))
        eager_toks = [int(t) for t in want.argmax(-1)]
        nxt = torch.tensor(eager_toks, dtype=torch.long, device="cuda")
        toks.fill_(V - 1)  # the input this test made is garbage now; the next step gets a new tensor
        toks = nxt
    assert runner.stats["replays"] == 2


def test_warmup_captures_every_bucket_and_leaves_the_cache_alone():
    model = _model(2048)
    c1, toks = _prefilled(model, [_rand(20, 7)], ["a"], 40)
    c2 = copy.deepcopy(c1)
    before = [_bits(t) for t in c1.k + c1.v]
    runner = DecodeRunner(model, c1, 1).warmup()
    assert sorted(runner._graphs) == runner.widths() == [16, 32, 64, 128]
    assert runner.stats == {"graphs": 4, "replays": 0, "eager_warm": 4, "eager_fallback": 0}
    assert all(torch.equal(a, _bits(t)) for a, t in zip(before, c1.k + c1.v))
    got = runner.step(toks, ["a"])
    assert torch.equal(_bits(got), _bits(DecodeRunner(model, c2, 1, capture=False).step(toks, ["a"])))
    assert runner.stats["replays"] == 1 and runner.stats["graphs"] == 4


def test_quantize_weights_drops_the_graphs():
    torch.manual_seed(0)
    model = build_llama("llama3-tiny", device="cuda").eval()
    c1, toks = _prefilled(model, [_rand(12, 8)], ["a"], 16)
    runner = DecodeRunner(model, c1, 1)
    for _ in range(3):
        toks = [int(runner.step(toks, ["a"]).argmax(-1))]
    assert runner.stats["replays"] == 2
    model.quantize_weights_("fp8")
    c2 = copy.deepcopy(c1)
    got = runner.step(toks, ["a"]).clone()  # a fresh warm step on the quantised modules, not a replay of the old ones
    assert runner.stats["replays"] == 2 and runner.stats["eager_warm"] == 2 and not runner._graphs
    assert torch.equal(_bits(got), _bits(model.decode_step(toks, c2, ["a"])))


# ---------------------------------------------------------------------------------------- end to end
REQUESTS = [(_rand(7, 11), 12, {}), (_rand(40, 12), 5, dict(temperature=0.9, top_p=0.8, seed=4)),
            (_rand(23, 13), 9, dict(temperature=0.7, seed=2, repetition_penalty=1.2, frequency_penalty=0.3)),
            (_rand(3, 14), 14, {}), (_rand(9, 15), 3, {}), (_rand(130, 16), 7, dict(temperature=1.0, min_p=0.05, seed=9))]


def _serve(engine):
    for prompt, n, kw in REQUESTS:
        engine.add_request(list(prompt), n, **kw)
    events = []
    while engine.has_work():
        events.extend(engine.step())
    return events


def test_engine_events_do_not_depend_on_the_knob():
    model = _model()
    want = _serve(GenerationEngine(model, max_slots=4, num_blocks=64))
    on = GenerationEngine(model, max_slots=4, num_blocks=64, graph_decode=True)
    assert _serve(on) == want and len(want) == sum(n for _, n, _ in REQUESTS)
    assert on.runner.stats["replays"] > 0 and on.runner.stats["eager_fallback"] == 0


def test_deployment_status_reports_the_runner():
    from ray_community_amd.serve.llm import LlamaDeployment

    dep = LlamaDeployment.func_or_class("llama3-tiny", device="cuda", max_slots=2, num_blocks=32, graph_decode=True)

    async def run():
        toks = [t async for t in dep.generate(REQUESTS[0][0], max_new_tokens=8)]
        return toks, await dep.status()

    toks, st = asyncio.run(run())
    assert len(toks) == 8
    assert set(st["graph_decode"]) == {"graphs", "replays", "eager_warm", "eager_fallback"}
    assert st["graph_decode"]["replays"] > 0 and st["graph_decode"]["graphs"] == 1
    off = LlamaDeployment.func_or_class("llama3-tiny", device="cuda", max_slots=2, num_blocks=32)
    assert "graph_decode" not in asyncio.run(off.status())
