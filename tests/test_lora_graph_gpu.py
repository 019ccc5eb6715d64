"""Device-built LoRA routing, the fused LoRA kernel and graphed LoRA decode rounds on the GPU.

The cases, float64 oracle and bound are those of tests/test_lora_cpu.py (``exact`` at K = 128: bit for bit);
the padded, poisoned operands and the sentinel guard band those of tests/test_lora_gpu.py. The fused kernel
must also equal the two-pass kernels bit for bit, on host routing and on device routing, and a replayed LoRA
round must equal ``Llama.decode_step`` bit for bit (llama3-tiny at ``max_seq_len = 256``: one attention split
at every width, as in tests/test_decode_graph_gpu.py).
"""
import copy

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models import DecodeRunner, LoraAdapter, PagedKVCache, build_llama
from test_lora_cpu import PATTERNS, S, case, fails, pattern_idx, splits
from test_lora_gpu import NAMES, PROMPTS, SLACK, _device_operands, _sentinel

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _device_routing(idx):
    return ops.lora_routing(torch.tensor(idx, dtype=torch.int32, device="cuda"), slots=S)


@pytest.mark.parametrize("M", [1, 17, 33, 70])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_device_routing_equals_host_routing(pattern, M):
    idx = pattern_idx(pattern, M)
    host = ops.lora_routing(idx)
    # no adapter, as the device reads it: -1, a slot past the bank, a negative number
    dev = _device_routing([v if v >= 0 else (-1, S, -7)[m % 3] for m, v in enumerate(idx)])
    n, cap = host.n_tiles, min(M, min(S, M) + M // 16)
    assert dev.n_tiles == cap >= n and dev.any and dev.num_rows == M
    assert tuple(dev.tile_slot.shape) == (cap,) and tuple(dev.tile_rows.shape) == (cap, 16)
    assert torch.equal(dev.tile_slot[:n].cpu(), host.tile_slot) and torch.equal(dev.tile_rows[:n].cpu(), host.tile_rows)
    assert (dev.tile_slot[n:] == -1).all() and (dev.tile_rows[n:] == -1).all()


@pytest.mark.parametrize("R", [16, 48, 64, 128])
@pytest.mark.parametrize("N,K", [(16, 128), (272, 1152), (16, 2048), (16, 8192)])
def test_fused_kernel_meets_the_oracle_and_equals_two_pass(N, K, R):
    assert splits(K, R) == {128: 1, 1152: 2, 2048: 4, 8192: 16 if R <= 64 else 8}[K] == ops.lib().rca_lora_splits(K, R)
    for sel, (M, pattern) in enumerate((M, p) for M in (1, 17, 33) for p in ("cycle", "big_and_single")):
        c = case("exact" if K == 128 else "coded", M, N, K, R, pattern)
        for routing in (ops.lora_routing(c["idx"], "cuda"), _device_routing(c["idx"])):
            whole = {}
            for kernel in ("fused", "two_pass"):
                x, ybuf, y, co, A, B, scale = _device_operands(c, sel)
                assert ops.lora_add_(y, x, A, B, scale, routing, kernel=kernel) is y
                whole[kernel] = ybuf.cpu()
            label = (N, K, R, M, pattern, routing.n_tiles)
            got = whole["fused"]
            assert torch.equal(_bits(got), _bits(whole["two_pass"])), label
            keep = torch.ones(got.shape, dtype=torch.bool)
            keep[SLACK:SLACK + M, co:co + N] = False
            assert torch.equal(_bits(got)[keep], _sentinel(*got.shape)[keep]), (label, "guard band written")
            fail, share = fails(c, got[SLACK:SLACK + M, co:co + N].contiguous())
            assert not fail.any(), (label, int(fail.sum()), share)


def test_fused_refuses_a_capacity_above_128_and_writes_nothing():
    c = case("coded", 33, 48, 384, 192, "cycle")
    x, A, B, scale = (c[k].cuda() for k in ("x", "A", "B", "scale"))
    y = _sentinel(33, 48).view(torch.bfloat16).cuda()
    with pytest.raises(ValueError, match="fused"):
        ops.lora_add_(y, x, A, B, scale, _device_routing(c["idx"]), kernel="fused")
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _sentinel(33, 48))
    ops.lora_add_(y, x, A, B, scale, _device_routing(c["idx"]), kernel="two_pass")  # R = 192 stays on the two-pass kernels
    assert not torch.equal(_bits(y), _sentinel(33, 48))


@pytest.mark.parametrize("N,K,R", [(272, 1152, 48), (16, 2048, 128)])
def test_fused_rows_do_not_depend_on_the_batch(N, K, R):
    M = 33
    c = case("coded", M, N, K, R, "cycle")
    x, y0, A, B, scale = (c[k].cuda() for k in ("x", "y0", "A", "B", "scale"))
    idx = c["idx"]

    def run(xs, ys, ids, route=_device_routing):
        return ops.lora_add_(ys.clone(), xs, A, B, scale, route(ids), kernel="fused")

    full = run(x, y0, idx)
    assert not fails(c, full.cpu())[0].any()
    for m in range(M):  # each row alone
        assert torch.equal(run(x[m:m + 1], y0[m:m + 1], idx[m:m + 1]), full[m:m + 1]), m
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(4))
    got = run(x[perm.cuda()].contiguous(), y0[perm.cuda()].contiguous(), [idx[p] for p in perm.tolist()],
              lambda ids: ops.lora_routing(ids, "cuda"))
    assert torch.equal(got, full[perm.cuda()])


@pytest.mark.parametrize("weights", [None, "fp8"], ids=["bf16", "fp8_weights"])
def test_lora_rounds_replay_a_graph_and_equal_decode_step(weights):
    torch.manual_seed(0)
    base = build_llama("llama3-tiny", device="cuda", max_seq_len=256, weight_dtype=weights).eval()
    model = copy.deepcopy(base).enable_lora_(max_adapters=3, max_rank=4)
    ads = [LoraAdapter.random(model.cfg, 4, seed=i) for i in (1, 2, 3)]
    model.load_adapter("a", ads[0])
    model.load_adapter("b", ads[1])

    cache = PagedKVCache(model.cfg, 32, 16, device="cuda")
    want = model.generate(PROMPTS, 8, adapters=NAMES)
    assert model.generate(PROMPTS, 8, adapters=NAMES, graph_decode=True, cache=cache) == want
    (runner,) = cache._decode_runners.values()
    assert runner.stats["eager_fallback"] == 0 and runner.stats["replays"] > 0 and runner.stats["graphs"] == 1

    ids = [0, 1, 2]
    c1 = PagedKVCache(model.cfg, 32, 16, device="cuda")
    toks = [int(t) for t in model.prefill(PROMPTS, None, c1, ids, adapters=NAMES).argmax(-1)]
    runner = DecodeRunner(model, copy.deepcopy(c1), 3)
    for step in range(10):
        kw = {} if step in (3, 4, 5) else {"adapters": NAMES}  # three rounds without adapters in between
        plain = None if kw else base.decode_step(toks, copy.deepcopy(c1), ids)
        if step == 8:  # another adapter into slot 0, in place: the graph exists and must see the new bytes
            model.unload_adapter("a")
            assert model.load_adapter("a", ads[2]) == 0
        eager = model.decode_step(toks, c1, ids, **kw)
        got = runner.step(toks, ids, **kw)
        assert torch.equal(_bits(eager), _bits(got)), step
        assert plain is None or torch.equal(_bits(plain), _bits(got)), step
        toks = [int(t) for t in eager.argmax(-1)]
    assert runner.stats == {"graphs": 2, "replays": 8, "eager_warm": 2, "eager_fallback": 0}
    with pytest.raises(ValueError, match="unknown adapter"):
        runner.step(toks, ids, adapters=["zzz", None, None])
    # warmup captures both kinds of round for every width and leaves the cache alone
    warmed = DecodeRunner(model, copy.deepcopy(c1), 3).warmup()
    assert warmed.stats["graphs"] == 2 * len(warmed.widths()) and warmed.stats["replays"] == 0
    got = warmed.step(toks, ids, adapters=NAMES)
    assert torch.equal(_bits(model.decode_step(toks, c1, ids, adapters=NAMES)), _bits(got)) and warmed.stats["replays"] == 1
