"""Graphed decode on one MI355X: ``generate`` with ``graph_decode`` off and on, and the fused
RoPE + cache-append kernel against the two kernels it replaces.

Generate: ``Llama.generate`` tokens/s per (model, weights, KV dtype, batch) with the knob off and on,
the two arms interleaved in one process over repetitions (the first one warms up and, for the graph
arm, captures: each arm keeps one cache, so the runner and its graphs live across repetitions).
Medians. Step: the decode step alone, ``model.decode_step`` against ``runner.step``, ``--steps``
calls back to back with one synchronisation at the end, so ``*_step_ms`` is wall time per step with
the host free to run ahead. ``gpu_ms`` is the device time of one replay of the captured graph (events
around ``replay()``, median): the step's kernels with no host in between, which are the eager step's
kernels too. ``*_host_ms`` = ``*_step_ms`` - ``gpu_ms``: what the arm spends per step beyond the
kernels.

Op: ``ops.rope_kv_append_decode_`` against ``apply_rope_`` + ``kv_cache_append_`` on llama3-8b shapes
at B = 1 and 32, bf16 and fp8 cache, device events, medians (us).

    python scripts/decode_graph_bench.py [--models llama3-1b,llama3-8b] [--batches 1,8,32] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_community_amd import ops  # noqa: E402
from ray_community_amd.models import DecodeRunner, PagedKVCache, build_llama  # noqa: E402


def _events(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def _median(fn, rounds, iters):
    _events(fn, iters)
    return statistics.median(_events(fn, iters) for _ in range(rounds))


def op_bench(rounds, iters):
    Hq, Hk, D, page, W = 32, 8, 128, 16, 64
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    cs = ops.rope_cos_sin(W * page, D).cuda()
    for fp8 in (False, True):
        for B in (1, 32):
            num_blocks = B * W
            qkv = torch.randn(B, (Hq + 2 * Hk) * D, device="cuda", generator=g).bfloat16()
            shape = (num_blocks, page, Hk, D)
            kv = [torch.zeros(shape, device="cuda", dtype=torch.float8_e4m3fn if fp8 else torch.bfloat16) for _ in range(2)]
            sc = [torch.ones(shape[:3], device="cuda") for _ in range(2)] if fp8 else [None, None]
            table = torch.arange(num_blocks, dtype=torch.int32, device="cuda").view(B, W)
            lens = torch.full((B,), 500, dtype=torch.int32, device="cuda")
            positions = lens - 1
            slots = (table[:, 499 // page] * page + 499 % page).to(torch.int32)

            def fused():
                ops.rope_kv_append_decode_(qkv, cs, kv[0], kv[1], table, lens, Hq, Hk, D, k_scale=sc[0], v_scale=sc[1])

            def two():
                ops.apply_rope_(qkv, cs, 1, Hq, Hk, D, positions)
                ops.kv_cache_append_(kv[0], kv[1], qkv, slots, Hq, Hk, D, k_scale=sc[0], v_scale=sc[1])

            rows.append(dict(cache="fp8" if fp8 else "bf16", B=B, fused_us=round(_median(fused, rounds, iters), 2),
                             two_kernels_us=round(_median(two, rounds, iters), 2)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def _wall(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3  # ms


def model_bench(name, batches, new_tokens, prompt_len, reps, steps):
    rows = []
    for weights, kv_dtype in (("bf16", None), ("fp8", None), ("bf16", "fp8")):
        torch.manual_seed(0)
        model = build_llama(name, device="cuda", weight_dtype=weights if weights == "fp8" else None).eval()
        page = 16
        for B in batches:
            g = torch.Generator().manual_seed(B)
            prompts = torch.randint(0, model.cfg.vocab_size, (B, prompt_len), generator=g).tolist()
            need = B * -(-(prompt_len + new_tokens + 2 * steps + 8) // page)
            caches = {arm: PagedKVCache(model.cfg, need, page, device="cuda", kv_dtype=kv_dtype) for arm in ("off", "on")}
            secs = {"off": [], "on": []}
            for rep in range(reps + 1):  # first repetition: warm-up and capture; arms interleaved
                for arm in ("off", "on"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = model.generate(prompts, new_tokens, cache=caches[arm], graph_decode=arm == "on")
                    torch.cuda.synchronize()
                    if rep:
                        secs[arm].append(time.perf_counter() - t0)
                    assert all(len(t) == new_tokens for t in out)
            (runner,) = caches["on"]._decode_runners.values()
            gen_stats = dict(runner.stats)
            med = {arm: statistics.median(v) for arm, v in secs.items()}
            # the decode step alone, at the context length the generation ends at
            ids = [("bench", b) for b in range(B)]
            toks = [1] * B
            for arm in ("off", "on"):
                model.prefill(prompts, None, caches[arm], ids)
            step = {"off": lambda: model.decode_step(toks, caches["off"], ids), "on": lambda: runner.step(toks, ids)}
            for arm in ("off", "on"):
                _wall(step[arm], 3)
            wall = {arm: [] for arm in step}
            for _ in range(2):
                for arm in ("off", "on"):
                    wall[arm].append(_wall(step[arm], steps // 2 - 2))
            graph = runner._graphs[runner.width_for(caches["on"].blocks_held(ids[0]))]
            gpu_ms = _median(graph.replay, 5, 10) / 1e3
            for arm in ("off", "on"):
                for sid in ids:
                    caches[arm].free(sid)
            off_ms, on_ms = min(wall["off"]), min(wall["on"])
            rows.append(dict(model=name, weights=weights, kv=kv_dtype or "bf16", batch=B, new_tokens=new_tokens,
                             prompt_len=prompt_len, off_tok_s=round(B * new_tokens / med["off"], 1),
                             on_tok_s=round(B * new_tokens / med["on"], 1),
                             generate_speedup=round(med["off"] / med["on"], 3),
                             off_min_max_s=[round(min(secs["off"]), 4), round(max(secs["off"]), 4)],
                             on_min_max_s=[round(min(secs["on"]), 4), round(max(secs["on"]), 4)],
                             off_step_ms=round(off_ms, 3), on_step_ms=round(on_ms, 3), gpu_ms=round(gpu_ms, 3),
                             off_host_ms=round(off_ms - gpu_ms, 3), on_host_ms=round(on_ms - gpu_ms, 3),
                             step_speedup=round(off_ms / on_ms, 3), generate_stats=gen_stats))
            print(json.dumps(rows[-1]), flush=True)
            del caches, runner, graph, step
        del model
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama3-1b,llama3-8b")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64, help="decode steps of the step-alone timing, per arm")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-op", action="store_true")
    ap.add_argument("--no-generate", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "op": [], "generate": []}
    if not args.no_op:
        result["op"] = op_bench(args.rounds, args.iters)
    if not args.no_generate:
        for name in args.models.split(","):
            result["generate"] += model_bench(name, [int(b) for b in args.batches.split(",")], args.new_tokens,
                                              args.prompt_len, args.reps, args.steps)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
