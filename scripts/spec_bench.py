"""Speculative decoding on one MI355X: the split-KV verify attention and the engine.

Kernel arm: ``ops.paged_attention_extend`` at Hq=32, Hk=8, D=128, page 16 for (B, prior context,
new tokens) in ``SHAPES``; arms ``num_splits`` = 1 (the unsplit launch), the heuristic's choice
(``None``) and a sweep over 2 / 4 / 8 / 16. Engine arm: llama3-1b bf16, greedy, batch 1 and 8,
a prompt with repeated spans, 256 new tokens; ``GenerationEngine(fused_sampling=True)`` against
``GenerationEngine(speculative=4)``: tokens/s, acceptance rate, tokens per verify step.

Arms are interleaved round by round, kernels timed with device events, and everything is reported
as a median with min-max.

    python scripts/spec_bench.py [--rounds 20] [--no-engine] [--no-kernel] [--json out.json]
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
from ray_community_amd.models import GenerationEngine, build_llama  # noqa: E402

SHAPES = [(1, 4096, 5), (1, 32768, 5), (8, 4096, 5), (32, 4096, 5), (4, 3584, 512)]
SWEEP = (2, 4, 8, 16)


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def kernel_bench(rounds, iters, B, prior, new, Hq=32, Hk=8, D=128, page=16):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = prior + new
    pages = -(-ctx // page)
    num_blocks = B * pages
    qkv = torch.randn(B * new, (Hq + 2 * Hk) * D, device=dev, dtype=torch.bfloat16, generator=g)
    k_cache = torch.randn(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16, generator=g)
    v_cache = torch.randn(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16, generator=g)
    table = torch.randperm(num_blocks, device=dev, generator=g).to(torch.int32).view(B, pages)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    cu = torch.arange(0, (B + 1) * new, new, dtype=torch.int32, device=dev)

    def arm(ns):
        return lambda: ops.paged_attention_extend(qkv, k_cache, v_cache, table, lens, cu, new, Hq, Hk, D,
                                                  num_splits=ns)

    chosen = ops.paged_extend_num_splits(B, Hk, new, Hq // Hk, pages * page, page)
    arms = {"1": arm(1), "heuristic": arm(None), **{str(n): arm(n) for n in SWEEP}}
    base = arms["1"]().float()
    err = {k: round(((fn().float() - base).abs().max() / base.abs().max()).item(), 5) for k, fn in arms.items()}
    times = {k: [] for k in arms}
    for _ in range(2):  # warm-up
        for fn in arms.values():
            _time(fn, iters)
    for _ in range(rounds):  # interleaved arms
        for k, fn in arms.items():
            times[k].append(_time(fn, iters))
    res = {"shape": dict(B=B, prior=prior, new=new, Hq=Hq, Hk=Hk, D=D, page=page), "heuristic_picks": chosen,
           "rel_diff_vs_unsplit": err}
    for k, t in times.items():
        res[k] = {"us": round(statistics.median(t), 1), "us_min_max": [round(min(t), 1), round(max(t), 1)]}
    return res


def repeated_prompt(V, seed, length=192, span=24):
    """A prompt made of a few spans, each occurring several times (what prompt lookup feeds on)."""
    g = torch.Generator().manual_seed(seed)
    spans = [torch.randint(0, V, (span,), generator=g).tolist() for _ in range(3)]
    out = []
    while len(out) < length:
        out += spans[int(torch.randint(0, 3, (1,), generator=g))]
    return out[:length]


def engine_run(model, batch, speculative, new_tokens=256):
    eng = GenerationEngine(model, max_slots=batch, num_blocks=batch * 32 + 8, page_size=16, fused_sampling=True,
                           speculative=speculative)
    for b in range(batch):
        eng.add_request(repeated_prompt(model.cfg.vocab_size, b), new_tokens)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while eng.has_work():
        n += len(eng.step())
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), dict(eng.spec_stats)


def engine_bench(model, batch, reps):
    arms = {"plain": None, "speculative4": 4}
    rates, stats = {k: [] for k in arms}, {}
    for rep in range(reps + 1):  # the first repetition is the warm-up
        for k, spec in arms.items():  # interleaved arms
            r, st = engine_run(model, batch, spec)
            if rep:
                rates[k].append(r)
                stats[k] = st
    res = {"batch": batch}
    for k, r in rates.items():
        res[k] = {"tokens_per_s": round(statistics.median(r), 1),
                  "tokens_per_s_min_max": [round(min(r), 1), round(max(r), 1)]}
    st = stats["speculative4"]
    res["speculative4"].update(st, acceptance=round(st["accepted"] / max(st["drafted"], 1), 3),
                               tokens_per_verify_step=round(st["emitted"] / max(st["verify_steps"], 1), 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_bench.py needs a GPU")
    res = {}
    if not args.no_kernel:
        res["kernel"] = []
        for shape in SHAPES:
            res["kernel"].append(kernel_bench(args.rounds, args.iters, *shape))
            print(json.dumps(res["kernel"][-1]), flush=True)
    if not args.no_engine:
        torch.manual_seed(0)
        model = build_llama("llama3-1b", device="cuda").eval()
        res["engine"] = []
        for batch in (1, 8):
            res["engine"].append(engine_bench(model, batch, args.reps))
            print(json.dumps(res["engine"][-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
