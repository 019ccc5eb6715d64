"""Multi-LoRA on one MI355X: the cost of ``ops.lora_add_`` per target linear, and of adapters in ``generate``.

Op: on the four layer shapes of llama3-8b (qkv, o, gate_up, down; bank capacity = parts x rank 16) and per
M in {1, 8, 32, 512}, ``ops.lora_add_`` (two launches) with all rows on one adapter and with every row on its
own adapter (32 slots, rows cycled over them), next to the bf16 ``F.linear`` of the base projection at the
same M. Timed with device events, medians (us). ``launch_floor_us`` is the same op on a 16 x 128 linear with
one row: two launches with next to no work, the floor that the launches alone set.
End to end: ``Llama.generate`` tokens/s at batch 1 and 32 under three arms -- the base model, the same
weights with LoRA enabled but no adapter named, and every sequence on its own adapter -- interleaved in one
process, with bf16 and with fp8 weights. ``extra_us_per_step`` is (time of the arm - time of the base arm) /
new tokens, so it carries the prompt's share of the difference too; ``launch_share`` is 8 launches x layers x
launch_floor_us / 2 over that.

    python scripts/lora_bench.py [--rounds 10] [--models llama3-8b,llama3-1b] [--no-e2e] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_community_amd import ops  # noqa: E402
from ray_community_amd.models import LLAMA_PRESETS, LoraAdapter, build_llama, weight_bytes  # noqa: E402
from ray_community_amd.models import lora as lora_mod  # noqa: E402

MS = [1, 8, 32, 512]
RANK, SLOTS = 16, 32


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def _median(fn, rounds, iters):
    _time(fn, iters)
    return statistics.median(_time(fn, iters) for _ in range(rounds))


def _op_case(M, N, K, R, g):
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16, generator=g)
    y = torch.randn(M, N, device="cuda", dtype=torch.bfloat16, generator=g)
    A = (torch.randn(SLOTS, R, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    B = (torch.randn(SLOTS, N, R, device="cuda", generator=g) * 0.02).bfloat16()
    scale = torch.full((SLOTS,), 2.0, device="cuda")
    assert ops.lora_supported(M, N, K, R, y, x, A, B, scale)
    return x, y, A, B, scale


def launch_floor(rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    x, y, A, B, scale = _op_case(1, 16, 128, 16, g)
    routing = ops.lora_routing([0], "cuda")
    return _median(lambda: ops.lora_add_(y, x, A, B, scale, routing), rounds, iters)


def op_bench(name, rounds, iters):
    cfg, rows = LLAMA_PRESETS[name], []
    g = torch.Generator(device="cuda").manual_seed(0)
    for target, (K, N) in lora_mod.target_dims(cfg).items():
        R = -(-len(lora_mod.PARTS[target]) * RANK // 16) * 16
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
        for M in MS:
            x, y, A, B, scale = _op_case(M, N, K, R, g)
            one = ops.lora_routing([0] * M, "cuda")
            own = ops.lora_routing([m % SLOTS for m in range(M)], "cuda")
            t_one = _median(lambda: ops.lora_add_(y, x, A, B, scale, one), rounds, iters)
            t_own = _median(lambda: ops.lora_add_(y, x, A, B, scale, own), rounds, iters)
            t_base = _median(lambda: F.linear(x, w), rounds, iters)
            rows.append(dict(model=name, linear=target, N=N, K=K, R=R, M=M, splits=ops.lib().rca_lora_splits(K, R),
                             one_adapter_us=round(t_one, 2), one_adapter_tiles=one.n_tiles,
                             own_adapter_us=round(t_own, 2), own_adapter_tiles=own.n_tiles,
                             base_linear_us=round(t_base, 2)))
            print(json.dumps(rows[-1]), flush=True)
        del w
    return rows


def e2e_bench(name, batches, new_tokens, prompt_len, reps, floor_us):
    rows = []
    for weights in ("bf16", "fp8"):
        torch.manual_seed(0)
        base = build_llama(name, device="cuda").eval()
        sd = {k: v.clone() for k, v in base.state_dict().items()}
        lora = build_llama(name, device="cuda").eval()
        lora.load_state_dict(sd)
        del sd
        if weights == "fp8":
            base.quantize_weights_("fp8")
            lora.quantize_weights_("fp8")
        base_bytes = weight_bytes(base)
        lora.enable_lora_(max_adapters=max(batches), max_rank=RANK)
        distinct = [LoraAdapter.random(lora.cfg, RANK, seed=i) for i in range(4)]  # the slots matter, not the values
        for i in range(max(batches)):
            lora.load_adapter(f"ad{i}", distinct[i % 4])
        for B in batches:
            g = torch.Generator().manual_seed(B)
            prompts = torch.randint(0, base.cfg.vocab_size, (B, prompt_len), generator=g).tolist()
            arms = (("base", base, {}), ("unused", lora, {}), ("own", lora, {"adapters": [f"ad{i}" for i in range(B)]}))
            secs = {arm: [] for arm, _, _ in arms}
            for rep in range(reps + 1):  # first repetition: warm-up; arms interleaved
                for arm, m, kw in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = m.generate(prompts, new_tokens, **kw)
                    torch.cuda.synchronize()
                    if rep:
                        secs[arm].append(time.perf_counter() - t0)
                    assert all(len(t) == new_tokens for t in out)
            med = {arm: statistics.median(v) for arm, v in secs.items()}
            extra = {arm: (med[arm] - med["base"]) / new_tokens * 1e6 for arm in ("unused", "own")}
            launches_us = 8 * base.cfg.num_layers * floor_us / 2
            rows.append(dict(model=name, weights=weights, batch=B, new_tokens=new_tokens, prompt_len=prompt_len,
                             **{f"{arm}_tok_s": round(B * new_tokens / med[arm], 1) for arm in med},
                             **{f"{arm}_min_max_s": [round(min(v), 4), round(max(v), 4)] for arm, v in secs.items()},
                             base_step_us=round(med["base"] / new_tokens * 1e6, 1),
                             unused_extra_us_per_step=round(extra["unused"], 1),
                             own_extra_us_per_step=round(extra["own"], 1),
                             launches_us_per_step=round(launches_us, 1),
                             launch_share=round(launches_us / extra["own"], 3) if extra["own"] > 0 else None,
                             base_weight_bytes=base_bytes, bank_bytes=lora_mod.bank_bytes(lora)))
            print(json.dumps(rows[-1]), flush=True)
        del base, lora
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--models", default="llama3-8b,llama3-1b")
    ap.add_argument("--no-op", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    floor_us = launch_floor(args.rounds, args.iters)
    result = {"device": torch.cuda.get_device_name(0), "rank": RANK, "launch_floor_us": round(floor_us, 2), "op": [],
              "generate": []}
    print(json.dumps({"launch_floor_us": result["launch_floor_us"]}), flush=True)
    if not args.no_op:
        result["op"] = op_bench("llama3-8b", args.rounds, args.iters)
    if not args.no_e2e:
        for name in args.models.split(","):
            result["generate"] += e2e_bench(name, (1, 32), args.new_tokens, args.prompt_len, args.reps, floor_us)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
