"""Paged decode attention and end-to-end generation on one MI355X.

Kernel: ``ops.paged_attention_decode`` at B=32, context 4096, Hq=32, Hk=8, D=128, page 16 against
``F.scaled_dot_product_attention`` on the same K/V gathered contiguous beforehand (the gather is
not timed, which makes the baseline generous). KV bytes = 2 * B * ctx * Hk * D * 2. The two arms
are interleaved round by round, timed with device events, and reported as medians. The same
shape is also timed per split count and at G = 8 (Hq=64).
End to end: ``Llama.generate`` tokens/s for llama3-1b at batch 1 and batch 32.

    python scripts/decode_bench.py [--rounds 20] [--no-e2e] [--json out.json]
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
from ray_community_amd.models import build_llama  # noqa: E402


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def kernel_bench(rounds, iters, B=32, ctx=4096, Hq=32, Hk=8, D=128, page=16, num_splits=None):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    pages = ctx // page
    num_blocks = B * pages
    k_cache = torch.randn(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16, generator=g)
    v_cache = torch.randn(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16, generator=g)
    table = torch.randperm(num_blocks, device=dev, generator=g).to(torch.int32).view(B, pages)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    q = torch.randn(B, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    # baseline operands: the same K/V, gathered contiguous (not timed)
    kg = k_cache[table.long()].reshape(B, ctx, Hk, D).transpose(1, 2).contiguous()
    vg = v_cache[table.long()].reshape(B, ctx, Hk, D).transpose(1, 2).contiguous()
    q4 = q.view(B, Hq, 1, D)

    def hip():
        return ops.paged_attention_decode(q, k_cache, v_cache, table, lens, Hq, Hk, D, num_splits=num_splits)

    def sdpa():
        return F.scaled_dot_product_attention(q4, kg, vg, enable_gqa=True)

    a, b = hip().float(), sdpa().reshape(B, Hq * D).float()
    err = ((a - b).abs().max() / b.abs().max()).item()
    for _ in range(3):  # warm-up
        _time(hip, iters)
        _time(sdpa, iters)
    t_hip, t_sdpa = [], []
    for _ in range(rounds):  # interleaved arms
        t_hip.append(_time(hip, iters))
        t_sdpa.append(_time(sdpa, iters))
    kv_bytes = 2 * B * ctx * Hk * D * 2
    us_hip, us_sdpa = statistics.median(t_hip), statistics.median(t_sdpa)
    splits = num_splits or ops.lib().rca_attn_decode_num_splits(B, Hk, ctx, page)
    return {"shape": dict(B=B, ctx=ctx, Hq=Hq, Hk=Hk, D=D, page=page), "num_splits": splits,
            "hip_us": round(us_hip, 2), "hip_us_min_max": [round(min(t_hip), 2), round(max(t_hip), 2)],
            "hip_kv_GBps": round(kv_bytes / us_hip / 1e3, 1),
            "sdpa_us": round(us_sdpa, 2), "sdpa_us_min_max": [round(min(t_sdpa), 2), round(max(t_sdpa), 2)],
            "sdpa_kv_GBps": round(kv_bytes / us_sdpa / 1e3, 1), "speedup": round(us_sdpa / us_hip, 3),
            "rel_err_vs_sdpa": err}


def e2e_bench(batch, prompt_len=128, new_tokens=64, reps=3):
    torch.manual_seed(0)
    m = build_llama("llama3-1b", device="cuda").eval()
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, m.cfg.vocab_size, (batch, prompt_len), generator=g).tolist()
    m.generate(prompts, 8)  # warm-up
    rates = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(prompts, new_tokens)
        torch.cuda.synchronize()
        rates.append(sum(len(o) for o in out) / (time.perf_counter() - t0))
    return {"batch": batch, "prompt_len": prompt_len, "new_tokens": new_tokens,
            "tokens_per_s": round(statistics.median(rates), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench.py needs a GPU")
    res = {"kernel": kernel_bench(args.rounds, args.iters),
           "kernel_splits": [kernel_bench(max(args.rounds // 4, 3), args.iters, num_splits=s) for s in (1, 2, 4, 8)]}
    res["kernel_g8"] = kernel_bench(max(args.rounds // 2, 3), args.iters, Hq=64)  # G = 8: one wave per SIMD
    print(json.dumps(res["kernel"]), flush=True)
    print(json.dumps(res["kernel_g8"]), flush=True)
    for r in res["kernel_splits"]:
        print(json.dumps({k: r[k] for k in ("num_splits", "hip_us", "hip_kv_GBps")}), flush=True)
    if not args.no_e2e:
        res["generate"] = [e2e_bench(1), e2e_bench(32)]
        for r in res["generate"]:
            print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
