"""Paged decode attention and end-to-end generation on one MI355X.

Kernel: ``ops.paged_attention_decode`` at B=32, context 4096, Hq=32, Hk=8, D=128, page 16 against
``F.scaled_dot_product_attention`` on the same K/V gathered contiguous beforehand (the gather is
not timed, which makes the baseline generous). KV bytes = 2 * B * ctx * Hk * D * 2. The two arms
are interleaved round by round, timed with device events, and reported as medians. The same
shape is also timed per split count and at G = 8 (Hq=64).
End to end: ``Llama.generate`` tokens/s for llama3-1b at batch 1 and batch 32.

    python scripts/decode_bench.py [--rounds 20] [--no-e2e] [--json out.json]

``--kv-dtype fp8`` measures the FP8 KV cache instead: the bf16-cache and fp8-cache decode kernels
on the same K/V, interleaved in one process, at the shape above, at G = 8 and at B=1 with context
32768 (us, effective KV TB/s, the bf16 arm's min-max), and ``generate`` tokens/s at batch 32 with
both cache dtypes.
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


def fp8_kernel_bench(rounds, iters, B=32, ctx=4096, Hq=32, Hk=8, D=128, page=16):
    """The bf16-cache and the fp8-cache decode on the same K/V (N(0, 1), quantised by the append
    kernel), interleaved round by round in this process; the fp8 kernel at both step sizes.
    Effective KV bytes: 2 * B * ctx * Hk * D * 2 for bf16, 2 * B * ctx * Hk * (D + 4) for fp8."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    pages = ctx // page
    num_blocks = B * pages
    W = (Hq + 2 * Hk) * D
    k_cache = torch.empty(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16)
    v_cache = torch.empty_like(k_cache)
    k8 = torch.empty(num_blocks, page, Hk, D, device=dev, dtype=torch.float8_e4m3fn)
    v8 = torch.empty_like(k8)
    ks = torch.empty(num_blocks, page, Hk, device=dev, dtype=torch.float32)
    vs = torch.empty_like(ks)
    rows = 4096
    for s0 in range(0, num_blocks * page, rows):  # fill both caches through the two append kernels
        n = min(rows, num_blocks * page - s0)
        qkv = torch.randn(n, W, device=dev, dtype=torch.bfloat16, generator=g)
        slots = torch.arange(s0, s0 + n, device=dev, dtype=torch.int32)
        ops.kv_cache_append_(k_cache, v_cache, qkv, slots, Hq, Hk, D)
        ops.kv_cache_append_(k8, v8, qkv, slots, Hq, Hk, D, k_scale=ks, v_scale=vs)
    table = torch.randperm(num_blocks, device=dev, generator=g).to(torch.int32).view(B, pages)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    q = torch.randn(B, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    set_step = ops.lib().rca_attn_decode_fp8_set_step

    def bf16():
        return ops.paged_attention_decode(q, k_cache, v_cache, table, lens, Hq, Hk, D)

    def fp8(step):
        def run():
            set_step(step)
            return ops.paged_attention_decode(q, k8, v8, table, lens, Hq, Hk, D, k_scale=ks, v_scale=vs)
        return run

    arms = {"bf16": bf16, "fp8_step32": fp8(32), "fp8_step16": fp8(16)}
    a, b = bf16().float(), arms["fp8_step32"]().float()
    moved = ((a - b).abs().amax(-1) / a.abs().amax(-1)).max().item()  # what the quantisation itself moves
    times = {k: [] for k in arms}
    for _ in range(3):  # warm-up
        for fn in arms.values():
            _time(fn, iters)
    for _ in range(rounds):  # interleaved arms
        for k, fn in arms.items():
            times[k].append(_time(fn, iters))
    set_step(32)
    nbytes = {"bf16": 2 * B * ctx * Hk * D * 2}
    nbytes["fp8_step32"] = nbytes["fp8_step16"] = 2 * B * ctx * Hk * (D + 4)
    res = {"shape": dict(B=B, ctx=ctx, Hq=Hq, Hk=Hk, D=D, page=page),
           "num_splits": ops.lib().rca_attn_decode_num_splits(B, Hk, ctx, page), "fp8_vs_bf16_row_diff": moved}
    for k, t in times.items():
        us = statistics.median(t)
        res[k] = {"us": round(us, 2), "us_min_max": [round(min(t), 2), round(max(t), 2)],
                  "kv_TBps": round(nbytes[k] / us / 1e6, 3)}
    res["fp8_over_bf16_time"] = round(res["fp8_step32"]["us"] / res["bf16"]["us"], 3)
    res["byte_floor"] = round((D + 4) / (2 * D), 3)
    return res


def fp8_e2e_bench(batch=32, prompt_len=128, new_tokens=64, reps=3):
    """``generate`` tokens/s on llama3-1b with both cache dtypes, repetitions interleaved."""
    torch.manual_seed(0)
    m = build_llama("llama3-1b", device="cuda").eval()
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, m.cfg.vocab_size, (batch, prompt_len), generator=g).tolist()
    rates = {None: [], "fp8": []}
    for kv in rates:
        m.generate(prompts, 8, kv_cache_dtype=kv)  # warm-up
    for _ in range(reps):
        for kv in rates:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(prompts, new_tokens, kv_cache_dtype=kv)
            torch.cuda.synchronize()
            rates[kv].append(sum(len(o) for o in out) / (time.perf_counter() - t0))
    return {"batch": batch, "prompt_len": prompt_len, "new_tokens": new_tokens,
            "bf16_tokens_per_s": round(statistics.median(rates[None]), 1),
            "bf16_tokens_per_s_min_max": [round(min(rates[None]), 1), round(max(rates[None]), 1)],
            "fp8_tokens_per_s": round(statistics.median(rates["fp8"]), 1)}


def fp8_main(args):
    res = {"kernel": [fp8_kernel_bench(args.rounds, args.iters),                      # the README's shape
                      fp8_kernel_bench(args.rounds, args.iters, Hq=64),               # G = 8
                      fp8_kernel_bench(args.rounds, args.iters, B=1, ctx=32768)]}     # one long sequence
    for r in res["kernel"]:
        print(json.dumps(r), flush=True)
    if not args.no_e2e:
        res["generate"] = fp8_e2e_bench()
        print(json.dumps(res["generate"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: the fp8-cache kernels against the bf16-cache ones, both arms in this process")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench.py needs a GPU")
    if args.kv_dtype == "fp8":
        res = fp8_main(args)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
        return
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
