"""Paged extend attention and chunked prefill on one MI355X.

Kernel: ``ops.paged_attention_extend`` at Hq=32, Hk=8, D=128, page 16 for (B=4, prior context
3584, chunk 512) and (B=1, prior 0, chunk 4096), against ``F.scaled_dot_product_attention`` with
an explicit mask on the same K/V gathered contiguous beforehand (the gather is not timed, which
makes the baseline generous); the second shape also against ``ops.flash_attention_qkv``. FLOPs =
4 * D * Hq * (visible (query, key) pairs). The arms are interleaved round by round, timed with
device events, and reported as medians with min-max.
Engine: llama3-1b, one request decoding while a 4096-token prompt arrives; the longest gap between
that request's consecutive tokens and the newcomer's time to first token, for ``prefill_chunk``
None, 512 and 2048.

    python scripts/extend_bench.py [--rounds 20] [--no-engine] [--json out.json]

``--kv-dtype fp8`` measures the extend kernel over an FP8 KV cache against the bf16 cache instead,
both arms interleaved in one process, at (B=4, prior 3584, chunk 512) and at a 5-row verify shape
(B=8, prior 4091, split-KV by the default policy).
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
from ray_community_amd.models import GenerationEngine, build_llama  # noqa: E402


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def kernel_bench(rounds, iters, B, prior, chunk, Hq=32, Hk=8, D=128, page=16):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = prior + chunk
    pages = ctx // page
    num_blocks = B * pages
    W = (Hq + 2 * Hk) * D
    qkv = torch.randn(B * chunk, W, device=dev, dtype=torch.bfloat16, generator=g)
    k_cache = torch.randn(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16, generator=g)
    v_cache = torch.randn(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16, generator=g)
    table = torch.randperm(num_blocks, device=dev, generator=g).to(torch.int32).view(B, pages)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    cu = torch.arange(0, (B + 1) * chunk, chunk, dtype=torch.int32, device=dev)
    if prior == 0:  # the chunk's own K/V are the whole cache: the flash forward sees the same problem
        slots = (table.long()[:, :, None] * page + torch.arange(page, device=dev)).reshape(-1)
        k_cache.view(-1, Hk, D)[slots] = qkv[:, Hq * D: (Hq + Hk) * D].reshape(-1, Hk, D)
        v_cache.view(-1, Hk, D)[slots] = qkv[:, (Hq + Hk) * D:].reshape(-1, Hk, D)
    kg = k_cache[table.long()].reshape(B, ctx, Hk, D).transpose(1, 2).contiguous()
    vg = v_cache[table.long()].reshape(B, ctx, Hk, D).transpose(1, 2).contiguous()
    q4 = qkv[:, : Hq * D].reshape(B, chunk, Hq, D).transpose(1, 2).contiguous()
    pos = torch.arange(prior, ctx, device=dev)
    mask = torch.arange(ctx, device=dev)[None, :] <= pos[:, None]  # [chunk, ctx]

    arms = {"hip": lambda: ops.paged_attention_extend(qkv, k_cache, v_cache, table, lens, cu, chunk, Hq, Hk, D),
            "sdpa": lambda: F.scaled_dot_product_attention(q4, kg, vg, attn_mask=mask, enable_gqa=True)}
    if prior == 0 and ops.flash_attention_supported(chunk, D, Hq, Hk):
        arms["flash"] = lambda: ops.flash_attention_qkv(qkv, B, chunk, Hq, Hk, D, causal=True)
    a = arms["hip"]().float()
    b = arms["sdpa"]().transpose(1, 2).reshape(B * chunk, Hq * D).float()
    err = ((a - b).abs().max() / b.abs().max()).item()
    times = {k: [] for k in arms}
    for _ in range(2):  # warm-up
        for fn in arms.values():
            _time(fn, iters)
    for _ in range(rounds):  # interleaved arms
        for k, fn in arms.items():
            times[k].append(_time(fn, iters))
    flops = 4.0 * D * Hq * B * sum(range(prior + 1, ctx + 1))
    res = {"shape": dict(B=B, prior=prior, chunk=chunk, Hq=Hq, Hk=Hk, D=D, page=page), "rel_err_vs_sdpa": err}
    for k, t in times.items():
        us = statistics.median(t)
        res[k] = {"us": round(us, 1), "us_min_max": [round(min(t), 1), round(max(t), 1)],
                  "TFLOPs": round(flops / us / 1e6, 1)}
    return res


def fp8_kernel_bench(rounds, iters, B, prior, chunk, Hq=32, Hk=8, D=128, page=16, num_splits=1):
    """The extend kernel over a bf16 and over an fp8 cache holding the same K/V (N(0, 1), written
    by the two append kernels), interleaved round by round in this process."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = prior + chunk
    pages = -(-ctx // page)
    num_blocks = B * pages
    W = (Hq + 2 * Hk) * D
    qkv = torch.randn(B * chunk, W, device=dev, dtype=torch.bfloat16, generator=g)
    k_cache = torch.empty(num_blocks, page, Hk, D, device=dev, dtype=torch.bfloat16)
    v_cache = torch.empty_like(k_cache)
    k8 = torch.empty(num_blocks, page, Hk, D, device=dev, dtype=torch.float8_e4m3fn)
    v8 = torch.empty_like(k8)
    ks = torch.empty(num_blocks, page, Hk, device=dev, dtype=torch.float32)
    vs = torch.empty_like(ks)
    for s0 in range(0, num_blocks * page, 4096):
        n = min(4096, num_blocks * page - s0)
        rows = torch.randn(n, W, device=dev, dtype=torch.bfloat16, generator=g)
        slots = torch.arange(s0, s0 + n, device=dev, dtype=torch.int32)
        ops.kv_cache_append_(k_cache, v_cache, rows, slots, Hq, Hk, D)
        ops.kv_cache_append_(k8, v8, rows, slots, Hq, Hk, D, k_scale=ks, v_scale=vs)
    table = torch.randperm(num_blocks, device=dev, generator=g).to(torch.int32).view(B, pages)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    cu = torch.arange(0, (B + 1) * chunk, chunk, dtype=torch.int32, device=dev)
    arms = {"bf16": lambda: ops.paged_attention_extend(qkv, k_cache, v_cache, table, lens, cu, chunk, Hq, Hk, D,
                                                       num_splits=num_splits),
            "fp8": lambda: ops.paged_attention_extend(qkv, k8, v8, table, lens, cu, chunk, Hq, Hk, D,
                                                      num_splits=num_splits, k_scale=ks, v_scale=vs)}
    times = {k: [] for k in arms}
    for _ in range(2):  # warm-up
        for fn in arms.values():
            _time(fn, iters)
    for _ in range(rounds):  # interleaved arms
        for k, fn in arms.items():
            times[k].append(_time(fn, iters))
    flops = 4.0 * D * Hq * B * sum(range(prior + 1, ctx + 1))
    splits = num_splits or ops.paged_extend_num_splits(B, Hk, chunk, Hq // Hk, pages * page, page)
    res = {"shape": dict(B=B, prior=prior, chunk=chunk, Hq=Hq, Hk=Hk, D=D, page=page), "num_splits": splits}
    for k, t in times.items():
        us = statistics.median(t)
        res[k] = {"us": round(us, 1), "us_min_max": [round(min(t), 1), round(max(t), 1)],
                  "TFLOPs": round(flops / us / 1e6, 1)}
    return res


def engine_bench(model, prefill_chunk, prompt_len=4096, warm_tokens=8, reps=3):
    """Longest gap (ms) between consecutive tokens of a decoding request while a ``prompt_len``
    prompt arrives, and the newcomer's time to first token (ms). Median of ``reps``."""
    g = torch.Generator().manual_seed(1)
    V = model.cfg.vocab_size
    gaps, ttfts = [], []
    for _ in range(reps + 1):  # the first repetition is the warm-up
        eng = GenerationEngine(model, max_slots=4, num_blocks=2 * (prompt_len // 16) + 64, page_size=16,
                               prefill_chunk=prefill_chunk)
        a = eng.add_request(torch.randint(0, V, (64,), generator=g).tolist(), 400)
        stamps = []
        for _ in range(warm_tokens):
            eng.step()
        torch.cuda.synchronize()
        b = eng.add_request(torch.randint(0, V, (prompt_len,), generator=g).tolist(), 4)
        t0 = time.perf_counter()
        stamps.append(t0)
        ttft = None
        while ttft is None:
            ev = eng.step()
            torch.cuda.synchronize()
            now = time.perf_counter()
            if any(rid == a for rid, _, _ in ev):
                stamps.append(now)
            if any(rid == b for rid, _, _ in ev):
                ttft = now - t0
        gaps.append(max(y - x for x, y in zip(stamps, stamps[1:])) * 1e3)
        ttfts.append(ttft * 1e3)
        eng.cancel(a)
        eng.cancel(b)
    return {"prefill_chunk": prefill_chunk, "prompt_len": prompt_len,
            "max_gap_ms": round(statistics.median(gaps[1:]), 2),
            "max_gap_ms_min_max": [round(min(gaps[1:]), 2), round(max(gaps[1:]), 2)],
            "ttft_ms": round(statistics.median(ttfts[1:]), 2),
            "ttft_ms_min_max": [round(min(ttfts[1:]), 2), round(max(ttfts[1:]), 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: the extend kernel over an fp8 cache against the bf16 one, both arms in this process")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extend_bench.py needs a GPU")
    if args.kv_dtype == "fp8":
        # a chunked-prefill shape, and 5 draft rows to verify over a long context (split-KV)
        res = {"kernel": [fp8_kernel_bench(args.rounds, args.iters, 4, 3584, 512),
                          fp8_kernel_bench(args.rounds, args.iters, 8, 4091, 5, num_splits=None)]}
        for r in res["kernel"]:
            print(json.dumps(r), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    res = {"kernel": [kernel_bench(args.rounds, args.iters, 4, 3584, 512),
                      kernel_bench(args.rounds, args.iters, 1, 0, 4096)]}
    for r in res["kernel"]:
        print(json.dumps(r), flush=True)
    if not args.no_engine:
        torch.manual_seed(0)
        model = build_llama("llama3-1b", device="cuda").eval()
        res["engine"] = [engine_bench(model, c) for c in (None, 512, 2048)]
        for r in res["engine"]:
            print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
