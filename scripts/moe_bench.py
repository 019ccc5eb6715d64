"""Mixture of experts on one MI355X: ``ops.moe_ffn``'s kernels against the grouped torch arm, and MoE ``generate``.

Op: at the mixtral-8x7b layer shape (E 8, k 2, H 4096, I 14336) and per T in {1, 8, 32, 64, 128, 256}, the
four launches of ``ops/csrc/moe.hip`` (``ops._moe_kernel``) and ``reference.moe_ffn_grouped`` (a sort, one host
read of the counts and two bf16 ``F.linear``s per expert in use) on the same routed batch, alternated round by
round in one process and timed with device events: median (min .. max) in us. ``TB/s`` is the bytes of the
expert weights actually touched (3 H I bf16 per expert that a row names) over the median. ``max_diff`` is the
largest difference of the two arms' outputs on that batch. ``M_MOE`` in ``ops/__init__.py`` is the largest
power-of-two T at which the kernels win.
End to end: ``Llama.generate`` tokens/s, eager against ``graph_decode=True``, on ``mixtral-tiny`` and on a
``mixtral-8x7b`` stack cut to ``--layers`` layers, at batch 1 and 8.

    python scripts/moe_bench.py [--rounds 7] [--layers 2] [--rows 1,8,...] [--no-e2e] [--json out.json] [--format mxfp4]

``--rows`` times other batch sizes, such as the thousands of rows of a captured prefill (one align workgroup).
``--format mxfp4``: the experts are MXFP4 (random nibbles and block scales). Three arms alternate: the W4 kernels
of ``ops/csrc/moe_w4.hip`` (``ops._moe_w4_kernel``), ``ops.moe_ffn_w4``'s dequantise-and-group arm and the bf16
kernels on the dequantised weights; ``TB/s`` is over the bytes the arm's weights occupy (17/32 of a byte a weight
for the first two). ``M_MOE_W4`` is the largest measured T at which the W4 kernels beat the dequantise-and-group
arm. The ``generate`` rows run with ``expert_dtype="mxfp4"``.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_community_amd import ops  # noqa: E402
from ray_community_amd.models import LLAMA_PRESETS, PagedKVCache, build_llama  # noqa: E402
from ray_community_amd.ops import reference as ref  # noqa: E402

TS = [1, 8, 32, 64, 128, 256]


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def _random_mxfp4(E, N, K, g):
    """Random nibbles and E8M0 bytes 8 wide around 2^-1 / (3 sqrt(K)): weights of the size 1 / sqrt(K), as the bf16 arm draws."""
    mid = 127 - 1 - round(math.log2(3 * K ** 0.5))
    q = torch.randint(0, 256, (E, N, K // 2), device="cuda", dtype=torch.uint8, generator=g)
    return q, torch.randint(mid - 4, mid + 4, (E, N, K // 32), device="cuda", dtype=torch.uint8, generator=g)


def op_bench(rounds, iters, rows_list=TS, fmt="bf16"):
    """bf16: the bf16 kernels ("hip") against the grouped torch arm. mxfp4: the W4 kernels ("hip") against the op's
    dequantise-and-group arm ("grouped") and the bf16 kernels on the dequantised weights ("bf16_hip")."""
    cfg = LLAMA_PRESETS["mixtral-8x7b"]
    H, I, E, k = cfg.hidden_size, cfg.intermediate_size, cfg.num_experts, cfg.experts_per_token
    g = torch.Generator(device="cuda").manual_seed(0)
    router = (torch.randn(E, H, device="cuda", generator=g) / H ** 0.5).bfloat16()
    if fmt == "mxfp4":
        quads = [t for name, N, K in (("gate_up", 2 * I, H), ("down", H, I)) for t in _random_mxfp4(E, N, K, g)]
        wgu, wd = (torch.stack([ops.dequant_w4(q[e], s[e]) for e in range(E)]) for q, s in (quads[:2], quads[2:]))
    else:
        wgu = (torch.randn(E, 2 * I, H, device="cuda", generator=g) / H ** 0.5).bfloat16()
        wd = (torch.randn(E, H, I, device="cuda", generator=g) / I ** 0.5).bfloat16()
    own = 3 * H * I * (17 / 32 if fmt == "mxfp4" else 2)  # an expert's resident bytes; the bf16 kernels stream bf16
    nbytes = {"hip": own, "grouped": own}
    rows = []
    for T in rows_list:
        x = torch.randn(T, H, device="cuda", dtype=torch.bfloat16, generator=g)
        ids, weights = ops.moe_route(x, router, k)
        assert ops.moe_supported(T, H, I, E, k, x, ids, weights, wgu, wd)
        out = torch.empty_like(x)
        if fmt == "mxfp4":
            assert ops.moe_w4_supported(T, H, I, E, k, x, ids, weights, *quads)

            def grouped():  # the op's own arm above M_MOE_W4 rows
                keep, ops.M_MOE_W4 = ops.M_MOE_W4, 0
                try:
                    return ops.moe_ffn_w4(x, ids, weights, *quads)
                finally:
                    ops.M_MOE_W4 = keep
            arms = {"hip": lambda: ops._moe_w4_kernel(x, ids, weights, *quads, out), "grouped": grouped,
                    "bf16_hip": lambda: ops._moe_kernel(x, ids, weights, wgu, wd, out)}
        else:
            arms = {"hip": lambda: ops._moe_kernel(x, ids, weights, wgu, wd, out),
                    "grouped": lambda: ref.moe_ffn_grouped(x, ids, weights, wgu, wd)}
        diff = (arms["hip"]().float() - arms["grouped"]().float()).abs().max().item()
        times = {name: [] for name in arms}
        for fn in arms.values():
            _time(fn, iters)
        for _ in range(rounds):
            for name, fn in arms.items():
                times[name].append(_time(fn, iters))
        used = int(torch.unique(ids).numel())
        row = {"T": T, "format": fmt, "experts_used": used, "weight_gb": used * nbytes["hip"] / 1e9, "max_diff": diff}
        for name, ts in times.items():
            med = statistics.median(ts)
            row[name] = {"us": med, "min_us": min(ts), "max_us": max(ts),
                         "tb_s": used * nbytes.get(name, 3 * H * I * 2) / med / 1e6}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def e2e_bench(name, layers, rounds, new_tokens=64, fmt="bf16"):
    torch.manual_seed(0)
    over = {} if layers is None else {"num_layers": layers}
    model = build_llama(name, device="cuda", max_seq_len=512, expert_dtype="mxfp4" if fmt == "mxfp4" else None, **over).eval()
    rows = []
    for batch in (1, 8):
        g = torch.Generator().manual_seed(batch)
        prompts = [torch.randint(0, model.cfg.vocab_size, (32,), generator=g).tolist() for _ in range(batch)]
        caches = {graph: PagedKVCache(model.cfg, batch * 8, 16, device="cuda") for graph in (False, True)}
        times = {False: [], True: []}
        for r in range(rounds + 1):  # round 0 warms both arms up (and captures the graphs)
            for graph in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(prompts, new_tokens, cache=caches[graph], graph_decode=graph)
                torch.cuda.synchronize()
                if r:
                    times[graph].append(batch * new_tokens / (time.perf_counter() - t0))
                assert all(len(o) == new_tokens for o in out)
        row = {"model": name, "layers": model.cfg.num_layers, "batch": batch, "new_tokens": new_tokens}
        for graph, label in ((False, "eager"), (True, "graph")):
            row[label] = {"tok_s": statistics.median(times[graph]), "min": min(times[graph]), "max": max(times[graph])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--rows", type=lambda s: [int(t) for t in s.split(",")], default=TS)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--format", choices=("bf16", "mxfp4"), default="bf16", help="the expert weights' format")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench.py needs a GPU")
    fmt = args.format
    result = {"device": torch.cuda.get_device_name(0), "format": fmt, "op": op_bench(args.rounds, args.iters, args.rows, fmt)}
    if not args.no_e2e:
        result["e2e"] = (e2e_bench("mixtral-tiny", None, args.rounds, fmt=fmt)
                         + e2e_bench("mixtral-8x7b", args.layers, args.rounds, fmt=fmt))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
