"""FP8 weights on one MI355X: the W8A16 kernel against bf16 ``F.linear``, and ``generate`` tokens/s.

Kernel: per linear shape of llama3-8b and llama3-1b (qkv, o, gate_up, down, lm_head) and per M in
{1, 2, 4, 8, 16, 32, 64, 128}, ``ops._linear_w8_kernel`` (the kernel path of ``ops.linear_w8`` whatever
``M_SKINNY`` is) against ``F.linear`` on the dequantised bf16 weight. Both arms run in one process,
interleaved round by round, timed with device events, reported as medians (us) with the kernel's
achieved bytes/s of its own weight bytes (N * K). Both arms re-read a weight that an earlier iteration
may have left in the 256 MB last-level cache; shapes above that size (gate_up, lm_head of the 8B
model in bf16) stream from HBM.
End to end: ``Llama.generate`` tokens/s, bf16 weights against fp8 weights of the same random-init
model in the same run, at batch 1 and 32.
``--format mxfp4`` adds a third arm to both: ``ops._linear_w4_kernel`` on the MXFP4 quantisation of the
same weight (its own bytes: N * K / 2 nibbles + N * K / 32 scales) and a model quantised to MXFP4.

``--mid`` (how ``ops.M_MID`` / ``ops.M_MID_W4`` are set): per format and llama3-8b shape, for M in
{33, 48, 64, 96, 128, 192, 256, 384, 512, 1024}, four arms interleaved round by round: ``kernel="mid"``,
``kernel="dequant"`` (dequantise + ``F.linear``, what a quantised model runs above the thresholds),
``kernel="skinny"``, and bf16 ``F.linear`` on a resident bf16 weight for context. Medians (us) with min and
max, the mid arm's TB/s of its own weight bytes and TF/s, and per format the largest M of the grid up to
which the mid arm is no slower than the dequant arm on every shape (a tie within the arms' spread goes
to the mid arm).

    python scripts/linear_w8_bench.py [--rounds 10] [--models llama3-8b,llama3-1b] [--no-e2e] [--json out.json]
                                      [--format mxfp4] [--ms 1,16,32,64] [--graph-decode] [--mid]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_community_amd import ops  # noqa: E402
from ray_community_amd.models import LLAMA_PRESETS, PagedKVCache, build_llama, weight_bytes  # noqa: E402
from ray_community_amd.ops import reference as ref  # noqa: E402

MS = [1, 2, 4, 8, 16, 32, 64, 128]
MID_MS = [33, 48, 64, 96, 128, 192, 256, 384, 512, 1024]


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def shapes(name):
    cfg = LLAMA_PRESETS[name]
    H, I, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    return [("qkv", (cfg.num_heads + 2 * cfg.num_kv_heads) * D, H), ("o", H, cfg.num_heads * D),
            ("gate_up", 2 * I, H), ("down", H, I), ("lm_head", cfg.vocab_size, H)]


def kernel_bench(name, rounds, iters, ms, mxfp4):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, N, K in shapes(name):
        w = torch.randn(N, K, device="cuda", generator=g) * 0.02
        q, s = ref.quantize_weight_fp8_ref(w)
        wd = ops.dequant_w8(q, s)
        q4, e4 = ref.quantize_weight_mxfp4_ref(w) if mxfp4 else (None, None)
        del w
        for M in ms:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16, generator=g)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            assert ops.linear_w8_supported(M, N, K, x, q, s, out)

            def fp8():
                return ops._linear_w8_kernel(x, q, s, out)

            def bf16():
                return F.linear(x, wd)

            err = ((fp8().float() - bf16().float()).abs().max() / bf16().float().abs().max()).item()
            for _ in range(2):
                _time(fp8, iters), _time(bf16, iters)
            extra = {}
            if mxfp4:
                assert ops.linear_w4_supported(M, N, K, x, q4, e4, out)
                wd4 = ops.dequant_w4(q4, e4)

                def mx():
                    return ops._linear_w4_kernel(x, q4, e4, out)

                ref4 = F.linear(x, wd4).float()
                extra["mxfp4_rel_diff"] = round(((mx().float() - ref4).abs().max() / ref4.abs().max()).item(), 5)
                del wd4, ref4
                _time(mx, iters), _time(mx, iters)
            a, b, c4 = [], [], []
            for _ in range(rounds):  # the timed rounds: every arm in every round
                a.append(_time(fp8, iters))
                b.append(_time(bf16, iters))
                if mxfp4:
                    c4.append(_time(mx, iters))
            t8, t16 = statistics.median(a), statistics.median(b)
            if mxfp4:
                t4 = statistics.median(c4)
                extra.update(mxfp4_us=round(t4, 2), mxfp4_min_max=[round(min(c4), 2), round(max(c4), 2)],
                             mxfp4_weight_TBps=round((N * K // 2 + N * K // 32) / t4 * 1e-6, 3))
            rows.append(dict(model=name, linear=label, N=N, K=K, M=M, fp8_us=round(t8, 2), bf16_us=round(t16, 2), **extra,
                             fp8_min_max=[round(min(a), 2), round(max(a), 2)],
                             bf16_min_max=[round(min(b), 2), round(max(b), 2)],
                             fp8_weight_TBps=round(N * K / t8 * 1e-6, 3), bf16_weight_TBps=round(2 * N * K / t16 * 1e-6, 3),
                             rel_diff=round(err, 5)))
            print(json.dumps(rows[-1]), flush=True)
        del q, s, wd, q4, e4
    return rows


def mid_bench(name, rounds, iters, ms):
    rows, chosen = [], {}
    g = torch.Generator(device="cuda").manual_seed(0)
    for fmt in ("mxfp4", "fp8"):
        ok = {M: True for M in ms}
        for label, N, K in shapes(name):
            w = torch.randn(N, K, device="cuda", generator=g) * 0.02
            if fmt == "mxfp4":
                linear, (q, s), wbytes = ops.linear_w4, ref.quantize_weight_mxfp4_ref(w), N * K // 2 + N * K // 32
                wd = ops.dequant_w4(q, s)
            else:
                linear, (q, s), wbytes = ops.linear_w8, ref.quantize_weight_fp8_ref(w), N * K
                wd = ops.dequant_w8(q, s)
            del w
            for M in ms:
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16, generator=g)
                out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
                arms = {a: (lambda a=a: linear(x, q, s, out=out, kernel=a)) for a in ("mid", "dequant", "skinny")}
                arms["bf16"] = lambda: F.linear(x, wd)
                same = torch.equal(arms["mid"]().clone(), arms["skinny"]())
                for fn in arms.values():
                    _time(fn, iters)
                t = {a: [] for a in arms}
                for _ in range(rounds):  # the timed rounds: every arm in every round
                    for a, fn in arms.items():
                        t[a].append(_time(fn, iters))
                med = {a: statistics.median(v) for a, v in t.items()}
                spread = max((max(v) - min(v)) / med[a] for a, v in t.items() if a in ("mid", "dequant"))
                ok[M] &= med["mid"] <= med["dequant"] * (1 + spread)
                rows.append(dict(format=fmt, linear=label, N=N, K=K, M=M, **{f"{a}_us": round(med[a], 2) for a in arms},
                                 **{f"{a}_min_max": [round(min(v), 2), round(max(v), 2)] for a, v in t.items()},
                                 spread=round(spread, 3), mid_weight_TBps=round(wbytes / med["mid"] * 1e-6, 3),
                                 mid_TFps=round(2.0 * M * N * K / med["mid"] * 1e-6, 1), mid_equals_skinny=same))
                print(json.dumps(rows[-1]), flush=True)
            del q, s, wd
        chosen[fmt] = max([m for i, m in enumerate(ms) if all(ok[v] for v in ms[:i + 1])], default=None)
        print(json.dumps({"format": fmt, "mid_no_slower_on_every_shape": ok, "largest_M": chosen[fmt]}), flush=True)
    return rows, chosen


def e2e_bench(name, batches, new_tokens, prompt_len, reps, mxfp4=False, graph_decode=False):
    torch.manual_seed(0)
    model = build_llama(name, device="cuda").eval()
    bytes16 = weight_bytes(model)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    quant = build_llama(name, device="cuda").eval()
    quant.load_state_dict(sd)
    del sd
    quant.quantize_weights_("fp8")
    arms = [("bf16", model), ("fp8", quant)]
    if mxfp4:
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        arms.append(("mxfp4", build_llama(name, device="cuda").eval()))
        arms[-1][1].load_state_dict(sd)
        del sd
        arms[-1][1].quantize_weights_("mxfp4")
    rows = []
    for B in batches:
        g = torch.Generator().manual_seed(B)
        prompts = torch.randint(0, model.cfg.vocab_size, (B, prompt_len), generator=g).tolist()
        times = {arm: [] for arm, _ in arms}
        # graphed arms keep one cache each, so one runner and its graphs live across the repetitions and no
        # graph is destroyed while another arm captures
        blocks = B * -(-(prompt_len + new_tokens + 8) // 16)
        caches = {arm: PagedKVCache(m.cfg, blocks, 16, device="cuda") for arm, m in arms} if graph_decode else {}
        for rep in range(reps + 1):  # first repetition: warm-up; arms interleaved
            for arm, m in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kw = {"graph_decode": True, "cache": caches[arm]} if graph_decode else {}
                out = m.generate(prompts, new_tokens, **kw)
                torch.cuda.synchronize()
                if rep:
                    times[arm].append(B * new_tokens / (time.perf_counter() - t0))
                assert all(len(t) == new_tokens for t in out)
        rows.append(dict(model=name, batch=B, new_tokens=new_tokens, prompt_len=prompt_len,
                         bf16_tok_s=round(statistics.median(times["bf16"]), 1),
                         fp8_tok_s=round(statistics.median(times["fp8"]), 1),
                         bf16_min_max=[round(min(times["bf16"]), 1), round(max(times["bf16"]), 1)],
                         fp8_min_max=[round(min(times["fp8"]), 1), round(max(times["fp8"]), 1)],
                         bf16_weight_bytes=bytes16, fp8_weight_bytes=weight_bytes(quant), graph_decode=graph_decode,
                         **({"mxfp4_tok_s": round(statistics.median(times["mxfp4"]), 1),
                             "mxfp4_min_max": [round(min(times["mxfp4"]), 1), round(max(times["mxfp4"]), 1)],
                             "mxfp4_weight_bytes": weight_bytes(arms[-1][1])} if mxfp4 else {})))
        print(json.dumps(rows[-1]), flush=True)
        del caches, kw
        gc.collect()  # drop the arms' graphs here, not in the middle of the next batch's captures
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--models", default="llama3-8b,llama3-1b")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--format", default="fp8", choices=["fp8", "mxfp4"], help="mxfp4: add the MXFP4 arm")
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--graph-decode", action="store_true", help="generate(graph_decode=True) in every arm")
    ap.add_argument("--mid", action="store_true", help="the mid-M arms on llama3-8b's shapes instead of the kernel table")
    args = ap.parse_args()
    mxfp4 = args.format == "mxfp4"
    result = {"device": torch.cuda.get_device_name(0), "M_SKINNY": ops.M_SKINNY, "M_SKINNY_W4": ops.M_SKINNY_W4,
              "M_MID": ops.M_MID, "M_MID_W4": ops.M_MID_W4, "kernel": [], "generate": []}
    if args.mid:
        ms = MID_MS if args.ms == ",".join(map(str, MS)) else [int(m) for m in args.ms.split(",")]
        result["mid"], result["mid_largest_M"] = mid_bench("llama3-8b", args.rounds, args.iters, ms)
    for name in args.models.split(","):
        if not args.no_kernel and not args.mid:
            result["kernel"] += kernel_bench(name, args.rounds, args.iters, [int(m) for m in args.ms.split(",")], mxfp4)
        if not args.no_e2e:
            result["generate"] += e2e_bench(name, [int(b) for b in args.batches.split(",")], args.new_tokens,
                                            args.prompt_len, args.reps, mxfp4, args.graph_decode)
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
