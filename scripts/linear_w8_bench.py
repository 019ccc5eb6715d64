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

    python scripts/linear_w8_bench.py [--rounds 10] [--models llama3-8b,llama3-1b] [--no-e2e] [--json out.json]
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
from ray_community_amd.models import LLAMA_PRESETS, build_llama, weight_bytes  # noqa: E402
from ray_community_amd.ops import reference as ref  # noqa: E402

MS = [1, 2, 4, 8, 16, 32, 64, 128]


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


def kernel_bench(name, rounds, iters):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, N, K in shapes(name):
        w = torch.randn(N, K, device="cuda", generator=g) * 0.02
        q, s = ref.quantize_weight_fp8_ref(w)
        wd = ops.dequant_w8(q, s)
        del w
        for M in MS:
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
            a, b = [], []
            for _ in range(rounds):
                a.append(_time(fp8, iters))
                b.append(_time(bf16, iters))
            t8, t16 = statistics.median(a), statistics.median(b)
            rows.append(dict(model=name, linear=label, N=N, K=K, M=M, fp8_us=round(t8, 2), bf16_us=round(t16, 2),
                             fp8_min_max=[round(min(a), 2), round(max(a), 2)],
                             bf16_min_max=[round(min(b), 2), round(max(b), 2)],
                             fp8_weight_TBps=round(N * K / t8 * 1e-6, 3), bf16_weight_TBps=round(2 * N * K / t16 * 1e-6, 3),
                             rel_diff=round(err, 5)))
            print(json.dumps(rows[-1]), flush=True)
        del q, s, wd
    return rows


def e2e_bench(name, batches, new_tokens, prompt_len, reps):
    torch.manual_seed(0)
    model = build_llama(name, device="cuda").eval()
    bytes16 = weight_bytes(model)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    quant = build_llama(name, device="cuda").eval()
    quant.load_state_dict(sd)
    del sd
    quant.quantize_weights_("fp8")
    rows = []
    for B in batches:
        g = torch.Generator().manual_seed(B)
        prompts = torch.randint(0, model.cfg.vocab_size, (B, prompt_len), generator=g).tolist()
        times = {"bf16": [], "fp8": []}
        for rep in range(reps + 1):  # first repetition: warm-up; arms interleaved
            for arm, m in (("bf16", model), ("fp8", quant)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = m.generate(prompts, new_tokens)
                torch.cuda.synchronize()
                if rep:
                    times[arm].append(B * new_tokens / (time.perf_counter() - t0))
                assert all(len(t) == new_tokens for t in out)
        rows.append(dict(model=name, batch=B, new_tokens=new_tokens, prompt_len=prompt_len,
                         bf16_tok_s=round(statistics.median(times["bf16"]), 1),
                         fp8_tok_s=round(statistics.median(times["fp8"]), 1),
                         bf16_min_max=[round(min(times["bf16"]), 1), round(max(times["bf16"]), 1)],
                         fp8_min_max=[round(min(times["fp8"]), 1), round(max(times["fp8"]), 1)],
                         bf16_weight_bytes=bytes16, fp8_weight_bytes=weight_bytes(quant)))
        print(json.dumps(rows[-1]), flush=True)
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
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "M_SKINNY": ops.M_SKINNY, "kernel": [], "generate": []}
    for name in args.models.split(","):
        if not args.no_kernel:
            result["kernel"] += kernel_bench(name, args.rounds, args.iters)
        if not args.no_e2e:
            result["generate"] += e2e_bench(name, (1, 32), args.new_tokens, args.prompt_len, args.reps)
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
