"""Sampling cost per decode step on one GPU: the per-row PyTorch sampler the engine used so far
against the batched HIP sampler (``ops.sample_logits``), and the engine end to end.

    python scripts/sample_bench.py [--rounds 20] [--skip-engine] [--out profiles/sampling.json]

Shape: V = 128256 bf16 logits (``randn * 4``), B in {1, 32, 256}, temperature 0.8, top_k 50 and
(where the arm has it) top_p 0.9. Arms, each timed with a host clock around work that ends in a
device synchronise (every arm ends in a host copy, which is part of what it costs a step):
  (a) ``sample_tokens`` per row plus ``int()``, as ``GenerationEngine`` samples by default;
  (b) ``sample_tokens`` once on the batch plus ``.tolist()``, top_k only (it has no top_p);
  (c) ``ops.sample_logits`` (top_k and top_p) plus ``.tolist()``: parameter copy, launch, host copy.
The arms are interleaved round by round after a warm-up of every shape; medians with min-max.
One more row times the kernel of (c) alone with device events and states it as a multiple of one
read of the logits at ``--stream-tbs`` (the project's measured stream rate, 6.5 TB/s).
End to end: tokens/s of a llama3-1b engine with 32 sampled slots, ``fused_sampling`` off and on,
alternating in one process. Prints one JSON line per measurement; a run without a GPU fails.

``--penalties`` and / or ``--logprobs N`` run these arms instead (``profiles/sampling_penalties.md``):
``ops.penalize_logits`` and ``ops.token_logprobs`` at B = 32, V = 128256, bf16, 4096 tokens of history
per row (1024 prompt + 3072 produced): the call as the decode round makes it (host lists: checks,
packing, one upload, launch; ended by a synchronise), the same call on device tensors, and the
kernel alone by device events; then llama3-1b ``generate`` tokens/s, 32 prompts of 512 tokens,
with and without them against the plain ``fused_sampling`` arm, alternating in one process.
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
from ray_community_amd.models.llama import sample_tokens  # noqa: E402

V, T, K, P = 128256, 0.8, 50, 0.9


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench_arms(B, rounds, stream_tbs):
    g = torch.Generator(device="cuda").manual_seed(1)
    logits = (torch.randn(B, V, device="cuda", generator=g) * 4).bfloat16()
    gens = [torch.Generator(device="cuda").manual_seed(b) for b in range(B)]
    step = [0]

    def arm_a():
        return [int(sample_tokens(logits[b][None], T, K, gens[b])[0]) for b in range(B)]

    def arm_b():
        return sample_tokens(logits, T, K, gens[0]).tolist()

    def arm_c():
        step[0] += 1
        return ops.sample_logits(logits, T, K, P, 0.0, seeds=1, steps=step[0]).tolist()

    arms = {"a_per_row_sample_tokens": arm_a, "b_batched_sample_tokens_topk_only": arm_b, "c_sample_logits": arm_c}
    for fn in arms.values():
        for _ in range(3):
            fn()
    ms = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            ms[name].append(_timed(fn))
    # kernel alone: device events around back-to-back launches of the C entry on prepared parameters
    import numpy as np

    from ray_community_amd.ops._lib import lib, stream_ptr

    packed = np.zeros((B, 8), dtype=np.int32)
    packed[:, 0], packed[:, 2] = np.array([T, P], dtype=np.float32).view(np.int32)
    packed[:, 1], packed[:, 4] = K, 1
    packed[:, 6] = np.arange(B)
    params = torch.from_numpy(packed).cuda()
    tokens = torch.empty(B, dtype=torch.int64, device="cuda")
    L, st = lib(), stream_ptr(logits.device)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kern, reps = [], 20
    for _ in range(rounds):
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            L.rca_sample_logits(logits.data_ptr(), logits.stride(0), 1, params.data_ptr(), 0, tokens.data_ptr(), B, V,
                                st)
        stop.record()
        torch.cuda.synchronize()
        kern.append(start.elapsed_time(stop) / reps)
    read_ms = B * V * 2 / (stream_tbs * 1e12) * 1e3
    out = {"B": B, "V": V, "dtype": "bf16", "rounds": rounds, "ms": {k: _stat(v) for k, v in ms.items()}}
    out["a_over_c"] = out["ms"]["a_per_row_sample_tokens"]["median"] / out["ms"]["c_sample_logits"]["median"]
    out["b_over_c"] = out["ms"]["b_batched_sample_tokens_topk_only"]["median"] / out["ms"]["c_sample_logits"]["median"]
    out["c_kernel_ms"] = _stat(kern)
    out["one_read_of_logits_ms"] = read_ms
    out["c_kernel_over_one_read"] = out["c_kernel_ms"]["median"] / read_ms
    return out


def bench_engine(rounds, slots=32, new_tokens=32):
    torch.manual_seed(0)
    model = build_llama("llama3-1b", device="cuda", dtype=torch.bfloat16).eval()
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, model.cfg.vocab_size, (24,), generator=g).tolist() for _ in range(slots)]

    def run(fused):
        eng = GenerationEngine(model, max_slots=slots, num_blocks=slots * 4 + 8, fused_sampling=fused)
        for i, p in enumerate(prompts):
            eng.add_request(p, new_tokens, temperature=T, top_k=K, seed=i)
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.has_work():
            n += len(eng.step())
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for fused in (False, True):
        run(fused)
    tps = {False: [], True: []}
    for _ in range(rounds):
        for fused in (False, True):
            tps[fused].append(run(fused))
    out = {"engine": "llama3-1b", "slots": slots, "new_tokens": new_tokens, "rounds": rounds,
           "tokens_per_s": {"fused_sampling_off": _stat(tps[False]), "fused_sampling_on": _stat(tps[True])}}
    tps = out["tokens_per_s"]
    out["on_over_off"] = tps["fused_sampling_on"]["median"] / tps["fused_sampling_off"]["median"]
    return out


def bench_penalty_ops(rounds, penalties, logprobs, B=32, hist=4096, prompt=1024):
    import numpy as np

    from ray_community_amd.ops._lib import lib, stream_ptr

    g = torch.Generator(device="cuda").manual_seed(1)
    logits = (torch.randn(B, V, device="cuda", generator=g) * 4).bfloat16()
    flat = torch.randint(0, V, (B * hist,), generator=torch.Generator().manual_seed(2)).tolist()
    ranges = [(b * hist, b * hist + prompt, (b + 1) * hist) for b in range(B)]
    tok_dev = torch.tensor(flat, dtype=torch.int32, device="cuda")
    rng_dev = torch.tensor(ranges, dtype=torch.int32, device="cuda")
    picked = ops.sample_logits(logits, T, K, P, 0.0, seeds=1, steps=0)
    L, st = lib(), stream_ptr(logits.device)
    arms, kernels = {}, {}
    if penalties:
        arms["penalize_logits_host_lists"] = lambda: ops.penalize_logits(logits, flat, ranges, 1.3, 0.4, 0.25)
        arms["penalize_logits_device_tensors"] = lambda: ops.penalize_logits(logits, tok_dev, rng_dev, 1.3, 0.4, 0.25)
        prm = torch.tensor([[1.3, 1 / 1.3, 0.25, 0.4]] * B, dtype=torch.float32, device="cuda")
        counts = torch.zeros(B * V, dtype=torch.int32, device="cuda")
        image = torch.empty(B, V, dtype=torch.float32, device="cuda")
        kernels["penalize_logits_kernel_ms"] = lambda: L.rca_penalize_logits(
            logits.data_ptr(), logits.stride(0), 1, tok_dev.data_ptr(), rng_dev.data_ptr(), prm.data_ptr(),
            counts.data_ptr(), image.data_ptr(), B, V, B * hist, st)
    if logprobs is not None:
        arms["token_logprobs"] = lambda: ops.token_logprobs(logits, picked, logprobs)
        lp = torch.empty(B, dtype=torch.float32, device="cuda")
        ids = torch.empty(B, max(logprobs, 1), dtype=torch.int64, device="cuda")
        tlp = torch.empty(B, max(logprobs, 1), dtype=torch.float32, device="cuda")
        kernels["token_logprobs_kernel_ms"] = lambda: L.rca_token_logprobs(
            logits.data_ptr(), logits.stride(0), 1, picked.data_ptr(), lp.data_ptr(), ids.data_ptr(), tlp.data_ptr(),
            B, V, logprobs, st)
    for fn in list(arms.values()) + list(kernels.values()):
        for _ in range(3):
            fn()
    ms = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            ms[name].append(_timed(fn))
    out = {"B": B, "V": V, "dtype": "bf16", "history": hist, "logprobs": logprobs, "rounds": rounds,
           "call_ms": {k: _stat(v) for k, v in ms.items()}}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn in kernels.items():
        kern, reps = [], 20
        for _ in range(rounds):
            torch.cuda.synchronize()
            start.record()
            for _ in range(reps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            kern.append(start.elapsed_time(stop) / reps)
        out[name] = _stat(kern)
    return out


def bench_penalty_generate(rounds, penalties, logprobs, batch=32, prompt_len=512, new_tokens=32):
    torch.manual_seed(0)
    model = build_llama("llama3-1b", device="cuda", dtype=torch.bfloat16).eval()
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, model.cfg.vocab_size, (prompt_len,), generator=g).tolist() for _ in range(batch)]
    pen = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.25)
    arms = {"plain_fused": {}}
    if penalties:
        arms["penalties"] = pen
    if logprobs is not None:
        arms["logprobs"] = {"logprobs": logprobs}
    if penalties and logprobs is not None:
        arms["penalties_and_logprobs"] = dict(pen, logprobs=logprobs)

    def run(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(prompts, new_tokens, temperature=T, top_k=K, seed=1, fused_sampling=True, **kw)
        torch.cuda.synchronize()
        toks = out[0] if "logprobs" in kw else out
        return sum(len(t) for t in toks) / (time.perf_counter() - t0)

    for kw in arms.values():
        run(kw)
    tps = {name: [] for name in arms}
    for _ in range(rounds):
        for name, kw in arms.items():
            tps[name].append(run(kw))
    out = {"generate": "llama3-1b", "batch": batch, "prompt_len": prompt_len, "new_tokens": new_tokens,
           "rounds": rounds, "tokens_per_s": {k: _stat(v) for k, v in tps.items()}}
    base = out["tokens_per_s"]["plain_fused"]["median"]
    out["over_plain"] = {k: v["median"] / base for k, v in out["tokens_per_s"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--engine-rounds", type=int, default=3)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--stream-tbs", type=float, default=6.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--penalties", action="store_true", help="the ops.penalize_logits arms instead of the sampler's")
    ap.add_argument("--logprobs", type=int, default=None, metavar="N", help="the ops.token_logprobs arms (N alternatives)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs a GPU: nothing here can be measured without one")
    results = []
    if a.penalties or a.logprobs is not None:
        results.append(bench_penalty_ops(a.rounds, a.penalties, a.logprobs))
        print(json.dumps(results[-1]), flush=True)
        if not a.skip_engine:
            results.append(bench_penalty_generate(a.engine_rounds, a.penalties, a.logprobs))
            print(json.dumps(results[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
        return
    for B in (1, 32, 256):
        results.append(bench_arms(B, a.rounds, a.stream_tbs))
        print(json.dumps(results[-1]), flush=True)
    if not a.skip_engine:
        results.append(bench_engine(a.engine_rounds))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
