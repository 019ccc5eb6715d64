#!/usr/bin/env python3
"""Headline benchmark: Ray Train tokens/sec, Llama-3-8B DDP (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line: nothing else is
measured, so ``--full`` (the switch for every secondary measurement) has nothing to add here.
``--dump-outputs DIR`` saves what the last timed step computed (train/llm.py
``training_step_outputs``: the loss and a seeded sample of the updated weights and AdamW moments)
as ``DIR/<name>.npy`` in float32; weights and tokens are seeded, so two builds run with the same
arguments see identical inputs and can be compared output for output.

Two launch modes, same worker function:
  * self-launched (no torchrun): ``TorchTrainer(num_workers=N, use_gpu=True)`` starts N GPU
    worker actors in a local session; each sees the union of the group's GPUs in
    ``HIP_VISIBLE_DEVICES`` and joins an RCCL process group (``train/torch/config.py``);
  * under ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`` (the
    driver's multi-GPU launch): TorchTrainer binds to the launcher's ranks instead.
Either way ``n_gpus`` is the process group's world size and must equal ``--gpus``. The worker function is the framework's Train
loop (``ray_community_amd.train.llm.llama_train_loop_per_worker``): full forward + backward +
bucketed DDP all-reduce + fused AdamW step inside the timed region, bf16 compute, fp32 master
weights, random-init Llama-3-8B weights, synthetic tokens. Weak scaling (fixed per-GPU batch).
Rank 0 prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


# the headline (BASELINE.json) is DDP; the sharded modes are different algorithms and are never
# reported under its name
METRIC_BY_MODE = {"ddp": "ray_train_tokens_per_sec_llama3_8b_ddp", "zero": "ray_train_tokens_per_sec_llama3_8b_zero",
                  "fsdp": "ray_train_tokens_per_sec_llama3_8b_fsdp"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--micro-batch", type=int, default=2)
    ap.add_argument("--bucket-mb", type=float, default=256.0)
    ap.add_argument("--parallel", default="ddp", choices=["ddp", "zero", "fsdp", "auto"],
                    help="ddp (default, the headline metric: replicated AdamW after a bucketed RCCL all-reduce) | "
                         "zero (ZeRO-1/2 sharded AdamW over reduce-scatter + all-gather) | fsdp (ZeRO-3: parameters "
                         "sharded, per-block all-gather) | auto (ddp at N=1, zero for N>1). Modes other than ddp "
                         "report under their own metric name (..._zero / ..._fsdp)")
    ap.add_argument("--grad-reduce-dtype", default="bf16", choices=["bf16", "fp32"],
                    help="dtype of the gradient collective (fp32 = torch DDP-under-AMP parity)")
    ap.add_argument("--overlap-optimizer", action="store_true",
                    help="run the AdamW update per bucket on a side stream, overlapped with the next forward")
    ap.add_argument("--fused-ce", type=int, default=None, choices=[0, 1],
                    help="1: chunked lm_head + one-pass HIP cross-entropy (no T x V logits); default: model preset")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, save the last step's outputs (loss, a seeded sample of the updated "
                         "weights and AdamW moments) as DIR/<name>.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement; this benchmark has none, so the run is the plain one")
    ap.add_argument("--device", default="cuda", help="cuda (the benchmark) | cpu (gloo rehearsal of the launch path)")
    args = ap.parse_args()

    external = "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1
    world = int(os.environ["WORLD_SIZE"]) if external else args.gpus
    rank = int(os.environ.get("RANK", "0")) if external else 0
    if external and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} ranks")

    import ray_community_amd as ray
    from ray_community_amd.train import RunConfig, ScalingConfig
    from ray_community_amd.train.llm import llama_train_loop_per_worker
    from ray_community_amd.train.torch import TorchTrainer

    loop_config = {"model": args.model, "seq_len": args.seq_len, "micro_batch": args.micro_batch,
                   "steps": args.steps, "warmup": args.warmup, "bucket_cap_mb": args.bucket_mb, "parallel": args.parallel,
                   "grad_reduce_dtype": args.grad_reduce_dtype, "device": args.device,
                   "overlap_optimizer": args.overlap_optimizer}
    if args.dump_outputs:
        loop_config["dump_outputs"] = os.path.abspath(args.dump_outputs)  # the workers' cwd is not the driver's
        os.makedirs(loop_config["dump_outputs"], exist_ok=True)
    if args.fused_ce is not None:
        loop_config["model_overrides"] = {"fused_ce": bool(args.fused_ce)}
    # workers' own output stays in their log files: stdout carries exactly one JSON line
    if not external and args.device == "cpu":
        ray.init(num_cpus=max(2, args.gpus), include_dashboard=False, log_to_driver=False)
    elif not external:
        ray.init(include_dashboard=False, log_to_driver=False)
    # self-launched: TorchTrainer starts N worker actors (one per GPU, RCCL group over xGMI);
    # under torchrun it binds to the launcher's ranks and runs this rank's share of the job.
    trainer = TorchTrainer(llama_train_loop_per_worker, train_loop_config=loop_config,
                           scaling_config=ScalingConfig(num_workers=max(1, world), use_gpu=args.device == "cuda"),
                           run_config=RunConfig(name="bench_llama", storage_path="/tmp/rca_bench"))
    result = trainer.fit()
    m = result.metrics
    if int(m["world_size"]) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but training ran on a process group of {m['world_size']}")
    world = int(m["world_size"])
    if rank == 0:
        out = {
            "metric": METRIC_BY_MODE.get(m.get("parallel"), "ray_train_tokens_per_sec_llama3_8b_" + str(m.get("parallel"))),
            "value": round(m["tokens_per_s"], 2),
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(m["ms_per_step"], 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic (random tokens, random-init weights)",
            "config": {
                "model": args.model,
                "global_batch": args.micro_batch * world,
                "seq_len": args.seq_len,
                "parallelism": f"dp{world}",
                "parallel_mode": m.get("parallel"),
                "grad_reduce_dtype": m.get("grad_reduce_dtype"),
                "launch": "torchrun" if external else "TorchTrainer worker actors",
                "process_group": m.get("process_group"),
                "tokens_per_step": args.micro_batch * world * args.seq_len,
                "optimizer": "AdamW fp32 master (fused HIP)",
                "data_parallel": {
                    "ddp": "DDP: bucketed RCCL all-reduce, replicated fused AdamW",
                    "zero": "DDP with ZeRO-sharded AdamW: bucketed reduce-scatter + all-gather",
                    "fsdp": "ZeRO-3: per-block all-gather of sharded weights, reduce-scatter of grads",
                }.get(m.get("parallel"), m.get("parallel")),
            },
            "extra": {
                "loss": round(m["loss"], 4),
                "peak_mem_gb": round(m["mem_gb"], 2),
                "model_tflops_per_gpu": round(m["tokens_per_s"] / world * m["flops_per_token"] / 1e12, 1),
                # per-step compute-stream stall on gradient/parameter collectives (max over ranks)
                "exposed_comm_ms": round(float(m.get("exposed_comm_ms", 0.0)), 3),
                # each rank's own ms/step over the timed steps (the job's number is the max)
                "rank_ms_per_step_min": min(m.get("rank_ms_per_step") or [m["ms_per_step"]]),
                "rank_ms_per_step_max": max(m.get("rank_ms_per_step") or [m["ms_per_step"]]),
                "rank_ms_per_step": m.get("rank_ms_per_step"),
            },
        }
        print(json.dumps(out), flush=True)
    if external:
        import torch.distributed as dist

        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
    if ray.is_initialized():
        ray.shutdown()


if __name__ == "__main__":
    main()
