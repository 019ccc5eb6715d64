"""Fused flat AdamW with fp32 master weights.

One HIP kernel launch per weight-decay group streams (fp32 master, bf16/f32 grad, m, v) ->
(master, m, v, bf16 model weights) at HBM rate. Gradient averaging (1/world from DDP) and
global-norm clipping (norm read from device memory) are folded into the same pass, so the
step needs no host synchronisation and no extra elementwise passes.
Works on any ``FlatParameters`` (CPU tensors use the PyTorch reference math).

Master format (``master_format``): "split" (the GPU bf16 default) keeps only the LOW 16 bits of
each fp32 master beside the bf16 model weight, which holds the high half rounded (the pair
reconstructs the master bit-exactly; ``ops.reference.split_master``): 26 instead of 28 B of HBM
traffic per parameter per step and 2 B/param less memory. "fp32" keeps a separate fp32 master.

Layering: ``adamw_update_`` updates one contiguous range (the only caller of the ``rca_adamw*``
range kernels and of the CPU reference); ``AdamWBase`` holds what every AdamW here shares (state,
step preamble, global norm, state dict); ``FlatAdamW`` (this file), ``ShardedAdamW`` (``fsdp.py``)
and ``FullyShardedAdamW`` (``fully_sharded.py``) add their buffer layout and the loop over it.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist

from .. import ops
from ..ops._lib import check, lib, stream_ptr
from .flat import FlatParameters


class AdamWStep(NamedTuple):
    """What one optimizer step hands to every ``adamw_update_`` of that step."""
    lr: float
    b1: float
    b2: float
    eps: float
    bc1: float
    bc2: float
    step: int
    grad_scale: float
    clip: float            # max global grad norm, 0.0 = no clipping
    sumsq: torch.Tensor    # [1] global sum of squared (unscaled) gradients; the kernels read it
    cpu_coef: float        # the clip coefficient, taken on the host for CPU tensors only


def _grad_dtype_code(g: torch.Tensor) -> int:
    if g.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"unsupported grad dtype {g.dtype}")
    return 0 if g.dtype == torch.bfloat16 else 1


def adamw_update_(weights, grad, m, v, hp: AdamWStep, wd: float, *, master=None, lo=None, stream=None):
    """One AdamW update of a contiguous range, given as equal-length 1-D views.

    ``lo`` given: split master (``weights`` holds the bf16 high halves). ``master`` given: fp32
    master, bf16 copy written to ``weights``. Neither: fp32 ``weights`` updated in place.
    ``stream``: raw HIP stream (default: the current stream of the gradient's device)."""
    n = grad.numel()
    if any(t is not None and t.numel() != n for t in (weights, m, v, master, lo)):
        raise ValueError("adamw_update_ needs views of equal length")  # a slice past a buffer's end is cut short
    if n == 0:
        return
    if grad.is_cuda:
        rest = (grad.data_ptr(), _grad_dtype_code(grad), m.data_ptr(), v.data_ptr(), n, hp.lr, hp.b1, hp.b2, hp.eps,
                wd, hp.bc1, hp.bc2, hp.grad_scale, hp.sumsq.data_ptr() if hp.clip else 0, float(hp.clip),
                stream_ptr(grad.device) if stream is None else stream)
        if lo is not None:
            check(lib().rca_adamw_split(weights.data_ptr(), lo.data_ptr(), *rest), "adamw_split")
        elif master is not None:
            check(lib().rca_adamw(master.data_ptr(), weights.data_ptr(), *rest), "adamw")
        else:
            check(lib().rca_adamw(weights.data_ptr(), 0, *rest), "adamw")
        return
    p = ops.reference.join_master(weights, lo) if lo is not None else (weights if master is None else master)
    ops.reference.adamw_ref(p, grad, m, v, hp.lr, hp.b1, hp.b2, hp.eps, wd, hp.step, grad_mul=hp.grad_scale,
                            clip=hp.cpu_coef)
    if lo is not None:
        hi, lo_ = ops.reference.split_master(p)
        weights.copy_(hi)
        lo.copy_(lo_)
    elif master is not None:
        weights.copy_(master.to(weights.dtype))


class AdamWBase:
    """State and step preamble shared by the flat, ZeRO and fully sharded AdamW. A subclass sets
    its layout attributes, then calls ``__init__`` with the weights it owns (one 1-D tensor), and
    sets ``_shard`` to its data-parallel wrapper (rank, world, pg) if its state is a shard."""
    _shard = None

    def __init__(self, weights: torch.Tensor, lr, betas, eps, weight_decay, max_grad_norm, lr_schedule,
                 master_weights: bool = True, master_format: str = "fp32"):
        self.lr = lr
        self.b1, self.b2 = betas
        self.eps = eps
        self.wd = weight_decay
        self.max_grad_norm = max_grad_norm
        self.lr_schedule = lr_schedule
        self.step_count = 0
        n, dev = weights.numel(), weights.device
        self.master_weights = master_weights and weights.dtype != torch.float32
        self.split_master = _use_split(master_format, self.master_weights, weights)
        self.lo = torch.zeros(n, dtype=torch.int16, device=dev) if self.split_master else None
        self._master = None if self.split_master else (weights.float() if self.master_weights else weights)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._grad_scale = 1.0

    @property
    def param_groups(self):  # minimal torch.optim compatibility for LR schedulers / logging
        return [{"lr": self.lr, "weight_decay": self.wd}]

    def current_lr(self) -> float:
        return self.lr_schedule(self.step_count) if self.lr_schedule else self.lr

    @property
    def clip(self) -> float:
        return self.max_grad_norm if self.max_grad_norm and self.max_grad_norm > 0 else 0.0

    def _owned_weights(self) -> torch.Tensor:
        """The model-dtype weights this optimizer updates, in the order of ``m`` / ``v``."""
        raise NotImplementedError

    @property
    def master(self) -> torch.Tensor:
        """fp32 master of the owned elements (split format: reconstructed, a fresh tensor)."""
        if self.split_master:
            return ops.reference.join_master(self._owned_weights(), self.lo)
        return self._master

    def _global_sumsq(self, grads, pg=None, world: int = 1):
        """Sum of squares of ``grads`` over all ranks into ``_sumsq`` (no host sync)."""
        ops.grad_sumsq(grads, out=self._sumsq)
        if world > 1:
            dist.all_reduce(self._sumsq, group=pg)

    def _begin_step(self, grad_scale: float) -> AdamWStep:
        """Bump the step and fix its scalars; call once ``_sumsq`` holds this step's norm (when
        clipping). Only a CPU ``_sumsq`` is read here: the GPU kernels read it on the device."""
        self._grad_scale = grad_scale
        self.step_count += 1
        t = self.step_count
        clip, coef = self.clip, 1.0
        if clip and not self._sumsq.is_cuda:
            nrm = math.sqrt(float(self._sumsq)) * abs(grad_scale)
            coef = min(1.0, clip / (nrm + 1e-6))
        return AdamWStep(self.current_lr(), self.b1, self.b2, self.eps, 1.0 - self.b1 ** t, 1.0 - self.b2 ** t, t,
                         grad_scale, clip, self._sumsq, coef)

    def _update(self, weights, grad, a: int, b: int, wd: float, hp: AdamWStep, stream=None):
        """``adamw_update_`` of optimizer state [a, b) against equal-length weight / grad views."""
        master = self._master[a:b] if self.master_weights and not self.split_master else None
        lo = self.lo[a:b] if self.split_master else None
        adamw_update_(weights, grad, self.m[a:b], self.v[a:b], hp, wd, master=master, lo=lo, stream=stream)

    def grad_norm(self) -> float:
        """Global grad norm of the last step (host sync — call only for logging)."""
        return math.sqrt(float(self._sumsq.item())) * abs(self._grad_scale)

    def state_dict(self):
        """The optimizer state (for a sharded optimizer: this rank's shard, one file per rank)."""
        sd = {"step": self.step_count, "m": self.m, "v": self.v, "master": self.master if self.master_weights else None}
        if self._shard is not None:
            sd.update(rank=self._shard.rank, world=self._shard.world)
        sd.update(lr=self.lr, betas=(self.b1, self.b2), eps=self.eps, wd=self.wd)
        return sd

    def _load_moments(self, sd):
        if self._shard is not None and sd.get("world", self._shard.world) != self._shard.world:
            raise ValueError("sharded optimizer state was saved with a different world size")
        self.step_count = sd["step"]
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])


class FlatAdamW(AdamWBase):
    def __init__(self, flat: FlatParameters, lr: float = 3e-4, betas=(0.9, 0.95), eps: float = 1e-8,
                 weight_decay: float = 0.1, max_grad_norm: Optional[float] = 1.0, master_weights: bool = True,
                 lr_schedule=None, master_format: str = "auto"):
        self.flat = flat
        super().__init__(flat.data, lr, betas, eps, weight_decay, max_grad_norm, lr_schedule, master_weights,
                         master_format)
        self.last_grad_norm = None  # device tensor (sum of squares, pre-scale)
        self.track_grad_norm = False
        self._ov = None  # forward-overlap state (overlap_with_forward)
        # transposed bf16 weights W^T refreshed by the update itself (see _setup_transposed)
        self.transposed_weights = (self.split_master and flat.data.is_cuda
                                   and os.environ.get("RCA_ADAMW_WT", "1") != "0")
        self._wt_epoch = [0]  # bumped whenever the weights change outside the fused update
        self._wt_params = None
        self._segs = None

    # ------------------------------------------------------------------ forward overlap
    def overlap_with_forward(self, module: "torch.nn.Module", enabled: bool = True):
        """Run the update bucket by bucket on a side HIP stream, overlapped with the NEXT forward.

        AdamW is HBM-bound (28 B/param: ~37 ms for 8B params at ~6 TB/s) while the forward is
        MFMA-bound, so instead of a serial optimizer pass the update of each gradient bucket is
        issued on its own stream in the order the next forward consumes the weights (the no-decay
        tail holding the norm weights, then buckets from the END of the layout = the first
        layers) and a forward pre-hook on every module with parameters waits only for the
        buckets holding those parameters. A forward hook on the root waits for the whole update
        (and the gradient zeroing that follows it) before the loss is returned, so backward never
        races the optimizer. Same update rule and result as the serial step.
        """
        if self._ov is not None:
            for h in self._ov["hooks"]:
                h.remove()
            self._ov = None
        if not enabled or not self.flat.device.type == "cuda":
            return self
        flat = self.flat
        mod_buckets = {}
        hooks = []
        for m in module.modules():
            bis = sorted({flat.param_bucket[id(p)] for p in m.parameters(recurse=False) if id(p) in flat.param_bucket})
            if bis:
                mod_buckets[id(m)] = bis
                hooks.append(m.register_forward_pre_hook(self._ov_pre_forward))
        hooks.append(module.register_forward_hook(self._ov_post_forward))
        tail = [b.index for b in flat.buckets if b.start >= flat.decay_end]
        order = tail + [b.index for b in reversed(flat.buckets) if b.index not in tail]
        self._ov = {"stream": torch.cuda.Stream(device=flat.device), "mod_buckets": mod_buckets, "hooks": hooks,
                    "order": order, "events": [None] * len(flat.buckets), "done": None,
                    "evs": [torch.cuda.Event() for _ in flat.buckets], "done_ev": torch.cuda.Event()}
        return self

    def _ov_pre_forward(self, m, args):
        ov = self._ov
        if ov is None or ov["done"] is None:  # no update in flight
            return
        cur = torch.cuda.current_stream(self.flat.device)
        for bi in ov["mod_buckets"].get(id(m), ()):
            ev = ov["events"][bi]
            if ev is not None:
                cur.wait_event(ev)
                ov["events"][bi] = None

    def _ov_post_forward(self, m, args, out):
        self.wait_pending_update()

    def wait_pending_update(self):
        """Make the current stream wait for an in-flight overlapped update (no host sync)."""
        ov = self._ov
        if ov is not None and ov["done"] is not None:
            torch.cuda.current_stream(self.flat.device).wait_event(ov["done"])
            ov["done"] = None
            ov["events"] = [None] * len(self.flat.buckets)

    def _owned_weights(self) -> torch.Tensor:
        return self.flat.data

    def _setup_transposed(self):
        """W^T buffers for the fused-wgrad linear weights + the segment table of the update.

        Each ``FusedWgradLinear`` weight W [R, C] (R, C multiples of 128) gets a persistent bf16
        ``W^T`` [C, R] (``p._rca_wt``) that the segmented update kernel rewrites from the new
        weights in the same pass (one extra 2-B write per parameter); the backward dgrad reads it
        instead of transposing W (``parallel/fused_linear.py::weight_t``). Validity is keyed on
        (p._version, epoch): in-place edits of a weight or a bumped epoch (load_state_dict,
        sync_master, an update that did not refresh W^T) make the backward fall back to a
        transpose pass into the same buffer."""
        flat = self.flat
        mats = []
        for p in flat.fused:
            if p.dim() == 2 and p.shape[0] % 128 == 0 and p.shape[1] % 128 == 0:
                p._rca_wt = torch.empty(p.shape[1], p.shape[0], dtype=p.dtype, device=p.device)
                p._rca_wt_key = None
                p._rca_wt_epoch = self._wt_epoch
                mats.append((flat.param_offset[id(p)], p))
        mats.sort(key=lambda t: t[0])
        rows, blk = [], 0

        def add_range(s, e):
            nonlocal blk
            # split at the weight-decay boundary: a 1-D segment carries one decay flag
            for a, b in ((s, min(e, flat.decay_end)), (max(s, flat.decay_end), e)):
                if b > a:
                    rows.append([a, b - a, blk, 0, 0, 0, int(a < flat.decay_end), 0])
                    blk += (b - a + 4095) // 4096

        cur = 0
        for off, p in mats:
            add_range(cur, off)
            R, C = p.shape
            rows.append([off, p.numel(), blk, p._rca_wt.data_ptr(), R, C, int(off < flat.decay_end), 0])
            blk += (R // 128) * (C // 128)
            cur = off + p.numel()
        add_range(cur, flat.numel)
        self._wt_params = [p for _, p in mats]
        self._segs = torch.tensor(rows, dtype=torch.int64, device=flat.device)
        self._seg_blocks = blk

    def sync_master(self):
        """Re-read model weights into the fp32 master copy (after load_state_dict)."""
        self._wt_epoch[0] += 1
        if self.split_master:
            self.lo.zero_()
        elif self.master_weights:
            self._master.copy_(self.flat.data.float())

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        flat = self.flat
        flat.finalize_fresh()
        g = flat.step_grad
        pre, flat.precomputed_sumsq = flat.precomputed_sumsq, None
        if self.clip or self.track_grad_norm:
            if pre is not None and pre.device == self._sumsq.device:
                self._sumsq.copy_(pre)  # taken during backward (DistributedDataParallel precompute_grad_norm)
            else:
                self._global_sumsq([g])
            self.last_grad_norm = self._sumsq  # sqrt taken lazily by grad_norm()
        hp = self._begin_step(grad_scale)
        self._wt_epoch[0] += 1  # every update changes W: W^T is stale unless refreshed below
        ov = self._ov  # None on CPU
        if ov is None and self.transposed_weights:
            gdt = _grad_dtype_code(g)
            if self._segs is None:
                self._setup_transposed()
            check(lib().rca_adamw_split_seg(
                flat.data.data_ptr(), self.lo.data_ptr(), g.data_ptr(), gdt,
                self.m.data_ptr(), self.v.data_ptr(), self._segs.data_ptr(), self._segs.shape[0],
                self._seg_blocks, hp.lr, self.b1, self.b2, self.eps, self.wd, hp.bc1, hp.bc2, grad_scale,
                self._sumsq.data_ptr() if hp.clip else 0, float(hp.clip), stream_ptr(g.device)), "adamw_split_seg")
            ep = self._wt_epoch[0]
            for p in self._wt_params:
                p._rca_wt_key = (p._version, ep)
            return
        if ov is None:
            for s, e, wd in ((0, flat.decay_end, self.wd), (flat.decay_end, flat.numel, 0.0)):
                self._update(flat.data[s:e], g[s:e], s, e, wd, hp)
            return
        # overlapped: the side stream starts once the gradients (and their norm) are final
        self.wait_pending_update()
        main = torch.cuda.current_stream(g.device)
        side = ov["stream"]
        side.wait_stream(main)
        for bi in ov["order"]:
            b = flat.buckets[bi]
            s, e = b.start, min(b.end, flat.numel)
            self._update(flat.data[s:e], g[s:e], s, e, self.wd if s < flat.decay_end else 0.0, hp, side.cuda_stream)
            ev = ov["evs"][bi]
            ev.record(side)
            ov["events"][bi] = ev
        ov["done_ev"].record(side)
        ov["done"] = ov["done_ev"]
        ov["pending_zero"] = True

    def grad_norm(self) -> float:
        return super().grad_norm() if self.last_grad_norm is not None else 0.0

    def zero_grad(self, set_to_none: bool = False):
        ov = self._ov
        if ov is not None and ov.get("pending_zero") and ov["done"] is not None:
            # the update is still reading the gradients on the side stream: zero behind it there
            ov["pending_zero"] = False
            side = ov["stream"]
            with torch.cuda.stream(side):
                self.flat.zero_grad()
            ov["done"].record(side)
            return
        self.flat.zero_grad()

    def state_dict(self):
        self.wait_pending_update()
        return super().state_dict()

    def load_state_dict(self, sd):
        self._wt_epoch[0] += 1
        self._load_moments(sd)
        if self.master_weights and sd.get("master") is not None:
            if self.split_master:
                hi, lo = ops.reference.split_master(sd["master"].to(self.flat.device))
                self.flat.data.copy_(hi)
                self.lo.copy_(lo)
            else:
                self._master.copy_(sd["master"])
                self.flat.data.copy_(self._master.to(self.flat.dtype))


def _use_split(master_format: str, master_weights: bool, data: torch.Tensor) -> bool:
    """"auto": the split master on GPU bf16 models; "split" / "fp32" force the choice."""
    if master_format not in ("auto", "split", "fp32"):
        raise ValueError(f"master_format must be auto|split|fp32, got {master_format!r}")
    ok = master_weights and data.dtype == torch.bfloat16
    if master_format == "split" and not ok:
        raise ValueError("the split master format needs bf16 model weights with master_weights=True")
    if master_format == "auto":
        return ok and data.is_cuda and os.environ.get("RCA_ADAMW_SPLIT", "1") != "0"
    return master_format == "split"


class FlatSGD:
    """SGD with (Nesterov) momentum and weight decay over a ``FlatParameters`` buffer.

    The whole model is one contiguous tensor, so the update is three streaming passes over the
    flat buffers regardless of how many layers the model has (ResNet-50: 161 tensors -> 1).
    ``grad_scale`` (1/world from DDP) is folded into the momentum update.
    Reference semantics: ``torch.optim.SGD`` (momentum buffer initialised to the first gradient).
    """

    def __init__(self, flat: FlatParameters, lr: float = 0.1, momentum: float = 0.9, weight_decay: float = 0.0,
                 nesterov: bool = False, lr_schedule=None):
        self.flat = flat
        self.lr = lr
        self.momentum = momentum
        self.wd = weight_decay
        self.nesterov = nesterov
        self.lr_schedule = lr_schedule
        self.step_count = 0
        self.buf = torch.zeros(flat.numel, dtype=flat.grad.dtype, device=flat.device) if momentum else None

    @property
    def param_groups(self):
        return [{"lr": self.lr, "momentum": self.momentum, "weight_decay": self.wd}]

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        self.step_count += 1
        lr = self.lr_schedule(self.step_count) if self.lr_schedule else self.lr
        self.flat.finalize_fresh()
        p, g = self.flat.data, self.flat.step_grad
        if grad_scale != 1.0:
            g.mul_(grad_scale)
        if self.wd:
            # decay only the matrices/conv kernels (the flat layout puts them first)
            g[: self.flat.decay_end].add_(p[: self.flat.decay_end], alpha=self.wd)
        d = g
        if self.buf is not None:
            if self.step_count == 1:
                self.buf.copy_(g)
            else:
                self.buf.mul_(self.momentum).add_(g)
            d = g.add(self.buf, alpha=self.momentum) if self.nesterov else self.buf
        p.add_(d.to(p.dtype), alpha=-lr)

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    def state_dict(self):
        return {"step": self.step_count, "buf": self.buf, "lr": self.lr, "momentum": self.momentum, "wd": self.wd}

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        if self.buf is not None and sd.get("buf") is not None:
            self.buf.copy_(sd["buf"])
