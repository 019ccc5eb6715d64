"""Multi-LoRA inference for ``Llama``: many low-rank adapters resident next to one set of base
weights, selected per request.

``LoraAdapter`` holds one adapter in the model's fused layout: per layer and per target linear
(``qkv``, ``o``, ``gate_up``, ``down``) a down-projection ``A [r_t, in]``, an up-projection
``B [out, r_t]`` and ``scale = alpha / rank``. ``Llama.enable_lora_`` wraps the four linears of every
block in ``LoraLinear``: the base module (plain or ``QuantLinear``) untouched, plus that target's bank
of ``max_adapters`` slots (``A [S, R, in]``, ``B [S, out, R]``, ``scale [S]`` fp32). A forward call names
an adapter (or ``None``) per row; ``LoraLinear`` runs the base and then ``ops.lora_add_`` on its result
(``ops/csrc/lora.hip``: two launches per target, whatever the number of adapters in the batch). Without
a named adapter nothing is launched and every logit keeps its bits.
"""
from __future__ import annotations

import contextlib
import re

import torch
import torch.nn as nn

from .. import ops

TARGETS = ("qkv", "o", "gate_up", "down")
# projections fused into each target, in the order of their output rows
PARTS = {"qkv": ("q", "k", "v"), "o": ("o",), "gate_up": ("gate", "up"), "down": ("down",)}
_PEFT = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
         "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}


class AdapterSlotsFull(RuntimeError):
    """``Llama.load_adapter``: every slot of the bank holds an adapter."""


def part_dims(cfg):
    """``{projection: (in, out)}`` of the unfused projections of one block."""
    H, I, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    q, kv = cfg.num_heads * D, cfg.num_kv_heads * D
    return {"q": (H, q), "k": (H, kv), "v": (H, kv), "o": (q, H), "gate": (H, I), "up": (H, I), "down": (I, H)}


def target_dims(cfg):
    """``{target: (in, out)}`` of the fused linears of one block."""
    dims = part_dims(cfg)
    return {t: (dims[PARTS[t][0]][0], sum(dims[p][1] for p in PARTS[t])) for t in TARGETS}


class LoraAdapter:
    """One adapter: ``layers[i][target] = (A [r_t, in], B [out, r_t], scale)``, fp32 on the CPU."""

    def __init__(self, layers):
        self.layers = [{t: (A.detach().float().cpu(), B.detach().float().cpu(), float(s)) for t, (A, B, s) in lay.items()}
                       for lay in layers]

    @classmethod
    def random(cls, cfg, rank: int, seed: int = 0, alpha=None):
        """A seeded adapter of ``rank`` per projection (``qkv`` has rank ``3 * rank``, ``gate_up``
        ``2 * rank``), dense in the fused layout; ``alpha`` defaults to ``2 * rank``."""
        g = torch.Generator().manual_seed(int(seed))
        scale = float(2 * rank if alpha is None else alpha) / rank
        layers = []
        for _ in range(cfg.num_layers):
            lay = {}
            for t, (n_in, n_out) in target_dims(cfg).items():
                r = rank * len(PARTS[t])
                lay[t] = (torch.randn(r, n_in, generator=g) / n_in ** 0.5, torch.randn(n_out, r, generator=g) * 0.02, scale)
            layers.append(lay)
        return cls(layers)

    @classmethod
    def from_peft_state_dict(cls, sd, cfg, alpha):
        """From per-projection tensors ``layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight`` and
        ``layers.{i}.mlp.{gate,up,down}_proj.lora_{A,B}.weight`` (with or without a
        ``base_model.model.model.`` prefix). The ``A``s of a fused target are stacked along the rank
        axis and the ``B``s placed block-diagonally, so ``qkv`` has rank ``3r`` and ``gate_up``
        ``2r``; a missing projection contributes zeros. ``scale = alpha / r``."""
        found = {}
        for key, w in sd.items():
            m = re.search(r"(?:^|\.)layers\.(\d+)\.((?:self_attn|mlp)\.\w+_proj)\.lora_([AB])\.weight$", key)
            if m is None:
                raise ValueError(f"unexpected adapter tensor {key!r}")
            found[(int(m.group(1)), m.group(2), m.group(3))] = w.detach().float().cpu()
        ranks = {w.shape[0] for (_, _, ab), w in found.items() if ab == "A"}
        if len(ranks) != 1:
            raise ValueError(f"the projections of an adapter must share one rank, got {sorted(ranks)}")
        r = ranks.pop()
        if any(i >= cfg.num_layers for i, _, _ in found):
            raise ValueError(f"adapter names a layer beyond the model's {cfg.num_layers}")
        dims, layers = part_dims(cfg), []
        for i in range(cfg.num_layers):
            lay = {}
            for t, (n_in, n_out) in target_dims(cfg).items():
                A = torch.zeros(r * len(PARTS[t]), n_in)
                B = torch.zeros(n_out, r * len(PARTS[t]))
                row = 0
                for j, p in enumerate(PARTS[t]):
                    a, b = found.get((i, _PEFT[p], "A")), found.get((i, _PEFT[p], "B"))
                    if (a is None) != (b is None):
                        raise ValueError(f"layer {i} {_PEFT[p]}: lora_A and lora_B come together")
                    if a is not None:
                        if tuple(a.shape) != (r, dims[p][0]) or tuple(b.shape) != (dims[p][1], r):
                            raise ValueError(f"layer {i} {_PEFT[p]}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} "
                                             f"do not fit [{r}, {dims[p][0]}] / [{dims[p][1]}, {r}]")
                        A[j * r: (j + 1) * r] = a
                        B[row: row + dims[p][1], j * r: (j + 1) * r] = b
                    row += dims[p][1]
                lay[t] = (A, B, float(alpha) / r)
            layers.append(lay)
        return cls(layers)

    def save(self, path):
        torch.save({"lora_adapter": self.layers}, path)

    @classmethod
    def load(cls, path):
        return cls(torch.load(path, map_location="cpu")["lora_adapter"])


class LoraBank:
    """What the ``LoraLinear``s of one model share: which slot holds which adapter, and the routing
    of the forward call in flight."""

    def __init__(self, max_adapters: int, max_rank: int):
        self.max_adapters, self.max_rank = int(max_adapters), int(max_rank)
        self.slots = {}       # name -> slot
        self.routing = None   # ops.LoraRouting while a call with adapters runs

    def capacity(self, target) -> int:
        return -(-len(PARTS[target]) * self.max_rank // 16) * 16

    @contextlib.contextmanager
    def route(self, names, device):
        """Route the rows of one forward call: ``names`` has an adapter name or ``None`` per row."""
        unknown = {n for n in names if n is not None and n not in self.slots}
        if unknown:
            raise ValueError(f"unknown adapter(s) {sorted(map(str, unknown))}: loaded are {sorted(self.slots)}")
        self.routing = ops.lora_routing([-1 if n is None else self.slots[n] for n in names], device)
        try:
            yield
        finally:
            self.routing = None


class LoraLinear(nn.Module):
    """A target linear with its bank: ``base`` (a bias-free linear or ``QuantLinear``) plus the
    buffers ``lora_A [S, R, in]``, ``lora_B [S, out, R]`` (the base's activation dtype) and
    ``lora_scale [S]`` (fp32 through every cast). Inference only."""

    def __init__(self, base, bank: LoraBank, target: str, dtype, device):
        super().__init__()
        self.base, self.bank, self.target = base, bank, target
        self.in_features, self.out_features = base.in_features, base.out_features
        S, R = bank.max_adapters, bank.capacity(target)
        self.register_buffer("lora_A", torch.zeros(S, R, self.in_features, dtype=dtype, device=device))
        self.register_buffer("lora_B", torch.zeros(S, self.out_features, R, dtype=dtype, device=device))
        self.register_buffer("lora_scale", torch.zeros(S, dtype=torch.float32, device=device))

    def _apply(self, fn, recurse=True):
        scale = self.lora_scale
        super()._apply(fn, recurse)
        if self.lora_scale.dtype != torch.float32:  # a floating-point cast: move, do not convert
            self.lora_scale = scale.to(self.lora_scale.device)
        return self

    def forward(self, x):
        if torch.is_grad_enabled():
            raise RuntimeError("LoraLinear is inference-only (adapters are not trained here): call it under "
                               "torch.no_grad() or torch.inference_mode()")
        y = self.base(x)
        routing = self.bank.routing
        if routing is not None and routing.any:
            ops.lora_add_(y.view(-1, self.out_features), x.reshape(-1, self.in_features), self.lora_A, self.lora_B,
                          self.lora_scale, routing)
        return y

    @torch.no_grad()
    def set_slot(self, slot, A=None, B=None, scale=0.0):
        """Fill ``slot`` (the unused rank stays zero), or clear it."""
        self.lora_A[slot].zero_()
        self.lora_B[slot].zero_()
        self.lora_scale[slot] = float(scale)
        if A is not None:
            r = A.shape[0]
            self.lora_A[slot, :r].copy_(A)
            self.lora_B[slot, :, :r].copy_(B)

    def extra_repr(self):
        return f"target={self.target}, slots={self.bank.max_adapters}, capacity={self.bank.capacity(self.target)}"


def _targets(model):
    for blk in model.layers:
        yield blk.attn, "qkv"
        yield blk.attn, "o"
        yield blk.mlp, "gate_up"
        yield blk.mlp, "down"


def enable_lora_(model, max_adapters: int, max_rank: int):
    """Wrap the four linears of every block of a ``Llama`` in ``LoraLinear`` with room for
    ``max_adapters`` adapters of up to ``max_rank`` per projection (slot capacity per target:
    ``parts * max_rank`` rounded up to a multiple of 16). The model is inference-only afterwards."""
    if getattr(model, "lora", None) is not None:
        raise ValueError("LoRA is already enabled on this model")
    if int(max_adapters) < 1 or int(max_rank) < 1:
        raise ValueError("enable_lora_ needs max_adapters >= 1 and max_rank >= 1")
    bank = LoraBank(max_adapters, max_rank)
    w = model.embed.weight
    for parent, name in _targets(model):
        setattr(parent, name, LoraLinear(getattr(parent, name), bank, name, w.dtype, w.device))
    model.lora = bank
    return model


def _bank(model) -> LoraBank:
    bank = getattr(model, "lora", None)
    if bank is None:
        raise ValueError("LoRA is not enabled on this model: call enable_lora_(max_adapters, max_rank) first")
    return bank


def load_adapter(model, name, adapter: LoraAdapter):
    """Copy ``adapter`` into a free slot under ``name``; returns the slot."""
    bank = _bank(model)
    if name is None or name in bank.slots:
        raise ValueError(f"adapter name {name!r} is empty or already loaded")
    dims = target_dims(model.cfg)
    if len(adapter.layers) != len(model.layers):
        raise ValueError(f"adapter has {len(adapter.layers)} layers, the model {len(model.layers)}")
    for lay in adapter.layers:
        for t in TARGETS:
            A, B, _ = lay[t]
            r = A.shape[0]
            if r > len(PARTS[t]) * bank.max_rank:
                raise ValueError(f"adapter rank {r} of {t} exceeds {len(PARTS[t])} x max_rank {bank.max_rank}")
            if tuple(A.shape) != (r, dims[t][0]) or tuple(B.shape) != (dims[t][1], r):
                raise ValueError(f"adapter {t}: A {tuple(A.shape)} / B {tuple(B.shape)} do not fit a "
                                 f"[{dims[t][1]}, {dims[t][0]}] linear")
    free = sorted(set(range(bank.max_adapters)) - set(bank.slots.values()))
    if not free:
        raise AdapterSlotsFull(f"all {bank.max_adapters} adapter slots are in use: {sorted(bank.slots)}")
    slot = free[0]
    for (parent, t), lay in zip(_targets(model), (lay for lay in adapter.layers for _ in TARGETS)):
        getattr(parent, t).set_slot(slot, *lay[t])
    bank.slots[name] = slot
    return slot


def unload_adapter(model, name):
    bank = _bank(model)
    if name not in bank.slots:
        raise ValueError(f"unknown adapter {name!r}: loaded are {sorted(bank.slots)}")
    slot = bank.slots.pop(name)
    for parent, t in _targets(model):
        getattr(parent, t).set_slot(slot)


def bank_bytes(model) -> int:
    """Bytes of the adapter banks of a LoRA-enabled model."""
    return sum(b.numel() * b.element_size() for m in model.modules() if isinstance(m, LoraLinear)
               for b in (m.lora_A, m.lora_B, m.lora_scale))


def route(model, names, device):
    """The context of one forward call whose row ``m`` takes adapter ``names[m]`` (``None``: base).
    With no adapter named, on any model, nothing is set up."""
    if names is None or all(n is None for n in names):
        return contextlib.nullcontext()
    return _bank(model).route(names, device)
