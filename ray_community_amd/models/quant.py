"""FP8 weights for inference: ``QuantLinear`` and ``quantize_weights_``.

A quantised linear holds its weight as OCP e4m3 bytes ``[out, in]`` plus one power-of-two fp32
scale per output row (``ops.reference.quantize_weight_fp8_ref``), half the bytes of bf16, and runs
``ops.linear_w8``: the W8A16 kernel at decode batch sizes, dequantise + ``F.linear`` for prefill.
Activations stay bf16. Quantisation happens once, in torch, after the weights are loaded.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..ops import reference as ref
from .lora import LoraLinear

WEIGHT_DTYPES = (None, "auto", "fp8")


class QuantLinear(nn.Module):
    """A bias-free linear over an fp8 weight. Buffers: ``qweight`` (the e4m3 bytes, stored as
    ``uint8`` so that ``Module.to(dtype)`` leaves them alone) and ``scale`` (fp32, kept fp32 through
    ``.to(dtype)``, ``.half()`` and ``.bfloat16()``). No ``weight``, no gradients."""

    def __init__(self, in_features: int, out_features: int, device=None):
        super().__init__()
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.register_buffer("qweight", torch.zeros(out_features, in_features, dtype=torch.uint8, device=device))
        self.register_buffer("scale", torch.ones(out_features, dtype=torch.float32, device=device))

    @classmethod
    def from_weight(cls, weight):
        """The quantised linear of a ``[out, in]`` weight (on the weight's device)."""
        q, s = ref.quantize_weight_fp8_ref(weight.detach())
        m = cls(weight.shape[1], weight.shape[0], device="meta")
        m.qweight, m.scale = q.view(torch.uint8).contiguous(), s.contiguous()
        return m

    def _apply(self, fn, recurse=True):
        scale = self.scale
        super()._apply(fn, recurse)
        if self.scale.dtype != torch.float32:  # a floating-point cast: move, do not convert
            self.scale = scale.to(self.scale.device)
        return self

    def dequantized(self, dtype=torch.bfloat16):
        """The weight this module multiplies by, exactly, in ``dtype`` (bf16 or fp32)."""
        return ref.kv_dequantize_fp8_ref(self.qweight.view(torch.float8_e4m3fn), self.scale, dtype)

    def forward(self, x):
        if torch.is_grad_enabled():
            raise RuntimeError("QuantLinear is inference-only (fp8 weights have no gradient): call it under "
                               "torch.no_grad() or torch.inference_mode()")
        return ops.linear_w8(x, self.qweight, self.scale)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, weight=fp8_e4m3"


def quantize_weights_(model, dtype="fp8"):
    """Replace the linears of a ``Llama`` (``qkv``, ``o``, ``gate_up``, ``down``, ``lm_head``) by
    ``QuantLinear``s made from their current weights, in place, and free the originals. With tied
    embeddings ``embed.weight`` stays as it is for the lookup and ``lm_head`` becomes an fp8 copy of
    it that ``Llama.logits`` reads. Norm weights and the embedding are not quantised. Idempotent;
    ``None`` / ``"auto"`` leave the model alone; anything else raises ``ValueError``."""
    if dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight dtype must be one of {WEIGHT_DTYPES}, got {dtype!r}")
    if dtype != "fp8":
        return model
    with torch.no_grad():
        for blk in model.layers:
            for parent, name in ((blk.attn, "qkv"), (blk.attn, "o"), (blk.mlp, "gate_up"), (blk.mlp, "down")):
                lin = getattr(parent, name)
                if isinstance(lin, LoraLinear):  # LoRA enabled first: quantise the wrapped base
                    parent, name, lin = lin, "base", lin.base
                if not isinstance(lin, QuantLinear):
                    setattr(parent, name, QuantLinear.from_weight(lin.weight))
        if not isinstance(model.lm_head, QuantLinear):
            head = model.embed.weight if model.lm_head is None else model.lm_head.weight
            model.lm_head = QuantLinear.from_weight(head)
    model.weight_dtype = "fp8"
    return model


def weight_bytes(model) -> int:
    """Bytes of a module's parameters and buffers (shared tensors counted once)."""
    seen, total = set(), 0
    for t in list(model.parameters()) + list(model.buffers()):
        if id(t) not in seen:
            seen.add(id(t))
            total += t.numel() * t.element_size()
    return total
