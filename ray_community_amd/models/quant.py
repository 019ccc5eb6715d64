"""Quantised weights for inference: ``QuantLinear`` and ``quantize_weights_``.

``"fp8"``: a quantised linear holds its weight as OCP e4m3 bytes ``[out, in]`` plus one power-of-two
fp32 scale per output row (``ops.reference.quantize_weight_fp8_ref``), half the bytes of bf16, and runs
``ops.linear_w8``: the W8A16 skinny kernel up to ``ops.M_SKINNY`` rows, the mid-M kernel up to
``ops.M_MID`` (many live slots, a speculative verify round, a short prefill chunk; the same bits per row
as the skinny kernel, whatever the batch), dequantise + ``F.linear`` for longer prefill.
``"mxfp4"``: OCP microscaling FP4, two e2m1 nibbles a byte ``[out, in/2]`` plus one E8M0 scale byte per
32 inputs ``[out, in/32]`` (``ops.reference.quantize_weight_mxfp4_ref``), 4.25 bits a weight, through
``ops.linear_w4`` in the same way (``ops.M_SKINNY_W4``, ``ops.M_MID_W4``).
Activations stay bf16. Quantisation happens once, in torch, after the weights are loaded.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..ops import reference as ref
from .lora import LoraLinear

WEIGHT_FORMATS = ("fp8", "mxfp4")
WEIGHT_DTYPES = (None, "auto") + WEIGHT_FORMATS


class QuantLinear(nn.Module):
    """A bias-free linear over a quantised weight, ``weight_format`` ``"fp8"`` or ``"mxfp4"``.
    Buffers: ``qweight`` (the e4m3 bytes ``[out, in]`` or the e2m1 nibble pairs ``[out, in/2]``, stored
    as ``uint8`` so that ``Module.to(dtype)`` leaves them alone) and ``scale`` (fp8: fp32 ``[out]``,
    kept fp32 through ``.to(dtype)``, ``.half()`` and ``.bfloat16()``; mxfp4: E8M0 ``uint8
    [out, in/32]``). No ``weight``, no gradients."""

    def __init__(self, in_features: int, out_features: int, device=None, weight_format: str = "fp8"):
        super().__init__()
        if weight_format not in WEIGHT_FORMATS:
            raise ValueError(f"weight format must be one of {WEIGHT_FORMATS}, got {weight_format!r}")
        self.in_features, self.out_features, self.weight_format = int(in_features), int(out_features), weight_format
        if weight_format == "fp8":
            self.register_buffer("qweight", torch.zeros(out_features, in_features, dtype=torch.uint8, device=device))
            self.register_buffer("scale", torch.ones(out_features, dtype=torch.float32, device=device))
        else:
            if in_features % ref.MXFP4_BLOCK:
                raise ValueError(f"mxfp4 needs in_features % {ref.MXFP4_BLOCK} == 0, got {in_features}")
            self.register_buffer("qweight", torch.zeros(out_features, in_features // 2, dtype=torch.uint8, device=device))
            self.register_buffer("scale", torch.full((out_features, in_features // ref.MXFP4_BLOCK), 127,
                                                     dtype=torch.uint8, device=device))

    @classmethod
    def from_weight(cls, weight, fmt: str = "fp8"):
        """The quantised linear of a ``[out, in]`` weight (on the weight's device) in format ``fmt``."""
        m = cls(weight.shape[1], weight.shape[0], device="meta", weight_format=fmt)
        if fmt == "fp8":
            q, s = ref.quantize_weight_fp8_ref(weight.detach())
            m.qweight, m.scale = q.view(torch.uint8).contiguous(), s.contiguous()
        else:
            m.qweight, m.scale = ref.quantize_weight_mxfp4_ref(weight.detach())
        return m

    def _apply(self, fn, recurse=True):
        scale = self.scale
        super()._apply(fn, recurse)
        if self.scale.dtype != scale.dtype:  # a floating-point cast of the fp32 scales: move, do not convert
            self.scale = scale.to(self.scale.device)
        return self

    def dequantized(self, dtype=torch.bfloat16):
        """The weight this module multiplies by, exactly, in ``dtype`` (bf16 or fp32)."""
        if self.weight_format == "mxfp4":
            return ref.dequantize_mxfp4_ref(self.qweight, self.scale, dtype)
        return ref.kv_dequantize_fp8_ref(self.qweight.view(torch.float8_e4m3fn), self.scale, dtype)

    def forward(self, x):
        if torch.is_grad_enabled():
            raise RuntimeError(f"QuantLinear is inference-only ({self.weight_format} weights have no gradient): call "
                               "it under torch.no_grad() or torch.inference_mode()")
        if self.weight_format == "mxfp4":
            return ops.linear_w4(x, self.qweight, self.scale)
        return ops.linear_w8(x, self.qweight, self.scale)

    def extra_repr(self):
        kind = "fp8_e4m3" if self.weight_format == "fp8" else "mxfp4_e2m1"
        return f"in_features={self.in_features}, out_features={self.out_features}, weight={kind}"


def quantize_weights_(model, dtype="fp8"):
    """Replace the linears of a ``Llama`` (``qkv``, ``o``, ``gate_up``, ``down``, ``lm_head``) by
    ``QuantLinear``s made from their current weights in format ``dtype`` (``"fp8"`` or ``"mxfp4"``), in
    place, and free the originals. With tied embeddings ``embed.weight`` stays as it is for the lookup
    and ``lm_head`` becomes a quantised copy of it that ``Llama.logits`` reads. Norm weights and the
    embedding are not quantised. Idempotent for the same format; a model already quantised in the
    other format raises ``RuntimeError`` (its original weights are gone); ``None`` / ``"auto"`` leave
    the model alone; anything else raises ``ValueError``."""
    if dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight dtype must be one of {WEIGHT_DTYPES}, got {dtype!r}")
    if dtype not in WEIGHT_FORMATS:
        return model
    have = model.lm_head.weight_format if isinstance(model.lm_head, QuantLinear) else dtype
    if have != dtype:
        raise RuntimeError(f"the model's weights are already {have}: the originals are gone, so they cannot become {dtype}")
    with torch.no_grad():
        for blk in model.layers:
            for parent, name in ((blk.attn, "qkv"), (blk.attn, "o"), (blk.mlp, "gate_up"), (blk.mlp, "down")):
                lin = getattr(parent, name)
                if isinstance(lin, LoraLinear):  # LoRA enabled first: quantise the wrapped base
                    parent, name, lin = lin, "base", lin.base
                if not isinstance(lin, QuantLinear):
                    setattr(parent, name, QuantLinear.from_weight(lin.weight, dtype))
        if not isinstance(model.lm_head, QuantLinear):
            head = model.embed.weight if model.lm_head is None else model.lm_head.weight
            model.lm_head = QuantLinear.from_weight(head, dtype)
    model.weight_dtype = dtype
    return model


def weight_bytes(model) -> int:
    """Bytes of a module's parameters and buffers (shared tensors counted once)."""
    seen, total = set(), 0
    for t in list(model.parameters()) + list(model.buffers()):
        if id(t) not in seen:
            seen.add(id(t))
            total += t.numel() * t.element_size()
    return total
