"""ctypes binding of the gfx950 kernel library.

On a machine with a visible AMD GPU the HIP path is mandatory: if the library is missing
and cannot be built, ``lib()`` raises instead of silently falling back to eager PyTorch.
"""
from __future__ import annotations

import ctypes
import os
import threading

from . import build as _build

_LOCK = threading.Lock()
_LIB = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_ll = ctypes.c_longlong
c_float = ctypes.c_float
_KV = [c_void_p, c_void_p, c_void_p, c_void_p]  # k_cache, v_cache, k_scale, v_scale of the paged KV ops (csrc/paged_kv.h)
_TAIL = [c_int, c_int, c_int, c_float, c_int, c_void_p]  # page_size, max_blocks, num_blocks, scale, num_splits, stream

_SIGS = {
    "rca_rmsnorm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "rca_rmsnorm_bwd_blocks": (c_int, [c_int, c_int]),
    "rca_rmsnorm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_int, c_int, c_int, c_void_p]),
    "rca_swiglu_fwd": (c_int, [c_void_p, c_void_p, c_ll, c_int, c_void_p]),
    "rca_swiglu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_void_p]),
    "rca_swiglu_fwd_tr": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rca_swiglu_bwd_tr": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rca_probe_hwid": (c_int, [c_void_p, c_void_p]),
    "rca_gemm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_ll, c_ll, c_ll, c_int, c_int, c_int,
                              c_void_p]),
    "rca_gemm_set_variant": (c_int, [c_int]),
    "rca_attn_set_dkdv_hs": (c_int, [c_int]),
    "rca_attn_set_fwd_mode": (c_int, [c_int]),
    "rca_gemm_swiglu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_ll, c_ll,
                                    c_void_p]),
    "rca_transpose_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_ll, c_void_p]),
    "rca_rope": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rca_rope_bwd_tr": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "rca_ce_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_ll, c_void_p]),
    "rca_ce_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_ll, c_int, c_ll, c_void_p]),
    "rca_ce_fused": (c_int, [c_void_p] * 5 + [c_ll, c_int, c_ll, c_void_p]),
    "rca_sumsq": (c_int, [c_void_p, c_ll, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "rca_adamw": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_ll, c_float, c_float, c_float,
                          c_float, c_float, c_float, c_float, c_float, c_void_p, c_float, c_void_p]),
    "rca_adamw_split_set_blocks": (None, [c_ll]),
    "rca_adamw_split": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_ll, c_float, c_float,
                                c_float, c_float, c_float, c_float, c_float, c_float, c_void_p, c_float, c_void_p]),
    "rca_adamw_split_seg": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_ll,
                                    c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_void_p,
                                    c_float, c_void_p]),
    "rca_gae": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                        c_float, c_float, c_int, c_void_p, c_void_p, c_float, c_void_p]),
    "rca_vtrace": (c_int, [c_void_p] * 8 + [c_int, c_int, c_float, c_float, c_float, c_float, c_void_p]),
    "rca_standardize": (c_int, [c_void_p, c_ll, c_void_p, c_void_p, c_float, c_void_p]),
    "rca_batched_copy": (c_int, [c_void_p, c_int, c_void_p, c_ll, c_void_p]),
    "rca_attn_fwd": (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_ll] * 4 + [c_float, c_int, c_void_p]),
    "rca_attn_bwd2": (c_int, [c_void_p] * 10 + [c_int] * 5 + [c_ll] * 8 + [c_float, c_int, c_void_p, c_ll, c_void_p]),
    "rca_attn_bwd_ws_bytes": (c_ll, [c_int] * 6),
    "rca_attn_set_bwd_mode": (c_int, [c_int]),
    "rca_attn_set_hs_nops": (c_int, [c_int]),
    "rca_crop_resize_normalize": (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rca_bn_workspace": (c_ll, [c_ll, c_int]),
    "rca_bn_fwd": (c_int, [c_void_p] * 9 + [c_ll, c_int, c_float, c_float, c_int, c_void_p]),
    "rca_bn_apply": (c_int, [c_void_p] * 4 + [c_ll, c_int, c_int, c_void_p]),
    "rca_bn_set_unroll": (c_int, [c_int]),
    "rca_attn_set_dq_qw": (c_int, [c_int]),
    "rca_attn_set_fwd_nw": (c_int, [c_int]),
    "rca_gemm_affine_act": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_ll] * 4 + [c_int, c_void_p]),
    "rca_bn_bwd": (c_int, [c_void_p] * 11 + [c_ll, c_int, c_int, c_void_p]),
    "rca_gbdt_hist_workspace": (c_ll, [c_int, c_ll, c_int, c_int]),
    "rca_gbdt_hist_exact_workspace": (c_ll, [c_int, c_ll, c_int, c_int]),
    "rca_gbdt_hist_exact": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_ll, c_int, c_int,
                                    c_void_p]),
    "rca_gbdt_hist": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_ll, c_int, c_int,
                              c_void_p]),
    "rca_image_normalize": (c_int, [c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                     c_void_p]),
    "rca_kv_cache_append": (c_int, [c_void_p, c_ll, c_void_p, *_KV,  # qkv, row_stride, slot_mapping
        c_ll, c_int, c_int, c_int, c_ll, c_void_p]),  # T, Hq, Hk, D, num_slots, stream
    "rca_rope_kv_append_decode": (c_int, [c_void_p, c_ll, c_void_p, c_int,  # qkv, row_stride, cs, max_pos
        c_void_p, c_void_p, c_int, *_KV,  # block_table, context_lens, max_blocks
        c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),  # B, Hq, Hk, D, page_size, num_blocks, stream
    "rca_attn_decode_paged": (c_int, [c_void_p, c_ll, *_KV,  # q, q_stride
        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,  # block_table, context_lens, out, part_o, part_ml
        c_int, c_int, c_int, c_int, *_TAIL]),  # B, Hq, Hk, D
    "rca_attn_extend_paged": (c_int, [c_void_p, c_ll, *_KV,  # q, q_stride
        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,  # block_table, context_lens, cu_q_lens, out, part_o, part_ml
        c_int, c_ll, c_int, c_int, c_int, c_int, *_TAIL]),  # B, T, max_q_len, Hq, Hk, D
    "rca_attn_decode_num_splits": (c_int, [c_int] * 4),
    "rca_attn_decode_fp8_set_step": (c_int, [c_int]),
    "rca_attn_extend_num_splits": (c_int, [c_int] * 6),
    "rca_sample_logits": (c_int, [c_void_p, c_ll, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rca_penalize_logits": (c_int, [c_void_p, c_ll, c_int] + [c_void_p] * 5 + [c_int, c_int, c_int, c_void_p]),
    "rca_token_logprobs": (c_int, [c_void_p, c_ll, c_int] + [c_void_p] * 4 + [c_int, c_int, c_int, c_void_p]),
    "rca_linear_w8_splits": (c_int, [c_int, c_int]),
    "rca_linear_w8a16": (c_int, [c_void_p] * 5 + [c_ll, c_int, c_int, c_int, c_ll, c_ll, c_void_p]),
    "rca_dequant_w8": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rca_lora_splits": (c_int, [c_int, c_int]),
    "rca_lora_add": (c_int, [c_void_p, c_ll, c_void_p, c_ll] + [c_void_p] * 5 + [c_int, c_void_p, c_ll] + [c_int] * 5
                     + [c_void_p]),
}


def lib():
    """Load (building if needed) the kernel library."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = os.environ.get("RCA_KERNEL_LIB") or _build.LIB_PATH  # override: A/B builds of the library
        if path == _build.LIB_PATH and (not os.path.exists(path) or (_build.is_stale() and
                                                                   os.environ.get("RCA_NO_REBUILD") != "1")):
            try:
                _build.build()
            except Exception as e:  # pragma: no cover - only on broken toolchains
                # never run kernels older than their sources: a stale library silently keeps old
                # launch/grid semantics while the tests appear to pass
                why = "missing" if not os.path.exists(path) else "stale (sources changed) and the rebuild failed"
                raise RuntimeError(f"ray_community_amd HIP kernel library {why}: {e}\n"
                                   "set RCA_NO_REBUILD=1 to load the existing library anyway") from e
        L = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
        return L


def check(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}")


def stream_ptr(device=None) -> int:
    import torch

    return torch.cuda.current_stream(device).cuda_stream
