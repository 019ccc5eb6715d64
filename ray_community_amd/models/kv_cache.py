"""Paged KV cache for Llama generation.

Per layer the cache is two tensors ``[num_blocks, page_size, Hk, D]``; a sequence owns a list of
blocks (in logical order) and token ``i`` of it lives in slot ``blocks[i // page_size] * page_size
+ i % page_size``. Every block id and slot handed to the kernels (``ops.kv_cache_append_``,
``ops.paged_attention_decode``, ``ops.paged_attention_extend``) comes from this allocator, which
is what keeps them in range. ``fork`` lets a new sequence share the whole leading pages of another
(a common prompt prefix): blocks carry a reference count and return to the free list when their
last owner lets go.
"""
from __future__ import annotations

from typing import Dict, Hashable, List, Optional, Sequence

import torch


class KVCacheFull(RuntimeError):
    """The paged KV cache has too few free blocks for the request (nothing was allocated)."""


def _is_fp8(kv_dtype) -> bool:
    """``kv_dtype`` as a flag: ``None`` / ``"auto"`` keep the model dtype, ``"fp8"`` /
    ``torch.float8_e4m3fn`` select the quantised cache."""
    if kv_dtype is None or kv_dtype == "auto":
        return False
    if kv_dtype == "fp8" or kv_dtype is torch.float8_e4m3fn:
        return True
    raise ValueError(f"kv_dtype must be None, 'auto', 'fp8' or torch.float8_e4m3fn, got {kv_dtype!r}")


class PagedKVCache:
    """``kv_dtype="fp8"`` stores K and V as ``float8_e4m3fn`` with one fp32 power-of-two scale per
    (token, kv head): ``k_scale`` / ``v_scale`` are per-layer lists of ``[num_blocks, page_size,
    Hk]`` tensors (``None`` for the unquantised cache). Scales live by slot, like the pages, so
    ``fork`` shares them with the pages they belong to."""

    def __init__(self, cfg, num_blocks: int, page_size: int = 16, device=None, dtype=torch.bfloat16, kv_dtype=None):
        if num_blocks <= 0 or page_size <= 0:
            raise ValueError("num_blocks and page_size must be positive")
        self.cfg = cfg
        self.num_blocks = int(num_blocks)
        self.page_size = int(page_size)
        self.device = torch.device(device if device is not None else "cpu")
        self.fp8 = _is_fp8(kv_dtype)
        self.dtype = torch.float8_e4m3fn if self.fp8 else dtype
        shape = (self.num_blocks, self.page_size, cfg.num_kv_heads, cfg.head_dim)
        # uninitialised on purpose: slots past a sequence's length are never read
        self.k = [torch.empty(shape, device=self.device, dtype=self.dtype) for _ in range(cfg.num_layers)]
        self.v = [torch.empty(shape, device=self.device, dtype=self.dtype) for _ in range(cfg.num_layers)]
        self.k_scale = self.v_scale = None
        if self.fp8:
            self.k_scale = [torch.empty(shape[:3], device=self.device, dtype=torch.float32)
                            for _ in range(cfg.num_layers)]
            self.v_scale = [torch.empty(shape[:3], device=self.device, dtype=torch.float32)
                            for _ in range(cfg.num_layers)]
        self._free: List[int] = list(range(self.num_blocks - 1, -1, -1))  # stack: block 0 goes first
        self._blocks: Dict[Hashable, List[int]] = {}
        self._lens: Dict[Hashable, int] = {}
        self._refs: List[int] = [0] * self.num_blocks  # owners per block (> 1 only after fork)

    @staticmethod
    def block_bytes(cfg, page_size: int, dtype=torch.bfloat16, kv_dtype=None) -> int:
        """Bytes one block takes over all layers, K and V, the fp8 cache's scales included."""
        rows = 2 * cfg.num_layers * int(page_size) * cfg.num_kv_heads  # head rows of a block
        if _is_fp8(kv_dtype):
            return rows * (cfg.head_dim + 4)
        return rows * cfg.head_dim * torch.empty((), dtype=dtype).element_size()

    @property
    def nbytes(self) -> int:
        """Bytes of the cache's tensors."""
        tensors = self.k + self.v + (self.k_scale or []) + (self.v_scale or [])
        return sum(t.numel() * t.element_size() for t in tensors)

    def scales(self, layer: int):
        """``(k_scale, v_scale)`` of a layer for the ``ops`` calls: ``(None, None)`` unless fp8."""
        return (self.k_scale[layer], self.v_scale[layer]) if self.fp8 else (None, None)

    @property
    def num_free_blocks(self) -> int:
        return len(self._free)

    def blocks_needed(self, seq_id, n_tokens: int) -> int:
        """Blocks ``allocate(seq_id, n_tokens)`` would take from the free list."""
        have = len(self._blocks.get(seq_id, ()))
        total = self._lens.get(seq_id, 0) + int(n_tokens)
        return max(0, -(-total // self.page_size) - have)

    def allocate(self, seq_id, n_tokens: int) -> List[int]:
        """Grow ``seq_id`` (created on first use) by ``n_tokens``; returns the new tokens' slots."""
        if n_tokens < 0:
            raise ValueError("n_tokens must be >= 0")
        need = self.blocks_needed(seq_id, n_tokens)
        if need > len(self._free):
            raise KVCacheFull(f"need {need} blocks for {n_tokens} more tokens of sequence {seq_id!r}, "
                              f"{len(self._free)} of {self.num_blocks} free")
        blocks = self._blocks.setdefault(seq_id, [])
        for _ in range(need):
            blk = self._free.pop()
            self._refs[blk] = 1
            blocks.append(blk)
        start = self._lens.get(seq_id, 0)
        self._lens[seq_id] = start + int(n_tokens)
        P = self.page_size
        return [blocks[i // P] * P + i % P for i in range(start, start + int(n_tokens))]

    def free(self, seq_id) -> None:
        """Give up the blocks of ``seq_id`` (unknown ids are ignored): each goes back to the free
        list unless a forked sequence still shares it."""
        for blk in reversed(self._blocks.pop(seq_id, [])):
            self._release(blk)
        self._lens.pop(seq_id, None)

    def _release(self, blk: int) -> None:
        self._refs[blk] -= 1
        if self._refs[blk] == 0:
            self._free.append(blk)

    def fork(self, parent_id, child_id, n_tokens: int) -> None:
        """Start ``child_id`` as a sequence of ``n_tokens`` tokens sharing the first
        ``n_tokens / page_size`` blocks of ``parent_id`` (no copy). ``n_tokens`` must be a multiple
        of ``page_size`` (a partly filled shared page would be written by two owners) and at most
        the parent's length, and ``child_id`` must be unused; otherwise ``ValueError`` and nothing
        changes. Either sequence may be freed or rolled back first."""
        n_tokens = int(n_tokens)
        if child_id in self._blocks or child_id in self._lens:
            raise ValueError(f"sequence {child_id!r} already exists")
        if parent_id not in self._lens:
            raise ValueError(f"unknown parent sequence {parent_id!r}")
        if n_tokens < 0 or n_tokens % self.page_size:
            raise ValueError(f"n_tokens must be a non-negative multiple of page_size {self.page_size}, got {n_tokens}")
        if n_tokens > self._lens[parent_id]:
            raise ValueError(f"cannot share {n_tokens} tokens of sequence {parent_id!r}, which holds "
                             f"{self._lens[parent_id]}")
        if n_tokens == 0:
            return  # nothing shared: the child is created by its first allocate
        shared = self._blocks[parent_id][: n_tokens // self.page_size]
        for blk in shared:
            self._refs[blk] += 1
        self._blocks[child_id] = list(shared)
        self._lens[child_id] = n_tokens

    def rollback(self, seq_id, n_tokens: int) -> None:
        """Undo the last ``n_tokens`` of ``seq_id``: blocks they alone occupied go back to the free
        list (in the order ``allocate`` would hand them out again) unless a forked sequence still
        shares them, and a sequence left with no tokens is forgotten."""
        have = self._lens.get(seq_id, 0)
        if n_tokens < 0 or n_tokens > have:
            raise ValueError(f"cannot roll back {n_tokens} of {have} tokens of sequence {seq_id!r}")
        left = have - int(n_tokens)
        blocks = self._blocks.get(seq_id, [])
        keep = -(-left // self.page_size)
        while len(blocks) > keep:
            self._release(blocks.pop())
        if left == 0:
            self._blocks.pop(seq_id, None)
            self._lens.pop(seq_id, None)
        else:
            self._lens[seq_id] = left

    def length(self, seq_id) -> int:
        return self._lens.get(seq_id, 0)

    def blocks_held(self, seq_id) -> int:
        return len(self._blocks.get(seq_id, ()))

    def block_table(self, seq_ids: Sequence[Optional[Hashable]]) -> torch.Tensor:
        """int32 ``[len(seq_ids), max_blocks]`` on the cache's device, rows padded with 0 (the
        kernels never read past a sequence's length). ``None`` / unknown ids give an empty row."""
        rows = [self._blocks.get(s, []) if s is not None else [] for s in seq_ids]
        width = max([len(r) for r in rows] + [1])
        table = [r + [0] * (width - len(r)) for r in rows]
        return torch.tensor(table, dtype=torch.int32).reshape(len(rows), width).to(self.device)

    def fill_decode_inputs(self, seq_ids: Sequence[Optional[Hashable]], context_lens, block_table) -> None:
        """``context_lens(seq_ids)`` and ``block_table(seq_ids)`` written into host arrays the caller
        owns (numpy ``[B]`` and ``[B, W]``, e.g. views of a pinned staging tensor) instead of new device
        tensors; ``W`` must hold the longest block list, and the rest of a row is zeroed."""
        for b, s in enumerate(seq_ids):
            blocks = self._blocks.get(s, ()) if s is not None else ()
            context_lens[b] = self._lens.get(s, 0) if s is not None else 0
            block_table[b, :len(blocks)] = blocks
            block_table[b, len(blocks):] = 0

    def context_lens(self, seq_ids: Sequence[Optional[Hashable]]) -> torch.Tensor:
        """int32 ``[len(seq_ids)]``: tokens held per sequence (0 for ``None`` / unknown ids)."""
        lens = [self._lens.get(s, 0) if s is not None else 0 for s in seq_ids]
        return torch.tensor(lens, dtype=torch.int32).to(self.device)
