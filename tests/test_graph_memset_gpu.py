"""ops.graph_memsets_to_kernels (csrc/graph_memset.hip): the memset nodes of a captured HIP graph
become fill-kernel nodes that store the same bytes at the same place in the graph. Checked against
the bytes the memsets define (numpy), guard bytes around every range included, over several
replays: 1-, 2- and 4-byte patterns, unaligned heads and tails, ranges inside one 16-byte line,
a range of many blocks, and a pitched 2-D memset."""
import ctypes

import numpy as np
import pytest
import torch

from ray_community_amd import ops

pytestmark = pytest.mark.gpu

REGION = 128 << 10
GUARD = 0xAA
# (byte offset in its region, element bytes, value, width in elements, height, pitch in bytes)
CASES = [
    (0, 1, 0x5A, 1, 1, 0),             # one byte
    (5, 1, 0x22, 9, 1, 0),             # inside one 16-byte line: head only
    (3, 1, 0x11, 37, 1, 0),            # head, one aligned vector, tail
    (16, 1, 0x00, 4096, 1, 0),         # aligned, whole vectors only
    (2, 2, 0xBEEF, 301, 1, 0),         # 16-bit pattern, middle at phase 2
    (4, 4, 0xDEADBEEF, 1027, 1, 0),    # 32-bit pattern, middle at phase 0
    (12, 4, 0x01020304, 1, 1, 0),      # one 32-bit word (a reduction's semaphore)
    (65, 1, 0x33, 100_001, 1, 0),      # more than one block of vectors
    (7, 1, 0x44, 21, 5, 48),           # 2-D: 5 rows of 21 bytes, 48 bytes apart
]


def _expected():
    a = np.full(len(CASES) * REGION, GUARD, np.uint8)
    for i, (off, es, value, width, height, pitch) in enumerate(CASES):
        pat = np.frombuffer(int(value).to_bytes(4, "little")[:es], np.uint8)
        for r in range(height):
            s = i * REGION + off + r * pitch
            a[s: s + width * es] = np.tile(pat, width)
    return a


def test_memset_nodes_become_fill_kernels():
    from ray_community_amd._private.gpu_store import _check, _hip

    hip = _hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipMemsetAsync.argtypes = [vp, ctypes.c_int, sz, vp]
    hip.hipMemsetD16Async.argtypes = [vp, ctypes.c_ushort, sz, vp]
    hip.hipMemsetD32Async.argtypes = [vp, ctypes.c_int, sz, vp]
    hip.hipMemset2DAsync.argtypes = [vp, sz, ctypes.c_int, sz, sz, vp]
    buf = torch.zeros(len(CASES) * REGION, dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(buf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):  # fill kernel -> the memsets -> copy kernel
        buf.fill_(GUARD)
        s = torch.cuda.current_stream().cuda_stream
        for i, (off, es, value, width, height, pitch) in enumerate(CASES):
            p = buf.data_ptr() + i * REGION + off
            if height > 1:
                _check(hip.hipMemset2DAsync(p, pitch, value, width, height, s), "hipMemset2DAsync")
            elif es == 1:
                _check(hip.hipMemsetAsync(p, value, width, s), "hipMemsetAsync")
            elif es == 2:
                _check(hip.hipMemsetD16Async(p, value, width, s), "hipMemsetD16Async")
            else:
                _check(hip.hipMemsetD32Async(p, ctypes.c_int32(value).value, width, s), "hipMemsetD32Async")
        out.copy_(buf)
    assert ops.graph_memsets_to_kernels(graph) >= len(CASES)
    assert ops.graph_memsets_to_kernels(graph) == 0  # none left
    graph.instantiate()
    want = _expected()
    for replay in range(3):
        buf.zero_()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, t in (("buf", buf), ("out", out)):  # out: the fill kernels keep the memsets' dependents
            got = t.cpu().numpy()
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (replay, name, bad[:8], got[bad[:8]], want[bad[:8]])
