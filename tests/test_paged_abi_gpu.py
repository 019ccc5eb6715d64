"""The C ABI of the four paged KV entry points (ops/csrc/paged_kv.h): ``rca_kv_cache_append``,
``rca_rope_kv_append_decode``, ``rca_attn_decode_paged`` and ``rca_attn_extend_paged``, called
directly through ``ops.lib()`` with the arguments named in the prototype's order.

(a) For both cache kinds a direct call on valid arguments gives bit for bit what the ``ops``
function gives on the same tensors. (b) Arguments the entry points document as refused come back
with the documented code (-1 shape, -2 grid limit, -3 pointer or alignment) and nothing is written:
every writable buffer is canary-filled and compared after a stream synchronise. A refused call
launches nothing, and every pointer passed here is valid or caught by the check under test.
"""
import functools

import pytest
import torch

from ray_community_amd import ops

pytestmark = pytest.mark.gpu

B, HQ, HK, D, PAGE, NUM_BLOCKS, MAX_BLOCKS = 2, 4, 2, 64, 16, 4, 2
LENS = (17, 1)  # two pages of a block table row, and a single token
W = (HQ + 2 * HK) * D
SCALE = D ** -0.5
KINDS = ("bf16", "fp8")
OPS = ("rca_kv_cache_append", "rca_rope_kv_append_decode", "rca_attn_decode_paged", "rca_attn_extend_paged")
ATTN = OPS[2:]


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def _empty_caches(kind):
    """k_cache, v_cache, k_scale, v_scale (scales ``None`` for the bf16 kind), zero-filled."""
    shape = (NUM_BLOCKS, PAGE, HK, D)
    if kind == "bf16":
        return [torch.zeros(shape, device="cuda", dtype=torch.bfloat16) for _ in range(2)] + [None, None]
    return ([torch.zeros(shape, device="cuda", dtype=torch.float8_e4m3fn) for _ in range(2)]
            + [torch.zeros(shape[:3], device="cuda") for _ in range(2)])


@functools.lru_cache(maxsize=None)
def _world(kind):
    """Shared, read-only inputs: caches filled through ``ops.kv_cache_append_``, tables, queries."""
    g = torch.Generator().manual_seed(11)
    caches = _empty_caches(kind)
    rows = torch.randn(NUM_BLOCKS * PAGE, W, generator=g).bfloat16().cuda()
    ops.kv_cache_append_(caches[0], caches[1], rows, _i32(list(range(NUM_BLOCKS * PAGE))), HQ, HK, D,
                         k_scale=caches[2], v_scale=caches[3])
    return dict(caches=caches, qkv=torch.randn(B, W, generator=g).bfloat16().cuda(),
                q_ext=torch.randn(4, HQ * D, generator=g).bfloat16().cuda(),
                cs=ops.rope_cos_sin(MAX_BLOCKS * PAGE, D).cuda(), table=_i32([[2, 0], [3, 1]]), lens=_i32(LENS),
                slots=_i32([5, 40]), cu=_i32([0, 3, 4]))  # extend: chunks of 3 and 1 tokens, T = 4


def _canary(*shape, dtype=torch.bfloat16):
    return torch.full(shape, 5.0, device="cuda", dtype=dtype)


def _args(op, kind, num_splits=1):
    """(arguments of ``op`` in the C prototype's order, stream left out; the buffers it may write).
    The append ops get canary caches of their own, the attention ops the shared filled ones."""
    w = _world(kind)
    if op in ATTN:
        kc, vc, ks, vs = w["caches"]
        T = B if op == "rca_attn_decode_paged" else 4
        out = _canary(T, HQ * D)
        part_o = _canary(T, HQ, num_splits, D, dtype=torch.float32) if num_splits > 1 else None
        part_ml = _canary(T, HQ, num_splits, 2, dtype=torch.float32) if num_splits > 1 else None
        writes = [out] + ([part_o, part_ml] if num_splits > 1 else [])
    else:
        kc, vc, ks, vs = _empty_caches(kind)
        qkv = w["qkv"].clone()
        writes = [t for t in (kc, vc, ks, vs) if t is not None]
    if op == "rca_kv_cache_append":
        a = dict(qkv=qkv, row_stride=W, slot_mapping=w["slots"], k_cache=kc, v_cache=vc, k_scale=ks, v_scale=vs, T=B,
                 Hq=HQ, Hk=HK, D=D, num_slots=NUM_BLOCKS * PAGE)
    elif op == "rca_rope_kv_append_decode":
        a = dict(qkv=qkv, row_stride=W, cs=w["cs"], max_pos=w["cs"].shape[0], block_table=w["table"],
                 context_lens=w["lens"], max_blocks=MAX_BLOCKS, k_cache=kc, v_cache=vc, k_scale=ks, v_scale=vs, B=B,
                 Hq=HQ, Hk=HK, D=D, page_size=PAGE, num_blocks=NUM_BLOCKS)
        writes.append(qkv)
    elif op == "rca_attn_decode_paged":
        a = dict(q=w["qkv"], q_stride=W, k_cache=kc, v_cache=vc, k_scale=ks, v_scale=vs, block_table=w["table"],
                 context_lens=w["lens"], out=out, part_o=part_o, part_ml=part_ml, B=B, Hq=HQ, Hk=HK, D=D,
                 page_size=PAGE, max_blocks=MAX_BLOCKS, num_blocks=NUM_BLOCKS, scale=SCALE, num_splits=num_splits)
    else:
        a = dict(q=w["q_ext"], q_stride=HQ * D, k_cache=kc, v_cache=vc, k_scale=ks, v_scale=vs,
                 block_table=w["table"], context_lens=w["lens"], cu_q_lens=w["cu"], out=out, part_o=part_o,
                 part_ml=part_ml, B=B, T=4, max_q_len=3, Hq=HQ, Hk=HK, D=D, page_size=PAGE, max_blocks=MAX_BLOCKS,
                 num_blocks=NUM_BLOCKS, scale=SCALE, num_splits=num_splits)
    return a, writes


def _call(op, a):
    vals = [0 if v is None else v.data_ptr() if isinstance(v, torch.Tensor) else v for v in a.values()]
    return getattr(ops.lib(), op)(*vals, ops.stream_ptr())


def _same(got, want):
    return all(torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8))
               for g, w in zip(got, want))


# ------------------------------------------------------------------ (a) direct call == ops call
@pytest.mark.parametrize("kind", KINDS)
def test_append_matches_ops(kind):
    a, writes = _args("rca_kv_cache_append", kind)
    assert _call("rca_kv_cache_append", a) == 0
    want = _empty_caches(kind)
    ops.kv_cache_append_(want[0], want[1], a["qkv"], a["slot_mapping"], HQ, HK, D, k_scale=want[2], v_scale=want[3])
    assert _same(writes, [t for t in want if t is not None])
    assert a["k_cache"].view(-1, HK * D)[5].float().abs().sum() > 0  # the call did write its slots


@pytest.mark.parametrize("kind", KINDS)
def test_rope_append_matches_ops(kind):
    a, writes = _args("rca_rope_kv_append_decode", kind)
    assert _call("rca_rope_kv_append_decode", a) == 0
    want = _empty_caches(kind)
    qkv = ops.rope_kv_append_decode_(_world(kind)["qkv"].clone(), a["cs"], want[0], want[1], a["block_table"],
                                     a["context_lens"], HQ, HK, D, k_scale=want[2], v_scale=want[3])
    assert _same(writes, [t for t in want if t is not None] + [qkv])
    assert not torch.equal(qkv, _world(kind)["qkv"])


@pytest.mark.parametrize("num_splits", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_decode_matches_ops(kind, num_splits):
    a, _ = _args("rca_attn_decode_paged", kind, num_splits)
    assert _call("rca_attn_decode_paged", a) == 0
    want = ops.paged_attention_decode(a["q"], a["k_cache"], a["v_cache"], a["block_table"], a["context_lens"], HQ, HK,
                                      D, num_splits=num_splits, k_scale=a["k_scale"], v_scale=a["v_scale"])
    assert _same([a["out"]], [want]) and not torch.equal(a["out"], _canary(B, HQ * D))


@pytest.mark.parametrize("num_splits", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_extend_matches_ops(kind, num_splits):
    a, _ = _args("rca_attn_extend_paged", kind, num_splits)
    assert _call("rca_attn_extend_paged", a) == 0
    want = ops.paged_attention_extend(a["q"], a["k_cache"], a["v_cache"], a["block_table"], a["context_lens"],
                                      a["cu_q_lens"], 3, HQ, HK, D, num_splits=num_splits, k_scale=a["k_scale"],
                                      v_scale=a["v_scale"])
    assert _same([a["out"]], [want]) and not torch.equal(a["out"], _canary(4, HQ * D))


# ------------------------------------------------------------------------- (b) refused calls
def _one_scale(a):
    a["k_scale"] = _world("fp8")["caches"][2]  # a real scale tensor, its partner missing


def _cache_off_by_8(a):
    a["k_cache"] = a["k_cache"].data_ptr() + 8  # inside the cache, and what the alignment check catches


def _fp8_cache_off_by_4(a):
    a["v_cache"] = a["v_cache"].data_ptr() + 4  # the e4m3 cache is read 8 B at a time


def _fp8_scale_off_by_2(a):
    a["v_scale"] = a["v_scale"].data_ptr() + 2


REFUSED = [(op, "bf16", "one scale", _one_scale, -3) for op in OPS]
REFUSED += [(op, "bf16", "cache + 8 B", _cache_off_by_8, -3) for op in OPS]
REFUSED += [(op, "fp8", "cache + 4 B", _fp8_cache_off_by_4, -3) for op in OPS]
REFUSED += [(op, "fp8", "scale + 2 B", _fp8_scale_off_by_2, -3) for op in OPS]
REFUSED += [(op, "fp8", "one scale", lambda a: a.update(v_scale=None), -3) for op in OPS]
REFUSED += [(op, "bf16", "no workspace", lambda a: a.update(num_splits=2), -3) for op in ATTN]
REFUSED += [(op, "bf16", "page 24", lambda a: a.update(page_size=24), -1) for op in OPS[1:]]
REFUSED += [(op, "bf16", "Hq % Hk", lambda a: a.update(Hq=3), -1) for op in OPS]
REFUSED += [(op, "bf16", "B = 65536", lambda a: a.update(B=65536), -2) for op in ATTN]


@pytest.mark.parametrize("op,kind,what,mutate,code", REFUSED, ids=[f"{r[0]}-{r[1]}-{r[2]}" for r in REFUSED])
def test_refused_call_writes_nothing(op, kind, what, mutate, code):
    a, writes = _args(op, kind)
    for t in writes:
        t.view(torch.uint8).fill_(0x5A)
    before = [t.clone() for t in writes]
    mutate(a)
    assert _call(op, a) == code, what
    torch.cuda.current_stream().synchronize()
    assert _same(writes, before), f"{what}: a refused call wrote"
