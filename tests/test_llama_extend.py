"""Llama.extend (several new tokens per cached sequence), PagedKVCache.fork, chunked prefill and
shared prefixes in the generation engine: llama3-tiny in fp32 on the CPU (reference attention
path), plus bf16 twins on the GPU (the HIP extend kernel).

GPU bound: prefill (flash forward) and extend (paged extend kernel) are two bf16 kernels, so token
equality is not required. The yardstick is the max absolute logit error of the existing
``prefill`` against the fp32 reference-path model with the same weights and prompts; ``extend``,
whole and chunked, may have at most twice that (its only new error source is a second bf16
attention rounding of the same size). Both numbers are in profiles/extend_attention.md.
"""
import functools
import math

import pytest
import torch

from ray_community_amd.models import GenerationEngine, KVCacheFull, PagedKVCache, build_llama

gpu = pytest.mark.gpu
LENS = [1, 37, 128, 200]


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    return build_llama("llama3-tiny", dtype=torch.float32).eval()


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (n,), generator=g).tolist()


def _cache(m, blocks=64, page=16, device="cpu"):
    return PagedKVCache(m.cfg, blocks, page, device=device, dtype=m.embed.weight.dtype)


@functools.lru_cache(maxsize=None)
def _prompts():
    return [_prompt(n, 200 + n) for n in LENS]


@functools.lru_cache(maxsize=None)
def _prefill_logits():
    m = _model()
    cache = _cache(m)
    return m.prefill(_prompts(), None, cache, list(range(len(LENS))))


def _extend_chunked(m, prompts, cache, ids, chunk):
    """Feed the prompts ``chunk`` tokens per sequence per call; logits of each last prompt token."""
    out = [None] * len(prompts)
    for off in range(0, max(len(p) for p in prompts), chunk):
        idx = [b for b, p in enumerate(prompts) if off < len(p)]
        lg = m.extend([prompts[b][off: off + chunk] for b in idx], cache, [ids[b] for b in idx])
        for j, b in enumerate(idx):
            if off + chunk >= len(prompts[b]):
                out[b] = lg[j]
    return torch.stack(out)


# -------------------------------------------------------------------- extend vs prefill / decode
@pytest.mark.parametrize("chunk", [None, 7, 16, 33])
def test_extend_matches_prefill(chunk):
    m, prompts = _model(), _prompts()
    cache = _cache(m)
    ids = [("x", i) for i in range(len(prompts))]
    got = m.extend(prompts, cache, ids) if chunk is None else _extend_chunked(m, prompts, cache, ids, chunk)
    want = _prefill_logits()
    torch.testing.assert_close(got, want)
    assert got.argmax(-1).tolist() == want.argmax(-1).tolist()
    assert [cache.length(i) for i in ids] == LENS


def test_extend_after_decode_matches_from_scratch():
    m = _model()
    full = [_prompt(n + 3 + 5, 300 + n) for n in LENS]
    cache = _cache(m)
    ids = list(range(len(LENS)))
    m.extend([f[:n] for f, n in zip(full, LENS)], cache, ids)
    for s in range(3):
        m.decode_step([f[n + s] for f, n in zip(full, LENS)], cache, ids)
    got = m.extend([f[n + 3:] for f, n in zip(full, LENS)], cache, ids)
    want = m.extend(full, _cache(m), ids)  # the whole token list from scratch
    torch.testing.assert_close(got, want)
    assert got.argmax(-1).tolist() == want.argmax(-1).tolist()
    # and the greedy continuations from the two caches are identical
    other = _cache(m)
    m.extend(full, other, ids)
    tok = got.argmax(-1).tolist()
    for _ in range(4):
        a, b = m.decode_step(tok, cache, ids), m.decode_step(tok, other, ids)
        assert a.argmax(-1).tolist() == b.argmax(-1).tolist()
        tok = a.argmax(-1).tolist()


def test_extend_argument_checks():
    m = _model()
    cache = _cache(m)
    for tokens, ids in (([], []), ([[1], []], ["a", "b"]), ([[1]], ["a", "b"]), ([[1], [2]], ["a", "a"]),
                        ([[1] * 257], ["a"])):
        with pytest.raises(ValueError):
            m.extend(tokens, cache, ids)
    assert cache.num_free_blocks == cache.num_blocks


def test_kv_cache_full_in_mid_batch_leaves_cache_unchanged():
    m = _model()
    cache = _cache(m, blocks=4)
    m.extend([_prompt(20, 1)], cache, ["a"])  # 2 blocks
    free, la = cache.num_free_blocks, cache.length("a")
    with pytest.raises(KVCacheFull):  # "a" fits (1 more block), "b" fits (1), "c" does not
        m.extend([_prompt(20, 2), _prompt(10, 3), _prompt(5, 4)], cache, ["a", "b", "c"])
    assert cache.num_free_blocks == free == 2 and cache.length("a") == la == 20
    assert cache.length("b") == 0 and cache.blocks_held("b") == 0 and cache.blocks_held("c") == 0
    assert cache.blocks_held("a") == 2
    # the free list is in its old order: the next allocation gets the blocks it would have got
    assert [s // 16 for s in cache.allocate("d", 32)][::16] == [2, 3]


# ------------------------------------------------------------------------------------- fork
def test_fork_shares_blocks_and_counts_references():
    m = _model()
    cache = _cache(m, blocks=8)
    cache.allocate("p", 40)  # blocks 0, 1, 2
    cache.fork("p", "c", 32)
    tp, tc = cache.block_table(["p"])[0].tolist(), cache.block_table(["c"])[0].tolist()
    assert tc == tp[:2] and cache.length("c") == 32 and cache.blocks_held("c") == 2
    assert cache.num_free_blocks == 5
    assert cache.blocks_needed("c", 1) == 1 and cache.blocks_needed("c", 0) == 0
    new = cache.allocate("c", 3)
    assert all(s // 16 not in tp for s in new)  # the child writes its own page, never a shared one
    assert cache.num_free_blocks == 4
    cache.free("p")  # shared blocks stay; only the parent's own third block returns
    assert cache.num_free_blocks == 5 and cache.block_table(["c"])[0].tolist()[:2] == tp[:2]
    cache.rollback("c", 3 + 16)  # into the shared region: its own block returns, a shared one is dropped
    assert cache.num_free_blocks == 7 and cache.length("c") == 16
    cache.free("c")
    assert cache.num_free_blocks == 8
    # rollback into the shared region while the parent lives: decrement, no free
    cache.allocate("p", 32)
    cache.fork("p", "c", 32)
    cache.rollback("c", 16)
    assert cache.num_free_blocks == 6 and cache.blocks_held("c") == 1 and cache.blocks_held("p") == 2
    cache.free("c")
    assert cache.num_free_blocks == 6
    cache.free("p")
    assert cache.num_free_blocks == 8


def test_fork_misuse_raises_and_changes_nothing():
    m = _model()
    cache = _cache(m, blocks=8)
    cache.allocate("p", 40)
    cache.allocate("q", 5)
    for parent, child, n in (("p", "c", 20), ("p", "c", 48), ("p", "q", 16), ("nobody", "c", 16), ("p", "c", -16),
                             ("p", "p", 16)):
        with pytest.raises(ValueError):
            cache.fork(parent, child, n)
        assert cache.num_free_blocks == 4 and cache.length("c") == 0 and cache.blocks_held("c") == 0
        assert cache.length("p") == 40 and cache.length("q") == 5
    cache.free("p")
    cache.free("q")
    assert cache.num_free_blocks == 8


def test_fork_child_reads_survive_parent_free():
    m = _model()
    prefix, suffix = _prompt(32, 11), _prompt(9, 12)
    cache = _cache(m)
    m.extend([prefix], cache, ["p"])
    cache.fork("p", "c", 32)
    cache.free("p")
    got = m.extend([suffix], cache, ["c"])
    want = m.extend([prefix + suffix], _cache(m), ["w"])
    torch.testing.assert_close(got, want)
    cache.free("c")
    assert cache.num_free_blocks == cache.num_blocks


# ---------------------------------------------------------------------------------- generate
def test_generate_prefill_chunk_equals_generate():
    m = _model()
    prompts = [_prompt(5, 1), _prompt(17, 2), _prompt(130, 3)]
    assert m.generate(prompts, 10, prefill_chunk=16) == m.generate(prompts, 10)
    with pytest.raises(ValueError):
        m.generate(prompts, 10, prefill_chunk=0)


# ------------------------------------------------------------------------------------ engine
def _drain(engine, out=None, max_steps=400):
    out = {} if out is None else out
    for _ in range(max_steps):
        if not engine.has_work():
            return out
        for rid, tok, _ in engine.step():
            out.setdefault(rid, []).append(tok)
    raise AssertionError("engine did not drain")


def _blocks_of(engine):
    """Distinct cache blocks held by the engine's active requests."""
    c = engine.cache
    return {b for r in engine.slots if r is not None
            for b in c.block_table([r.seq_id])[0].tolist()[: c.blocks_held(r.seq_id)]}


def _two_requests(chunk):
    """A decodes; B (150 tokens) arrives after 3 steps. Returns (outputs, steps B needed, tokens A
    produced in each of those steps, engine)."""
    m = _model()
    eng = GenerationEngine(m, max_slots=4, num_blocks=64, page_size=16, prefill_chunk=chunk)
    a = eng.add_request(_prompt(9, 21), 30)
    out = {}
    for _ in range(3):
        for rid, tok, _ in eng.step():
            out.setdefault(rid, []).append(tok)
    b = eng.add_request(_prompt(150, 22), 6)
    steps, a_per_step = 0, []
    while b not in out:
        ev = eng.step()
        steps += 1
        a_per_step.append(sum(1 for rid, _, _ in ev if rid == a))
        for rid, tok, _ in ev:
            out.setdefault(rid, []).append(tok)
    _drain(eng, out)
    return (out[a], out[b]), steps, a_per_step, eng


def test_engine_chunked_prefill_keeps_decoding():
    (a0, b0), steps0, _, eng0 = _two_requests(None)
    (a1, b1), steps1, a_per_step, eng1 = _two_requests(16)
    assert steps0 == 1
    assert steps1 == math.ceil(150 / 16)  # the admitting step and ceil(150/16) - 1 further steps
    assert a_per_step == [1] * steps1     # A produced a token in every step while B prefilled
    assert (a1, b1) == (a0, b0) and len(a0) == 30 and len(b0) == 6
    assert eng1.prefill_chunk == 16 and eng1.num_prefilling == 0
    for eng in (eng0, eng1):
        assert eng.cache.num_free_blocks == eng.cache.num_blocks


def test_engine_chunk_budget_is_shared_in_arrival_order():
    m = _model()
    eng = GenerationEngine(m, max_slots=4, num_blocks=64, page_size=16, prefill_chunk=16)
    a, b = eng.add_request(_prompt(24, 31), 2), eng.add_request(_prompt(24, 32), 2)
    assert eng.step() == [] and eng.num_prefilling == 2          # 16 of A
    assert eng.cache.length(eng.slots[0].seq_id) == 16 and eng.cache.length(eng.slots[1].seq_id) == 0
    ev = eng.step()                                              # 8 of A (first token), 8 of B
    assert [rid for rid, _, _ in ev] == [a] and eng.cache.length(eng.slots[1].seq_id) == 8
    ev = eng.step()                                              # 16 of B (first token); A decodes
    assert sorted(rid for rid, _, _ in ev) == [a, b]
    ref = GenerationEngine(m, max_slots=4, num_blocks=64, page_size=16)
    ra, rb = ref.add_request(_prompt(24, 31), 2), ref.add_request(_prompt(24, 32), 2)
    want = _drain(ref)
    got = {a: [t for rid, t, _ in ev if rid == a], b: [t for rid, t, _ in ev if rid == b]}
    for rid, tok, _ in eng.step():
        got[rid].append(tok)
    assert got[b] == want[rb] and want[ra][1] == got[a][0]
    assert eng.cache.num_free_blocks == eng.cache.num_blocks


def test_engine_cancel_during_prefill_frees_blocks():
    m = _model()
    eng = GenerationEngine(m, max_slots=2, num_blocks=32, page_size=16, prefill_chunk=16)
    b = eng.add_request(_prompt(150, 22), 4)
    eng.step()
    eng.step()
    assert eng.num_prefilling == 1 and eng.cache.num_free_blocks == 30
    assert eng.cancel(b) and eng.num_prefilling == 0 and eng.num_active == 0
    assert eng.cache.num_free_blocks == 32 and not eng.has_work()


def test_engine_failing_extend_requeues(monkeypatch):
    m = _model()
    eng = GenerationEngine(m, max_slots=2, num_blocks=32, page_size=16, prefill_chunk=16)
    b = eng.add_request(_prompt(40, 23), 3)
    eng.step()
    real, calls = m.extend, []

    def boom(*a, **k):
        calls.append(1)
        raise RuntimeError("boom")

    monkeypatch.setattr(m, "extend", boom)
    with pytest.raises(RuntimeError, match="boom"):
        eng.step()
    assert calls and eng.slots == [None, None] and [r.rid for r in eng.waiting] == [b]
    assert eng.cache.num_free_blocks == 32 and eng.num_prefilling == 0
    monkeypatch.setattr(m, "extend", real)
    ref = GenerationEngine(m, max_slots=2, num_blocks=32, page_size=16)
    rb = ref.add_request(_prompt(40, 23), 3)
    assert _drain(eng)[b] == _drain(ref)[rb]


@pytest.mark.parametrize("chunk", [None, 16])
def test_engine_shared_prefix(chunk):
    m = _model()
    prefix = _prompt(40, 41)
    suffixes = [_prompt(n, 50 + n) for n in (3, 11, 20)]
    plain = GenerationEngine(m, max_slots=4, num_blocks=64, page_size=16, prefill_chunk=chunk)
    ids = [plain.add_request(prefix + s, 8) for s in suffixes]
    held_plain, want = 0, {}
    while plain.has_work():
        for rid, tok, _ in plain.step():
            want.setdefault(rid, []).append(tok)
        held_plain = max(held_plain, plain.cache.num_blocks - plain.cache.num_free_blocks)

    eng = GenerationEngine(m, max_slots=4, num_blocks=64, page_size=16, prefill_chunk=chunk)
    h = eng.register_prefix(prefix)
    assert eng.cache.num_free_blocks == 64  # lazy: nothing cached yet
    rids = [eng.add_request(s, 8, prefix=h) for s in suffixes]
    held, got = 0, {}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            got.setdefault(rid, []).append(tok)
        held = max(held, len(_blocks_of(eng)))
    assert [got[r] for r in rids] == [want[i] for i in ids]
    # peak distinct blocks of the three requests: the 2 shared pages are held once instead of three times
    assert held == held_plain - 2 * 2
    assert eng.cache.num_free_blocks == 64 - 3  # the pinned prefix: 40 tokens, 3 blocks
    late = eng.add_request(suffixes[0], 8, prefix=h)  # the cached prefix is reused
    eng.release_prefix(h)  # the accepted request keeps it alive
    with pytest.raises(ValueError):
        eng.add_request(suffixes[0], 2, prefix=h)
    with pytest.raises(ValueError):
        eng.release_prefix(h)
    with pytest.raises(ValueError):
        eng.add_request(suffixes[0], 2, prefix=12345)
    assert _drain(eng)[late] == want[ids[0]]
    assert eng.cache.num_free_blocks == eng.cache.num_blocks


def test_engine_release_prefix_with_sharers_running():
    m = _model()
    eng = GenerationEngine(m, max_slots=2, num_blocks=16, page_size=16, prefill_chunk=None)
    h = eng.register_prefix(_prompt(40, 41))
    r = eng.add_request(_prompt(3, 53), 8, prefix=h)
    assert eng.step() == []  # the prefix
    out = {r: [tok for _, tok, _ in eng.step()]}  # forked, suffix fed, first token
    assert len(out[r]) == 1
    eng.release_prefix(h)
    assert eng.cache.num_free_blocks == 16 - 3  # the sharer holds the 2 shared pages and one of its own
    _drain(eng, out)
    assert len(out[r]) == 8 and eng.cache.num_free_blocks == 16


# --------------------------------------------------------------------------------- GPU twins
@gpu
def test_extend_bf16_error_within_twice_prefill_error():
    ref = _model()
    torch.manual_seed(0)
    dev = build_llama("llama3-tiny", device="cuda", dtype=torch.bfloat16).eval()
    dev.load_state_dict({k: v.to(torch.bfloat16) for k, v in ref.state_dict().items()})
    ref16 = build_llama("llama3-tiny", dtype=torch.float32).eval()  # the same (bf16-rounded) weights in fp32
    ref16.load_state_dict({k: v.float().cpu() for k, v in dev.state_dict().items()})
    prompts = _prompts()
    ids = list(range(len(prompts)))
    want = ref16.extend(prompts, _cache(ref16), ids)

    def err(logits):
        return (logits.float().cpu() - want).abs().max().item()

    yard = err(dev.prefill(prompts, None, _cache(dev, device="cuda"), ids))
    whole = err(dev.extend(prompts, _cache(dev, device="cuda"), ids))
    chunked = {c: err(_extend_chunked(dev, prompts, _cache(dev, device="cuda"), ids, c)) for c in (7, 16, 33)}
    print(f"max |logit err| vs fp32: prefill {yard:.4e}, extend {whole:.4e}, chunked {chunked}, "
          f"max |logit| {want.abs().max().item():.3e}")
    assert whole <= 2 * yard
    for c, e in chunked.items():
        assert e <= 2 * yard, (c, e, yard)


@gpu
def test_engine_chunked_and_prefix_on_gpu():
    torch.manual_seed(0)
    dev = build_llama("llama3-tiny", device="cuda", dtype=torch.bfloat16).eval()
    prefix, suffix = _prompt(40, 41), _prompt(11, 61)
    eng = GenerationEngine(dev, max_slots=4, num_blocks=64, page_size=16, prefill_chunk=16)
    h = eng.register_prefix(prefix)
    a = eng.add_request(_prompt(150, 22), 6)
    b = eng.add_request(suffix, 6, prefix=h)
    out = _drain(eng)
    assert len(out[a]) == 6 and len(out[b]) == 6
    assert all(0 <= t < 1024 for r in (a, b) for t in out[r])
    eng.release_prefix(h)
    assert eng.cache.num_free_blocks == eng.cache.num_blocks
