"""Llama generation over the paged KV cache: prefill / decode_step / generate, the cache allocator
and the continuous-batching engine (CPU, llama3-tiny in fp32), plus the bf16 HIP path on a GPU."""
import functools

import pytest
import torch

from ray_community_amd.models import GenerationEngine, KVCacheFull, PagedKVCache, build_llama

MARGIN = 1e-3
LENS = [5, 128, 130]
N_DECODE = 8


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    return build_llama("llama3-tiny", dtype=torch.float32).eval()


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (n,), generator=g).tolist()


@functools.lru_cache(maxsize=None)
def _naive(prompt, n):
    """No-cache greedy loop (full forward per token) -> (tokens, steps safe to compare): the
    comparison stops at the first step whose top-2 logit margin is below MARGIN."""
    m = _model()
    toks, out, safe = list(prompt), [], None
    with torch.no_grad():
        for step in range(n):
            logits = m(torch.tensor([toks]))[0, -1]
            top = logits.topk(2).values
            if safe is None and (top[0] - top[1]).item() < MARGIN:
                safe = step
            out.append(int(logits.argmax()))
            toks.append(out[-1])
    return out, n if safe is None else safe


def _assert_matches_naive(cases, got):
    """cases: [(prompt tuple, n)]; got: generated token lists. >= 3/4 of all steps must be compared."""
    compared = total = 0
    for (prompt, n), toks in zip(cases, got):
        want, safe = _naive(prompt, n)
        assert len(toks) == n
        assert toks[:safe] == want[:safe]
        compared += safe
        total += n
    assert compared * 4 >= total * 3, f"only {compared} of {total} steps had a top-2 margin >= {MARGIN}"


def _teacher_forced(model, ref_model, device):
    """prefill + N_DECODE decode_steps fed the true next tokens -> (cached logits, reference
    full-forward logits, the model's own full-forward logits), each [len(LENS) * (1 + N_DECODE), V]."""
    full = [_prompt(n + N_DECODE, 100 + n) for n in LENS]
    cache = PagedKVCache(model.cfg, 48, 16, device=device, dtype=model.embed.weight.dtype)
    ids = list(range(len(LENS)))
    cached = [model.prefill([f[:n] for f, n in zip(full, LENS)], None, cache, ids)]
    for s in range(N_DECODE):
        cached.append(model.decode_step([f[n + s] for f, n in zip(full, LENS)], cache, ids))
    cached = torch.stack(cached, 1).float().cpu()  # [B, 1 + N, V]
    want, own = [], []
    with torch.no_grad():
        for f, n in zip(full, LENS):
            S = -(-len(f) // 128) * 128  # right padding: invisible to real tokens under the causal mask
            t = torch.zeros(1, S, dtype=torch.long)
            t[0, : len(f)] = torch.tensor(f)
            want.append(ref_model(t)[0, n - 1: n + N_DECODE].float())
            own.append(model(t.to(device))[0, n - 1: n + N_DECODE].float().cpu())
    for i in ids:
        cache.free(i)
    assert cache.num_free_blocks == cache.num_blocks
    return cached, torch.stack(want), torch.stack(own)


def test_cached_logits_match_full_forward():
    m = _model()
    cached, want, _ = _teacher_forced(m, m, "cpu")
    err, scale = (cached - want).abs().max().item(), want.abs().max().item()
    print(f"max |cached - full| = {err:.3e}, max |logit| = {scale:.3e}")
    assert err <= 1e-4 * scale


def test_greedy_generate_matches_naive_loop():
    m = _model()
    cases = [(tuple(_prompt(5, 1)), 12), (tuple(_prompt(17, 2)), 12), (tuple(_prompt(130, 3)), 12)]
    got = m.generate([list(p) for p, _ in cases], 12)
    _assert_matches_naive(cases, got)


def test_generate_sampling_is_seeded_and_stops_at_eos():
    m = _model()
    p = [_prompt(7, 4), _prompt(9, 5)]
    a = m.generate(p, 10, temperature=0.8, top_k=20, seed=3)
    assert a == m.generate(p, 10, temperature=0.8, top_k=20, seed=3)
    assert a != m.generate(p, 10, temperature=0.8, top_k=20, seed=4)
    greedy = m.generate(p, 10)
    eos = greedy[0][3]
    cut = m.generate(p, 10, eos_token_id=eos)
    k = greedy[0].index(eos)
    assert cut[0] == greedy[0][: k + 1]  # EOS is emitted, then the sequence stops
    if eos not in greedy[1]:
        assert cut[1] == greedy[1]  # its neighbour runs on


def test_cache_accounting():
    m = _model()
    cache = PagedKVCache(m.cfg, 4, 16, dtype=torch.float32)
    m.generate([_prompt(5, 1), _prompt(20, 2)], 6, cache=cache)
    assert cache.num_free_blocks == 4  # generate frees its blocks
    slots = cache.allocate("a", 33)  # 3 blocks
    assert len(slots) == 33 and len(set(slots)) == 33 and cache.num_free_blocks == 1
    assert all(0 <= s < 4 * 16 for s in slots)
    with pytest.raises(KVCacheFull):
        cache.allocate("b", 17)  # needs 2
    assert cache.num_free_blocks == 1 and cache.length("b") == 0 and cache.blocks_held("b") == 0
    with pytest.raises(KVCacheFull):
        cache.allocate("a", 32)  # growing "a" past the cache fails too, and leaves "a" as it was
    assert cache.length("a") == 33 and cache.num_free_blocks == 1
    assert cache.allocate("a", 15) == [slots[32] + 1 + i for i in range(15)]  # fills its last page
    held = {s // 16 for s in slots}
    cache.free("a")
    assert cache.num_free_blocks == 4
    again = cache.allocate("c", 48)
    assert {s // 16 for s in again} == held  # freed blocks are reused
    bt, cl = cache.block_table(["c", None]), cache.context_lens(["c", None])
    assert bt.dtype == torch.int32 and cl.dtype == torch.int32
    assert bt.shape == (2, 3) and bt[1].tolist() == [0, 0, 0] and cl.tolist() == [48, 0]
    with pytest.raises(KVCacheFull):  # over-committed generate: nothing stays allocated
        m.generate([_prompt(5, 1), _prompt(40, 2)], 4, cache=cache)
    assert cache.num_free_blocks == 1
    cache.free("c")
    assert cache.num_free_blocks == 4


def _drain(engine, max_steps=200):
    out, fin = {}, {}
    for _ in range(max_steps):
        if not engine.has_work():
            break
        for rid, tok, done in engine.step():
            assert not fin.get(rid), "token after finish"
            out.setdefault(rid, []).append(tok)
            fin[rid] = done
    assert not engine.has_work()
    return out, fin


def test_engine_request_admitted_mid_decode_matches_alone():
    m = _model()
    cases = [(tuple(_prompt(6, 11)), 14), (tuple(_prompt(21, 12)), 10), (tuple(_prompt(9, 13)), 8)]
    eng = GenerationEngine(m, max_slots=4, num_blocks=32)
    r0 = eng.add_request(list(cases[0][0]), 14)
    r1 = eng.add_request(list(cases[1][0]), 10)
    out = {}
    for _ in range(3):  # the first two are mid-decode ...
        for rid, tok, _done in eng.step():
            out.setdefault(rid, []).append(tok)
    assert eng.num_active == 2 and 1 < len(out[r0]) < 14
    r2 = eng.add_request(list(cases[2][0]), 8)  # ... when the third arrives
    rest, fin = _drain(eng)
    for rid, toks in rest.items():
        out.setdefault(rid, []).extend(toks)
    assert all(fin[r] for r in (r0, r1, r2))
    _assert_matches_naive(cases, [out[r0], out[r1], out[r2]])
    assert eng.cache.num_free_blocks == eng.cache.num_blocks


def test_engine_request_that_does_not_fit_waits():
    m = _model()
    eng = GenerationEngine(m, max_slots=4, num_blocks=3)  # 48 slots
    a = eng.add_request(_prompt(20, 21), 6)   # 26 tokens -> 2 blocks
    b = eng.add_request(_prompt(18, 22), 5)   # 23 tokens -> 2 blocks: does not fit beside a
    first = eng.step()
    assert {rid for rid, _, _ in first} == {a} and len(eng.waiting) == 1
    out, fin = _drain(eng)
    assert fin[a] and fin[b] and len(out[b]) == 5 and len(out[a]) + len(first) == 6
    assert eng.cache.num_free_blocks == 3
    with pytest.raises(ValueError):
        eng.add_request(_prompt(40, 23), 20)  # can never fit: refused at once, not queued forever


def test_engine_eos_stops_one_sequence_only():
    m = _model()
    pa, pb = _prompt(6, 31), _prompt(8, 32)
    ga, gb = m.generate([pa, pb], 10)
    eos = ga[2]
    eng = GenerationEngine(m, max_slots=2, num_blocks=8)
    a = eng.add_request(pa, 10, eos_token_id=eos)
    b = eng.add_request(pb, 10, eos_token_id=eos if eos not in gb else None)
    out, fin = _drain(eng)
    assert out[a] == ga[: ga.index(eos) + 1] and fin[a]
    assert out[b] == gb and fin[b]


@pytest.mark.gpu
def test_cached_path_on_gpu_is_as_accurate_as_full_forward():
    """bf16 model on the GPU (HIP prefill attention, HIP cache append and paged decode) against an
    fp32 copy on the reference path. Yardstick: the existing full bf16 forward's own error against
    that reference, measured here; the cached path may have at most twice that plus 1e-3 max|logit|."""
    from ray_community_amd import ops

    ref_model = _model()
    cfg = ref_model.cfg
    assert ops.paged_decode_supported(16, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads)
    m = build_llama("llama3-tiny", device="cuda", dtype=torch.bfloat16).eval()
    m.load_state_dict(ref_model.state_dict())
    ref_model = build_llama("llama3-tiny", dtype=torch.float32).eval()
    ref_model.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})  # the bf16-rounded weights
    cached, want, own = _teacher_forced(m, ref_model, "cuda")
    scale = want.abs().max().item()
    e_cached, e_full = (cached - want).abs().max().item(), (own - want).abs().max().item()
    print(f"cached err {e_cached:.3e}, full bf16 forward err {e_full:.3e}, max |logit| {scale:.3e}")
    assert torch.isfinite(cached).all()
    assert e_cached <= 2 * e_full + 1e-3 * scale
    out = m.generate([_prompt(5, 1), _prompt(130, 3)], 6)
    assert [len(o) for o in out] == [6, 6]


def test_cache_rollback_is_exact():
    m = _model()
    cache = PagedKVCache(m.cfg, 4, 16, dtype=torch.float32)
    first = cache.allocate("a", 16)
    cache.allocate("a", 1)  # takes a second block
    assert cache.num_free_blocks == 2
    cache.rollback("a", 1)  # ... which goes back
    assert cache.num_free_blocks == 3 and cache.length("a") == 16 and cache.blocks_held("a") == 1
    again = cache.allocate("a", 1)
    assert again[0] // 16 != first[0] // 16 and cache.blocks_held("a") == 2
    cache.rollback("a", 17)  # nothing left: the sequence is forgotten
    assert cache.num_free_blocks == 4 and cache.length("a") == 0 and "a" not in cache._lens
    with pytest.raises(ValueError):
        cache.rollback("a", 1)
    # decode_step is all or nothing: one full block left, two sequences that each need a new one
    cache.allocate("p", 16), cache.allocate("q", 16), cache.allocate("r", 16)
    with pytest.raises(KVCacheFull):
        m.decode_step([1, 2], cache, ["p", "q"])
    assert cache.num_free_blocks == 1 and cache.length("p") == 16 and cache.blocks_held("p") == 1
    with pytest.raises(KVCacheFull):  # a sequence first seen by decode_step leaves no trace either
        m.decode_step([1, 2], cache, ["new", "q"])
    assert cache.num_free_blocks == 1 and "new" not in cache._lens and "new" not in cache._blocks


def test_failed_prefill_leaves_the_cache_as_it_was():
    m = _model()
    cache = PagedKVCache(m.cfg, 4, 16, dtype=torch.float32)
    with pytest.raises(KVCacheFull):  # 3 blocks for the first prompt, then 2 more for the second
        m.prefill([_prompt(40, 71), _prompt(20, 72)], None, cache, ["a", "b"])
    assert cache.num_free_blocks == cache.num_blocks == 4
    assert "a" not in cache._lens and "a" not in cache._blocks
    assert cache.allocate("x", 64) == list(range(64))  # the free list is in its original order


def test_engine_cancel_frees_slot_and_blocks():
    m = _model()
    eng = GenerationEngine(m, max_slots=1, num_blocks=8)
    a = eng.add_request(_prompt(6, 41), 50)
    b = eng.add_request(_prompt(7, 42), 4)
    c = eng.add_request(_prompt(8, 43), 4)
    eng.step()
    assert eng.num_active == 1 and len(eng.waiting) == 2
    assert eng.cancel(c) and len(eng.waiting) == 1  # a waiting request
    assert eng.cancel(a) and eng.num_active == 0    # an active one: slot and blocks are free at once
    assert eng.cache.num_free_blocks == 8
    assert not eng.cancel(a) and not eng.cancel(12345)
    out, fin = _drain(eng)
    assert set(out) == {b} and fin[b] and len(out[b]) == 4  # no token of a or c after the cancel
    _assert_matches_naive([(tuple(_prompt(7, 42)), 4)], [out[b]])


def test_engine_requeues_when_prefill_fails():
    m = _model()

    class Flaky:
        """The model, with a prefill that fails once (as when a shared cache is drained by others)."""
        cfg, embed = m.cfg, m.embed
        decode_step = staticmethod(m.decode_step)
        fail = True

        def prefill(self, *a, **kw):
            if self.fail:
                self.fail = False
                raise KVCacheFull("taken by someone else")
            return m.prefill(*a, **kw)

    eng = GenerationEngine(Flaky(), max_slots=2, num_blocks=8)
    a = eng.add_request(_prompt(6, 51), 5)
    b = eng.add_request(_prompt(9, 52), 5)
    with pytest.raises(KVCacheFull):
        eng.step()
    assert eng.num_active == 0 and [r.rid for r in eng.waiting] == [a, b]  # back in line, in order
    assert eng.cache.num_free_blocks == 8
    out, fin = _drain(eng)
    assert fin[a] and fin[b]
    _assert_matches_naive([(tuple(_prompt(6, 51)), 5), (tuple(_prompt(9, 52)), 5)], [out[a], out[b]])


def test_engine_refuses_prompt_that_prefill_cannot_pad():
    m = build_llama("llama3-tiny", dtype=torch.float32, max_seq_len=200)
    eng = GenerationEngine(m, max_slots=2, num_blocks=16)
    with pytest.raises(ValueError, match="pads to 256"):
        eng.add_request(_prompt(130, 61), 5)  # 135 <= 200, but prefill would pad the prompt to 256
    eng.add_request(_prompt(100, 62), 5)
    assert len(eng.waiting) == 1
