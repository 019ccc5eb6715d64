"""Speculative decoding on the GPU (llama3-tiny bf16, HIP paged attention, split-KV verify).

On the GPU ``extend`` and ``decode_step`` round differently, so a near-tie may resolve differently
from the plain stream; the test therefore checks every emitted token against an fp32 model instead
of stream equality. Each stream is teacher-forced through the same weights in fp32 on the CPU
(one causal forward over prompt + stream): an emitted greedy token's fp32 logit must be within ``2 * E`` of
its row's maximum, ``E`` being the maximum absolute error, measured here, of the bf16 GPU
``prefill`` logits against the fp32 model on these prompts (a path this feature does not touch):
the yardstick-times-two rule of test_llama_extend.py. A sampled run must stay inside each step's
kept set, computed by ``sample_kept_ref`` on the fp32 logits with ``top_p`` widened by the margin of
test_sampling_gpu.py (1e-3) plus the mass the logit error ``2 * E`` can move.
"""
import functools

import pytest
import torch

from ray_community_amd.models import GenerationEngine, PagedKVCache, build_llama
from ray_community_amd.ops import reference as ref

gpu = pytest.mark.gpu
N_NEW = 32
K = 4
MARGIN = 1e-3


def _prompt(n, seed, span=6):
    g = torch.Generator().manual_seed(seed)
    spans = torch.randint(0, 1024, (3, span), generator=g).tolist()
    order = torch.randint(0, 3, (n // span + 1,), generator=g).tolist()
    return [t for o in order for t in spans[o]][:n]


PROMPTS = [_prompt(9, 1), _prompt(48, 2), _prompt(100, 3), _prompt(130, 4)]


@functools.lru_cache(maxsize=None)
def _models():
    torch.manual_seed(0)
    m32 = build_llama("llama3-tiny", dtype=torch.float32).eval()
    m16 = build_llama("llama3-tiny", device="cuda").eval()
    m16.load_state_dict(m32.state_dict())
    return m32, m16


def _fp32_logits(m32, seqs):
    """fp32 logits at every position of every sequence (one causal forward each)."""
    with torch.no_grad():
        return [m32(torch.tensor([s]))[0] for s in seqs]


@functools.lru_cache(maxsize=None)
def _yardstick():
    """E: max |bf16 GPU prefill logits - fp32 logits| at the prompts' last tokens."""
    m32, m16 = _models()
    cache = PagedKVCache(m16.cfg, 64, 16, device="cuda")
    got = m16.prefill(PROMPTS, None, cache, list(range(len(PROMPTS)))).float().cpu()
    want = torch.stack([lg[-1] for lg in _fp32_logits(m32, PROMPTS)])
    E = (got - want).abs().max().item()
    print(f"E = {E:.4f}")
    return E


def _run(speculative, **sampling):
    _, m16 = _models()
    eng = GenerationEngine(m16, max_slots=4, num_blocks=64, speculative=speculative)
    rids = [eng.add_request(p, N_NEW, **sampling) for p in PROMPTS]
    streams = {r: [] for r in rids}
    while eng.has_work():
        for rid, tok, _ in eng.step():
            streams[rid].append(tok)
    assert eng.cache.num_free_blocks == 64
    return [streams[r] for r in rids], dict(eng.spec_stats)


class _Replay:
    """Proposes the continuation a previous run produced."""
    num_draft = K

    def __init__(self, streams):
        self.full = [p + s for p, s in zip(PROMPTS, streams)]

    def propose(self, history, k):
        for f in self.full:
            if f[: len(history)] == history:
                return f[len(history): len(history) + k]
        return []


@gpu
def test_greedy_streams_are_correct_and_reproducible():
    m32, _ = _models()
    E = _yardstick()
    streams, st = _run(K)
    assert all(len(s) == N_NEW for s in streams)
    assert st["accepted"] <= st["drafted"]
    again, _ = _run(K)
    assert again == streams
    for p, s, lg in zip(PROMPTS, streams, _fp32_logits(m32, [p + s for p, s in zip(PROMPTS, streams)])):
        for i, tok in enumerate(s):
            x = lg[len(p) - 1 + i]
            assert (x.max() - x[tok]).item() <= 2 * E, (len(p), i, (x.max() - x[tok]).item(), E)
    replay, st = _run(_Replay(streams))
    assert st["accepted"] > 0 and st["verify_steps"] > 0
    for p, s, lg in zip(PROMPTS, replay, _fp32_logits(m32, [p + s for p, s in zip(PROMPTS, replay)])):
        for i, tok in enumerate(s):
            x = lg[len(p) - 1 + i]
            assert (x.max() - x[tok]).item() <= 2 * E


@gpu
def test_sampled_streams_stay_in_the_kept_set():
    m32, _ = _models()
    E = _yardstick()
    T, top_p = 0.9, 0.9
    streams, st = _run(K, temperature=T, top_p=top_p, seed=3)
    assert all(len(s) == N_NEW for s in streams) and st["accepted"] <= st["drafted"]
    for p, s, lg in zip(PROMPTS, streams, _fp32_logits(m32, [p + s for p, s in zip(PROMPTS, streams)])):
        for i, tok in enumerate(s):
            x = lg[len(p) - 1 + i]
            # a logit error of 2E scales a weight by at most exp(2E / T): every cumulative mass
            # fraction moves by less than exp(4E / T) - 1; the 1e-3 is test_sampling_gpu.py's margin
            slack = MARGIN + (torch.exp(torch.tensor(4 * E / T)).item() - 1)
            _, keep = ref.sample_kept_ref(x, T, 0, min(top_p + slack, 1.0), 0.0)
            assert keep[tok], (len(p), i, E)
