"""Sampling penalties and token logprobs on the CPU: the references of ``ops.penalize_logits`` and
``ops.token_logprobs`` against brute-force float64 loops, the plumbing through ``Sampling``,
``Llama.generate``, ``GenerationEngine`` (llama3-tiny, fp32, reference path) and ``LlamaDeployment``.

The speculative and engine/generate equalities compare streams whose logits come from different
reductions (``extend`` / ``decode_step``, about 1e-6 apart in fp32). As in test_speculative_cpu.py the
lm_head is scaled by ``LOGIT_SCALE`` so that decisions are peaked and that difference decides nothing.
"""
import functools
import json
import math
import urllib.request

import pytest
import torch

import ray_community_amd as ray
from ray_community_amd import ops, serve
from ray_community_amd.models import GenerationEngine, build_llama
from ray_community_amd.models.decoding import Sampling, Stream, _pack_histories, use_fused_sampling
from ray_community_amd.ops import reference as ref
from ray_community_amd.serve.llm import LlamaDeployment

PORT = 18167
LOGIT_SCALE = 12.0
V_TINY = 1024
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.25)


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


# --------------------------------------------------------------------------------- references
def _brute_penalties(x, tokens, rng, rep, pres, freq):
    """Float64 loop over one row: the real-number result at the fp32 values of the parameters."""
    start, prompt_end, end = rng
    rep, pres, freq = _f32(rep), _f32(pres), _f32(freq)
    out, counts = [], []
    for i, xi in enumerate(x.tolist()):
        seen = i in tokens[start:end]
        c = tokens[prompt_end:end].count(i)
        y = xi
        if seen:
            y = xi / rep if xi > 0 else xi * rep
        y -= freq * c
        if c > 0:
            y -= pres
        out.append(y)
        counts.append(c)
    return out, counts


def test_penalize_ref_against_the_float64_loop():
    V = 16
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, V, generator=g) * 4
    x[:, 5] = 0.0                      # x == 0 in the history
    x[:, 1], x[:, 2] = 2.71, -3.3      # x > 0 and x < 0 in the history
    x[:, 9], x[:, 10] = -1.7, 6.1
    x[:, 7] = -0.0
    #          prompt-only: 1, 7   both: 2, 5   output-only: 9 (x3), 10   absent: the rest
    tokens = [1, 2, 5, 7, 1, 9, 2, 9, 5, 10, 9, 2]
    ranges = [(0, 5, 12), (0, 5, 12), (0, 0, 12), (3, 5, 5)]   # row 2: all output; row 3: prompt only
    rep, pres, freq = [1.3, 0.7, 1.0, 2.0], [0.4, -0.5, 1.5, 0.3], [0.25, 0.1, -0.3, 0.9]
    for dtype in (torch.float32, torch.bfloat16):
        xs = x.to(dtype)
        got = ref.penalize_logits_ref(xs, tokens, ranges, rep, pres, freq)
        assert got.dtype == torch.float32 and got.shape == (4, V)
        for b in range(4):
            want, counts = _brute_penalties(xs[b].double(), tokens, ranges[b], rep[b], pres[b], freq[b])
            hist = set(tokens[ranges[b][0]: ranges[b][2]])
            for i in range(V):
                bound = 2.0 ** -24 * (3 * abs(want[i]) + abs(_f32(freq[b])) * counts[i] + abs(_f32(pres[b])))
                assert abs(float(got[b, i]) - want[i]) <= bound, (dtype, b, i, float(got[b, i]), want[i], bound)
                if i not in hist:  # absent: the exact image, bit for bit
                    assert got[b, i].view(torch.int32) == xs[b, i].float().view(torch.int32)
        changed = (got != xs.float()).sum(dim=1).tolist()
        # row 0 sees 1, 2, 5, 9, 10 and 7 (x = -0 in the prompt: unchanged); row 3 sees 7 and 1
        assert changed[0] == 5 and changed[3] == 1


def test_neutral_parameters_copy_exactly():
    g = torch.Generator().manual_seed(2)
    for dtype in (torch.float32, torch.bfloat16):
        x = (torch.randn(3, 50, generator=g) * 4).to(dtype)
        x[0, 3], x[1, 4] = -0.0, float("inf")
        got = ref.penalize_logits_ref(x, list(range(40)), [(0, 10, 40), (5, 5, 5), (0, 40, 40)], [1.0] * 3, [0.0] * 3,
                                      [0.0] * 3)
        assert torch.equal(got.view(torch.int32), x.float().view(torch.int32))
        assert torch.equal(ops.penalize_logits(x, list(range(40)), [(0, 10, 40), (5, 5, 5), (0, 40, 40)]).view(torch.int32),
                           x.float().view(torch.int32))


def _brute_order(row, n):
    return sorted(range(len(row)), key=lambda i: (-row[i], i))[:n]


def test_token_logprobs_ref():
    """Bound as in the GPU test: 2**-19 + 2**-21 * |lp|, which covers fp32 ``exp`` (1 ulp), the
    roundings of ``x - m`` and of the result."""
    V, n = 37, 5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, V, generator=g) * 4
    x[1] = 1.5                                        # all equal: ids 0..n-1
    x[2] = torch.arange(V, dtype=torch.float32) * -0.5
    x[2, 10:14] = x[2, 3]                             # values at ranks 3..7 tie: the tie straddles place n = 5
    x[3] = -x[3].abs() - 1.0
    x[3, 20], x[3, 2] = 0.0, -0.0                     # the two maxima, -0 == +0: by index
    tokens = torch.tensor([4, 36, 11, 2, 0])
    for dtype in (torch.float32, torch.bfloat16):
        xs = x.to(dtype)
        lp, ids, tlp = ref.token_logprobs_ref(xs, tokens, n)
        assert lp.dtype == torch.float32 and ids.dtype == torch.int64 and tlp.dtype == torch.float32
        assert lp.shape == (5,) and ids.shape == (5, n) and tlp.shape == (5, n)
        want = torch.log_softmax(xs.double(), dim=1)
        for b in range(5):
            assert ids[b].tolist() == _brute_order(xs[b].float().tolist(), n)
            for got, w in [(lp[b], want[b, tokens[b]])] + [(tlp[b, j], want[b, ids[b, j]]) for j in range(n)]:
                assert abs(float(got) - float(w)) <= 2.0 ** -19 + 2.0 ** -21 * abs(float(w))
        assert ids[1].tolist() == [0, 1, 2, 3, 4]
        assert ids[2].tolist() == [0, 1, 2, 3, 10]
        assert ids[3].tolist()[:2] == [2, 20]
    lp, ids, tlp = ref.token_logprobs_ref(x[:, :3], tokens.clamp(max=2), 5)   # top_n > V: -1 / -inf tail
    assert ids[:, 3:].eq(-1).all() and tlp[:, 3:].eq(float("-inf")).all() and ids[:, :3].ge(0).all()
    lp0, ids0, tlp0 = ops.token_logprobs(x, tokens, 0)
    assert ids0.shape == (5, 0) and tlp0.shape == (5, 0) and torch.equal(lp0, ref.token_logprobs_ref(x, tokens, 5)[0])


def test_out_of_range_parameters():
    x = torch.zeros(2, 8)
    for kw in (dict(repetition=0.0), dict(repetition=-1.0), dict(repetition=float("nan")), dict(repetition=float("inf")),
               dict(presence=float("inf")), dict(frequency=float("nan")), dict(repetition=[1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ops.penalize_logits(x, [1, 2], [(0, 1, 2), (0, 0, 0)], **kw)
    with pytest.raises(ValueError, match="tokens"):
        ops.penalize_logits(x, [1, 8], [(0, 1, 2), (0, 0, 0)], presence=1.0)
    with pytest.raises(ValueError, match="tokens"):
        ops.penalize_logits(x, [-1, 2], [(0, 1, 2), (0, 0, 0)], presence=1.0)
    for bad in ([(0, 1, 3), (0, 0, 0)], [(1, 0, 2), (0, 0, 0)], [(-1, 0, 2), (0, 0, 0)], [(0, 2, 1), (0, 0, 0)],
                [(0, 1, 2)]):
        with pytest.raises(ValueError, match="ranges"):
            ops.penalize_logits(x, [1, 2], bad, presence=1.0)
    for n in (-1, 21, True, 2.0):
        with pytest.raises(ValueError, match="top_n"):
            ops.token_logprobs(x, torch.zeros(2, dtype=torch.long), n)
    assert ops.penalize_logits(x[:0], [], []).shape == (0, 8)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(presence_penalty=float("inf")),
               dict(frequency_penalty=float("-inf")), dict(logprobs=21), dict(logprobs=-1), dict(logprobs=True),
               dict(logprobs=1.0)):
        with pytest.raises(ValueError):
            Sampling(**kw)
    s = Sampling(0.5, 3, 0.9, 0.0, None, False, 1.2, 0.1, 0.2, 4)   # appended after the existing fields
    assert (s.repetition_penalty, s.presence_penalty, s.frequency_penalty, s.logprobs) == (1.2, 0.1, 0.2, 4)
    assert Sampling(presence_penalty=0.5).fused and Sampling(logprobs=0).fused and Sampling(repetition_penalty=2).penalized
    assert not Sampling().fused and not Sampling(logprobs=3).penalized
    assert use_fused_sampling(False, 1.0, 0.0, frequency_penalty=0.1) and not use_fused_sampling(False, 1.0, 0.0)


def test_pack_histories_shares_a_region_per_stream():
    a = Stream("a", [1, 2, 3, 4], 8, Sampling(presence_penalty=1.0), prompt_len=3)
    b = Stream("b", [7, 8], 8, Sampling())
    flat, ranges = _pack_histories([(a, 1, ()), (a, 2, (9,)), (a, 3, (9, 10)), (b, 0, ())])
    assert flat == [1, 2, 3, 4, 9, 10, 7, 8]
    assert ranges == [(0, 3, 4), (0, 3, 5), (0, 3, 6), (6, 8, 8)]
    assert b.prompt_len == 2 and a.logprobs == []


# ----------------------------------------------------------------------------------- tiny Llama
@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    m = build_llama("llama3-tiny", dtype=torch.float32).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(LOGIT_SCALE)
    return m


def _rand(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V_TINY, (n,), generator=g).tolist()


def _repeats(n, seed, span=6):
    spans = [_rand(span, seed + i) for i in range(3)]
    return [t for o in _rand(n // span + 1, seed + 9) for t in spans[o % 3]][:n]


PROMPTS = [_rand(7, 11), _rand(40, 12), _repeats(70, 13)]


class _Scripted:
    """Drafts 3 tokens of the known continuation of whichever prompt the history starts with,
    every third drafted token replaced by a wrong one."""
    num_draft = 3

    def __init__(self, streams):
        self.full = [list(p) + list(s) for p, s in zip(PROMPTS, streams)]
        self.count = 0

    def propose(self, history, k):
        full = next(f for f, p in zip(self.full, PROMPTS) if history[:len(p)] == p)
        assert history == full[:len(history)], "the speculative stream left the plain one"
        out = []
        for t in full[len(history): len(history) + k]:
            self.count += 1
            out.append((t + 1) % V_TINY if self.count % 3 == 0 else t)
        return out


def _engine_streams(model, prompts, n, requests, **engine_kw):
    eng = GenerationEngine(model, max_slots=len(prompts), num_blocks=64, **engine_kw)
    rids = [eng.add_request(p, n, **kw) for p, kw in zip(prompts, requests)]
    out, lps = {r: [] for r in rids}, {r: [] for r in rids}
    while eng.has_work():
        events = eng.step()
        for rid, tok, _ in events:
            out[rid].append(tok)
        for rid in {e[0] for e in events}:
            got = eng.pop_logprobs(rid)
            assert got == [] or [e[0] for e in got] == [t for r, t, _ in events if r == rid]  # aligned
            lps[rid].extend(got)
    assert not eng._logprobs
    return [out[r] for r in rids], [lps[r] for r in rids]


def test_presence_penalty_never_repeats_a_token():
    model, n = _model(), 60
    prompt = _repeats(30, 5)
    plain = model.generate([prompt], n)[0]
    assert len(set(plain)) < n  # the unpenalized greedy stream does repeat itself
    got = model.generate([prompt], n, presence_penalty=1e6)[0]
    assert len(got) == n and len(set(got)) == n


def test_neutral_penalties_give_the_fused_stream():
    model = _model()
    for mode in (dict(temperature=0.0), dict(temperature=0.9, top_p=0.9, seed=8)):
        plain = model.generate(PROMPTS, 16, fused_sampling=True, **mode)
        assert model.generate(PROMPTS, 16, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                              **{**mode, "fused_sampling": True}) == plain
        # a neutral row next to a penalized one goes through penalize_logits and keeps its stream
        reqs = [dict(mode), dict(mode, **PEN), dict(mode)]
        got, _ = _engine_streams(model, PROMPTS, 16, reqs, fused_sampling=True)
        assert got[0] == plain[0] and got[2] == plain[2]


@pytest.mark.parametrize("mode", [dict(temperature=0.0), dict(temperature=0.9, top_p=0.9, seed=8)], ids=["greedy", "sampled"])
def test_engine_generate_and_speculative_agree_with_penalties(mode):
    model, n = _model(), 24
    plain = model.generate(PROMPTS, n, fused_sampling=True, **mode)
    want = model.generate(PROMPTS, n, **mode, **PEN)
    assert want != plain
    got, _ = _engine_streams(model, PROMPTS, n, [dict(mode, **PEN)] * 3)
    assert got == want
    # prompt lookup rarely drafts once repeats are penalized, so one run drafts the known
    # continuation with every third draft token spoiled: accepted and rejected drafts both occur
    assert model.generate(PROMPTS, n, speculative=3, **mode, **PEN) == want
    scripted = _Scripted(want)
    assert model.generate(PROMPTS, n, speculative=scripted, **mode, **PEN) == want
    stats = model.spec_stats
    assert stats["verify_steps"] > 0 and 0 < stats["accepted"] < stats["drafted"]
    got, _ = _engine_streams(model, PROMPTS, n, [dict(mode, **PEN)] * 3, speculative=_Scripted(want))
    assert got == want


def test_greedy_logprobs_match_a_plain_forward():
    """The cached forward and the plain one reduce in different orders (about 1e-6 relative in
    fp32, on logits of magnitude up to about 30 here): 1e-3 absolute is far above that and far below
    a wrong entry."""
    model, n = _model(), 6
    toks, lps = model.generate(PROMPTS[:2], n, logprobs=3)
    assert toks == model.generate(PROMPTS[:2], n, fused_sampling=True)
    for prompt, stream, entries in zip(PROMPTS, toks, lps):
        assert [e[0] for e in entries] == stream and len(entries) == n
        seq = list(prompt)
        for tok, lp, top in entries:
            assert len(top) == 3 and top[0] == (tok, lp)   # greedy: the chosen token leads
            assert top[0][1] >= top[1][1] >= top[2][1]
            with torch.no_grad():
                want = torch.log_softmax(model(torch.tensor([seq]))[0, -1].double(), dim=0)
            assert abs(lp - float(want[tok])) <= 1e-3
            for i, v in top:
                assert abs(v - float(want[i])) <= 1e-3
            seq.append(tok)
    assert model.generate([], 4, logprobs=0) == ([], [])
    alone, lp0 = model.generate(PROMPTS[:1], 3, logprobs=0)
    assert [len(e[2]) for e in lp0[0]] == [0, 0, 0] and alone[0] == toks[0][:3]


def test_engine_pop_logprobs_and_speculative_logprobs():
    model, n = _model(), 12
    mode = dict(temperature=0.9, top_p=0.9, seed=8)
    want_t, want_l = model.generate(PROMPTS, n, logprobs=2, **mode, **PEN)
    reqs = [dict(mode, logprobs=2, **PEN), dict(mode, **PEN), dict(mode, logprobs=2, **PEN)]
    got_t, got_l = _engine_streams(model, PROMPTS, n, reqs)
    assert got_t == want_t
    assert got_l[1] == [] and [e[0] for e in got_l[0]] == got_t[0] and len(got_l[2]) == n
    spec_t, spec_l = _engine_streams(model, PROMPTS, n, reqs, speculative=_Scripted(want_t))
    assert spec_t == want_t
    for a, b in zip(got_l[0] + got_l[2], spec_l[0] + spec_l[2]):
        assert a[0] == b[0] and [i for i, _ in a[2]] == [i for i, _ in b[2]]
        assert math.isclose(a[1], b[1], abs_tol=1e-3)   # extend vs decode_step logits: see above
    for a, b in zip(got_l[0], want_l[0]):
        assert a[0] == b[0] and math.isclose(a[1], b[1], abs_tol=1e-3)


# ----------------------------------------------------------------------------------------- Serve
@pytest.fixture(scope="module")
def llm_handle():
    ray.init(num_cpus=4, log_to_driver=False)
    serve.start(http_options={"port": PORT})
    app = LlamaDeployment.bind("llama3-tiny", dtype="float32", seed=0, max_slots=4, num_blocks=64)
    yield serve.run(app, name="llm_penalties", route_prefix="/llm")
    serve.shutdown()
    ray.shutdown()


def _post(body):
    req = urllib.request.Request(f"http://127.0.0.1:{PORT}/llm", method="POST", data=json.dumps(body).encode(),
                                 headers={"content-type": "application/json"})
    with urllib.request.urlopen(req, timeout=60) as r:
        return r.read().decode()


def test_serve_handle_and_http(llm_handle):
    torch.manual_seed(0)  # the replica seeds its weights the same way
    model = build_llama("llama3-tiny", dtype=torch.float32).eval()
    prompt, n = _repeats(20, 3), 10
    kw = dict(presence_penalty=1e6, repetition_penalty=1.2)
    want, want_lp = model.generate([prompt], n, logprobs=2, **kw)
    stream = llm_handle.options(method_name="generate", stream=True)
    items = list(stream.remote(prompt, max_new_tokens=n, logprobs=2, **kw))
    assert [it["token"] for it in items] == want[0] and len(set(want[0])) == n
    for it, (tok, lp, top) in zip(items, want_lp[0]):
        assert set(it) == {"token", "logprob", "top_logprobs"}
        # the replica's engine decodes over 4 slots, generate over 1 row: fp32 reductions about 1e-6 apart
        assert abs(it["logprob"] - lp) <= 1e-3 and [i for i, _ in it["top_logprobs"]] == [i for i, _ in top]
        assert it["top_logprobs"][0] == [it["token"], it["logprob"]]
    bare = list(stream.remote(prompt, max_new_tokens=n, **kw))
    assert bare == want[0] and all(isinstance(t, int) for t in bare)   # without logprobs: bare ids

    text = _post({"prompt_tokens": prompt, "max_new_tokens": n, "logprobs": 2, **kw})
    assert text.endswith("\n")
    assert [json.loads(line) for line in text.splitlines()] == items     # NDJSON
    text = _post({"prompt_tokens": prompt, "max_new_tokens": n, **kw})
    assert [int(x) for x in text.split()] == want[0]
    with pytest.raises(Exception):
        list(stream.remote(prompt, max_new_tokens=2, repetition_penalty=0.0))
    assert llm_handle.status.remote().result()["active"] == 0
