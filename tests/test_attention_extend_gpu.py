"""The gfx950 paged extend attention (ops/csrc/attention_extend.hip: causal attention of a ragged
batch of query chunks over a paged KV cache), checked per (token, head) row against a float64
oracle written here, independent of ops/reference.py.

Metric and bound are those of test_attention_decode_edges_gpu.py: ``_row_err`` = max_d |out - want|
/ max_d |want| per (token, head) row, bound ``ROW_BOUND`` = 2**-7 = twice the bf16 rounding floor of
an attention output row (profiles/decode_attention.md); the output format is the same here.

Case data: every cache is NaN except the live slots, blocks are handed out in shuffled order and
block-table padding points at an all-NaN block, so any read of a dead slot, of a block no
sequence owns or of a table entry past a sequence's pages poisons the output. Each sequence with
new tokens carries two spiked keys: the key AT its first new token's position and the key one
AFTER it are copies of that token's query (score sqrt(D) against ~N(0, 1) elsewhere). A causal
bound off by one in either direction then moves the oracle by far more than the bound
(``test_cases_have_teeth``, CPU only), so the same slip in the kernel fails the GPU tests.

Teeth exemptions: a sequence with one new token has no key past its position, so ``key <= p + 1``
(clamped to the context) is the true mask. In the shape-matrix batch these are (prior, new) =
(0, 1) and (17, 1): 2 of the batch's 8 sequences, and 2 of its 14 (sequence, direction) checks;
the batch is set by the issue, so that count is fixed. Every ``key <= p - 1`` check holds.

Worst rows measured on one MI355X are recorded in profiles/extend_attention.md.
"""
import functools
import itertools

import pytest
import torch

from ray_community_amd import ops

gpu = pytest.mark.gpu

ROW_BOUND = 2.0 ** -7
HK = 2
NAN = float("nan")
MATRIX = [(0, 1), (0, 130), (5, 31), (47, 32), (63, 33), (200, 129), (64, 0), (17, 1)]
EDGES = [(p, n) for p in (0, 1, 63, 64, 65) for n in (1, 15, 16, 17, 127, 128, 129)]


# ------------------------------------------------------------------------------ oracle and metric
def _oracle(c, shift=0):
    """float64 extend attention of case ``c`` on the CPU: query i of sequence b (position p =
    ctx - n + i) attends keys 0 .. min(p + shift, ctx - 1) of its sequence, key j living in slot
    table[b, j // page] * page + j % page. ``shift`` = 0 is the truth; +1 / -1 are the off-by-one
    masks of the teeth test. A query with no visible key gives zeros. Returns [T, Hq*D]."""
    Hq, D, page = c["Hq"], c["D"], c["page"]
    G = Hq // HK
    kf = c["k_cache"].double().reshape(-1, HK, D)
    vf = c["v_cache"].double().reshape(-1, HK, D)
    qf = c["q"].double().reshape(-1, Hq, D)
    table = c["table"].tolist()
    out = torch.zeros(qf.shape[0], Hq, D, dtype=torch.float64)
    for b, ((prior, n), q0) in enumerate(zip(c["seqs"], c["cu"].tolist())):
        if n == 0:
            continue
        ctx = prior + n
        slots = [table[b][j // page] * page + j % page for j in range(ctx)]
        k = kf[slots].repeat_interleave(G, dim=1)
        v = vf[slots].repeat_interleave(G, dim=1)
        s = torch.einsum("ihd,nhd->ihn", qf[q0: q0 + n], k) * c["scale"]
        lim = (torch.arange(prior, ctx) + shift).clamp(max=ctx - 1)
        hidden = torch.arange(ctx)[None, :] > lim[:, None]
        s = s.masked_fill(hidden[:, None, :], float("-inf"))
        mx = s.amax(-1, keepdim=True)
        p = torch.exp(s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
        den = p.sum(-1, keepdim=True)
        p = torch.where(den > 0, p / den.clamp_min(1e-300), torch.zeros_like(p))
        out[q0: q0 + n] = torch.einsum("ihn,nhd->ihd", p, v)
    return out.reshape(-1, Hq * D)


def _row_err(out, want, D):
    a = out.detach().cpu().double().reshape(out.shape[0], -1, D)
    b = want.reshape(want.shape[0], -1, D)
    num, den = (a - b).abs().amax(-1), b.abs().amax(-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))


def _check_rows(out, want, D, label):
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == tuple(want.shape)
    assert torch.isfinite(out).all(), f"{label}: non-finite output"
    worst = _row_err(out, want, D).max().item() if out.numel() else 0.0
    print(f"{label}: max row err {worst:.3e} (bound {ROW_BOUND:.3e})")
    assert worst < ROW_BOUND, label
    return worst


# ------------------------------------------------------------------------------------ case data
@functools.lru_cache(maxsize=None)
def _case(page, D, G, seqs=tuple(MATRIX), seed=0, spikes=True):
    """One ragged batch on the CPU (bf16): packed q, NaN-filled caches with shuffled blocks, table,
    context_lens, cu_q_lens. Cached: build once, never modified."""
    g = torch.Generator().manual_seed(1000 * page + 10 * D + G + seed)
    Hq = HK * G
    need = [-(-(p + n) // page) for p, n in seqs]
    num_blocks = sum(need) + 3  # spare blocks stay all NaN; one of them pads the table
    perm = torch.randperm(num_blocks, generator=g).tolist()
    pad = perm[sum(need)]
    table = torch.full((len(seqs), max(need + [1])), pad, dtype=torch.int32)
    k_cache = torch.full((num_blocks, page, HK, D), NAN, dtype=torch.bfloat16)
    v_cache = torch.full((num_blocks, page, HK, D), NAN, dtype=torch.bfloat16)
    T = sum(n for _, n in seqs)
    q = torch.randn(T, Hq, D, generator=g).to(torch.bfloat16)
    cu = [0] + list(itertools.accumulate(n for _, n in seqs))
    nxt = 0
    for b, (prior, n) in enumerate(seqs):
        ctx = prior + n
        k = torch.randn(ctx, HK, D, generator=g).to(torch.bfloat16)
        v = torch.randn(ctx, HK, D, generator=g).to(torch.bfloat16)
        if spikes and n >= 1:  # keys at and just past the first new token's position copy its query
            for j in (prior, prior + 1):
                if j < ctx:
                    k[j] = q[cu[b], ::G]
        blocks = perm[nxt: nxt + need[b]]
        nxt += need[b]
        table[b, : len(blocks)] = torch.tensor(blocks, dtype=torch.int32)
        for j in range(ctx):
            k_cache[blocks[j // page], j % page] = k[j]
            v_cache[blocks[j // page], j % page] = v[j]
    return dict(page=page, D=D, Hq=Hq, seqs=list(seqs), scale=D ** -0.5, q=q.reshape(T, Hq * D), k_cache=k_cache,
                v_cache=v_cache, table=table, lens=torch.tensor([p + n for p, n in seqs], dtype=torch.int32),
                cu=torch.tensor(cu, dtype=torch.int32), max_q=max(n for _, n in seqs))


@functools.lru_cache(maxsize=None)
def _want(page, D, G, seqs=tuple(MATRIX), seed=0, spikes=True):
    return _oracle(_case(page, D, G, seqs, seed, spikes))


def _run(c, device, q=None):
    d = torch.device(device)
    q = c["q"].to(d) if q is None else q
    return ops.paged_attention_extend(q, c["k_cache"].to(d), c["v_cache"].to(d), c["table"].to(d), c["lens"].to(d),
                                      c["cu"].to(d), c["max_q"], c["Hq"], HK, c["D"])


SHAPES = [(page, D, G) for page in (16, 48, 64) for D in (64, 128) for G in (1, 2, 4, 8)]


# ------------------------------------------------------------------------------- CPU: the test data
def test_cases_have_teeth():
    """Both off-by-one causal masks move the oracle by >= 4 * ROW_BOUND in some row of every
    sequence of the shape matrix, bar the exemptions named in the module docstring."""
    exempt = {(b, +1) for b, (_, n) in enumerate(MATRIX) if n == 1}  # no key past the only position
    checks = [(b, sh) for b, (_, n) in enumerate(MATRIX) if n >= 1 for sh in (+1, -1)]
    assert len(exempt) * 4 <= len(checks)
    assert len({b for b, _ in exempt}) * 4 <= len(MATRIX)
    for page, D, G in SHAPES:
        c, want = _case(page, D, G), _want(page, D, G)
        cu = c["cu"].tolist()
        for sh in (+1, -1):
            err = _row_err(_oracle(c, shift=sh), want, D)
            # a row that is all zero in the truth cannot occur; one that turns zero scores 1
            for b, (_, n) in enumerate(MATRIX):
                if n == 0:
                    continue
                worst = err[cu[b]: cu[b + 1]].max().item()
                if (b, sh) in exempt:
                    assert worst == 0.0
                else:
                    assert worst >= 4 * ROW_BOUND, (page, D, G, b, sh, worst)


def test_reference_path_matches_oracle_cpu():
    """CPU tensors take ops.reference.paged_attention_extend_ref; so does an unsupported head size."""
    for page, D, G in ((16, 64, 4), (48, 128, 1), (16, 96, 2)):
        c = _case(page, D, G)
        _check_rows(_run(c, "cpu"), _want(page, D, G), D, f"cpu reference page={page} D={D} G={G}")


def test_wrapper_argument_checks():
    c = _case(16, 64, 2)
    args = dict(q=c["q"], k=c["k_cache"], v=c["v_cache"], t=c["table"], l=c["lens"], cu=c["cu"])

    def call(max_q=c["max_q"], Hq=c["Hq"], **kw):
        a = {**args, **kw}
        return ops.paged_attention_extend(a["q"], a["k"], a["v"], a["t"], a["l"], a["cu"], max_q, Hq, HK, 64)

    call()
    for bad in (dict(q=c["q"][:, :-8]), dict(q=c["q"].float()), dict(v=c["v_cache"][:-1]), dict(t=c["table"][:-1]),
                dict(t=c["table"].long()), dict(l=c["lens"][:-1]), dict(cu=c["cu"][:-1]), dict(cu=c["cu"].long()),
                dict(max_q=-1), dict(max_q=c["q"].shape[0] + 1), dict(k=c["k_cache"].transpose(0, 1))):
        with pytest.raises(ValueError):
            call(**bad)
    assert "paged_attention_extend" in ops.__all__


# ----------------------------------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("page,D,G", SHAPES)
def test_shape_matrix(page, D, G):
    c = _case(page, D, G)
    _check_rows(_run(c, "cuda"), _want(page, D, G), D, f"matrix page={page} D={D} G={G}")


@gpu
@pytest.mark.parametrize("page", [16, 48])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_tile_edges(page, G, D):
    """new * G across 32 and 128 rows, contexts across the 64-key tile, one batch per shape."""
    c = _case(page, D, G, tuple(EDGES), 1)
    _check_rows(_run(c, "cuda"), _want(page, D, G, tuple(EDGES), 1), D, f"edges page={page} D={D} G={G}")


@gpu
@pytest.mark.parametrize("D,G", [(64, 2), (128, 4)])
def test_inplace_and_strided_q(D, G):
    c = _case(16, D, G)
    Hq, T = c["Hq"], c["q"].shape[0]
    base = _run(c, "cuda")
    fused = torch.randn(T, (Hq + 2 * HK) * D).to(torch.bfloat16).cuda()
    fused[:, : Hq * D] = c["q"].cuda()
    assert torch.equal(_run(c, "cuda", q=fused), base)
    wide = torch.zeros(T, Hq * D + 24, dtype=torch.bfloat16, device="cuda")
    wide[:, : Hq * D] = c["q"].cuda()
    view = wide[:, : Hq * D]
    assert not view.is_contiguous()
    assert torch.equal(_run(c, "cuda", q=view), base)
    _check_rows(base, _want(16, D, G), D, f"in-place D={D} G={G}")


@gpu
@pytest.mark.parametrize("page,D,G", [(16, 128, 4), (48, 64, 8), (64, 128, 1)])
def test_agrees_with_decode(page, D, G):
    seqs = tuple((p, 1) for p in (0, 1, 15, 16, 63, 64, 65, 200, 399))
    c, want = _case(page, D, G, seqs, 2), _want(page, D, G, seqs, 2)
    d = torch.device("cuda")
    ext = _run(c, "cuda")
    dec = ops.paged_attention_decode(c["q"].to(d), c["k_cache"].to(d), c["v_cache"].to(d), c["table"].to(d),
                                     c["lens"].to(d), c["Hq"], HK, D)
    _check_rows(ext, want, D, f"extend new=1 page={page} D={D} G={G}")
    _check_rows(dec, want, D, f"decode page={page} D={D} G={G}")
    # two kernels, two summation orders: each within the bound of the oracle, so within twice of each other
    assert _row_err(ext, dec.cpu().double(), D).max().item() < 2 * ROW_BOUND


@gpu
@pytest.mark.parametrize("D,G", [(64, 2), (128, 4)])
def test_agrees_with_flash_forward(D, G):
    S, Hq, page = 256, HK * G, 16
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(S, (Hq + 2 * HK) * D, generator=g).to(torch.bfloat16)
    blocks = torch.randperm(S // page + 1, generator=g).tolist()
    k_cache = torch.full((S // page + 1, page, HK, D), NAN, dtype=torch.bfloat16)
    v_cache = torch.full_like(k_cache, NAN)
    k_cache[blocks[:-1]] = qkv[:, Hq * D: (Hq + HK) * D].reshape(S // page, page, HK, D)
    v_cache[blocks[:-1]] = qkv[:, (Hq + HK) * D:].reshape(S // page, page, HK, D)
    c = dict(page=page, D=D, Hq=Hq, seqs=[(0, S)], scale=D ** -0.5, q=qkv[:, : Hq * D].contiguous(), k_cache=k_cache,
             v_cache=v_cache, table=torch.tensor([blocks[:-1]], dtype=torch.int32),
             lens=torch.tensor([S], dtype=torch.int32), cu=torch.tensor([0, S], dtype=torch.int32), max_q=S)
    want = _oracle(c)
    _check_rows(_run(c, "cuda", q=qkv.cuda()), want, D, f"extend vs oracle S={S} D={D} G={G}")
    flash = ops.flash_attention_qkv(qkv.cuda(), 1, S, Hq, HK, D, causal=True).reshape(S, Hq * D)
    _check_rows(flash, want, D, f"flash vs oracle S={S} D={D} G={G}")


@gpu
def test_deterministic():
    for page, D, G in ((48, 128, 8), (16, 64, 1)):
        c = _case(page, D, G)
        d = torch.device("cuda")
        dev = [c[k].to(d) for k in ("q", "k_cache", "v_cache", "table", "lens", "cu")]
        a = ops.paged_attention_extend(*dev, c["max_q"], c["Hq"], HK, D)
        b = ops.paged_attention_extend(*dev, c["max_q"], c["Hq"], HK, D)
        assert torch.equal(a, b)


@gpu
def test_unsupported_shape_takes_reference_on_gpu():
    c = _case(16, 96, 2)
    _check_rows(_run(c, "cuda"), _want(16, 96, 2), 96, "gpu reference D=96")
