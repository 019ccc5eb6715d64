"""Split-KV in the gfx950 paged extend attention (``ops.paged_attention_extend(num_splits=...)``):
every row tile's keys spread over ``num_splits`` workgroups and merged in a fixed order.

Construction, oracle, metric and bound are those of test_attention_extend_gpu.py, imported from
it: NaN-filled caches, shuffled blocks, table padding at an all-NaN block, two spiked keys per
sequence, a float64 oracle per (token, head) row, ``_row_err`` under ``ROW_BOUND`` = 2**-7.

The batch ``SPLIT_SEQS`` (prior, new): (130, 129) gives two row tiles at G = 1 and more at G = 8,
each with its own causal bound (so its own split size); (1023, 8) crosses a key-tile edge inside
the chunk; ``num_splits`` = 16 exceeds the key-tile count of most rows (empty splits), 3 splits
unevenly.

Teeth (CPU, ``test_split_cases_have_teeth``): both off-by-one causal masks move the oracle by
>= 4 * ROW_BOUND in every sequence with at least 2 new tokens: 5 of the batch's 8 sequences, 10
(sequence, direction) checks. Of the other three, (64, 0) has no rows, and (0, 1) and (17, 1) have
no key past their only position, so ``key <= p + 1`` is their true mask (the existing file's
exemption); their ``key <= p - 1`` checks are made too (2 more).

Worst rows measured on one MI355X are recorded in profiles/speculative_decoding.md.
"""
import pytest
import torch

from ray_community_amd import ops
from test_attention_extend_gpu import HK, ROW_BOUND, _case, _check_rows, _oracle, _row_err, _want

gpu = pytest.mark.gpu

SPLIT_SEQS = ((0, 1), (63, 2), (64, 5), (200, 5), (1023, 8), (130, 129), (64, 0), (17, 1))
SEED = 3
SHAPES = [(page, D, G) for page in (16, 64) for D in (64, 128) for G in (1, 4, 8)]


def _run(c, device, q=None, **kw):
    d = torch.device(device)
    q = c["q"].to(d) if q is None else q
    return ops.paged_attention_extend(q, c["k_cache"].to(d), c["v_cache"].to(d), c["table"].to(d), c["lens"].to(d),
                                      c["cu"].to(d), c["max_q"], c["Hq"], HK, c["D"], **kw)


def test_split_cases_have_teeth():
    checked = 0
    for page, D, G in SHAPES:
        c, want = _case(page, D, G, SPLIT_SEQS, SEED), _want(page, D, G, SPLIT_SEQS, SEED)
        cu = c["cu"].tolist()
        for sh in (+1, -1):
            err = _row_err(_oracle(c, shift=sh), want, D)
            for b, (_, n) in enumerate(SPLIT_SEQS):
                if n == 0:
                    continue
                worst = err[cu[b]: cu[b + 1]].max().item()
                if n == 1 and sh == +1:
                    assert worst == 0.0  # no key past the only position
                    continue
                assert worst >= 4 * ROW_BOUND, (page, D, G, b, sh, worst)
                checked += 1
    assert checked == len(SHAPES) * 12  # 10 checks of the 5 sequences with >= 2 new tokens, 2 of the others


def test_num_splits_below_one_raises():
    c = _case(16, 64, 1, SPLIT_SEQS, SEED)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            _run(c, "cpu", num_splits=bad)


def test_reference_ignores_num_splits_cpu():
    c = _case(16, 64, 4, SPLIT_SEQS, SEED)
    assert torch.equal(_run(c, "cpu", num_splits=4), _run(c, "cpu"))
    assert torch.equal(_run(c, "cpu", num_splits=None), _run(c, "cpu"))


@gpu
@pytest.mark.parametrize("num_splits", [2, 3, 16])
@pytest.mark.parametrize("page,D,G", SHAPES)
def test_split_shape_matrix(page, D, G, num_splits):
    c = _case(page, D, G, SPLIT_SEQS, SEED)
    _check_rows(_run(c, "cuda", num_splits=num_splits), _want(page, D, G, SPLIT_SEQS, SEED), D,
                f"split={num_splits} page={page} D={D} G={G}")


@gpu
def test_one_split_is_the_unsplit_launch():
    for page, D, G in ((16, 128, 4), (64, 64, 8)):
        c = _case(page, D, G, SPLIT_SEQS, SEED)
        assert torch.equal(_run(c, "cuda", num_splits=1), _run(c, "cuda"))


@gpu
def test_split_deterministic():
    for page, D, G, ns in ((16, 128, 8, 3), (64, 64, 1, 16)):
        c = _case(page, D, G, SPLIT_SEQS, SEED)
        d = torch.device("cuda")
        dev = [c[k].to(d) for k in ("q", "k_cache", "v_cache", "table", "lens", "cu")]
        a = ops.paged_attention_extend(*dev, c["max_q"], c["Hq"], HK, D, num_splits=ns)
        b = ops.paged_attention_extend(*dev, c["max_q"], c["Hq"], HK, D, num_splits=ns)
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("D,G", [(64, 4), (128, 8)])
def test_split_inplace_q(D, G):
    c = _case(16, D, G, SPLIT_SEQS, SEED)
    Hq, T = c["Hq"], c["q"].shape[0]
    base = _run(c, "cuda", num_splits=3)
    fused = torch.randn(T, (Hq + 2 * HK) * D).to(torch.bfloat16).cuda()
    fused[:, : Hq * D] = c["q"].cuda()
    assert torch.equal(_run(c, "cuda", q=fused, num_splits=3), base)
    _check_rows(base, _want(16, D, G, SPLIT_SEQS, SEED), D, f"in-place split=3 D={D} G={G}")


@gpu
def test_split_heuristic_choice_matches_oracle():
    """``num_splits=None``: whatever the heuristic picks for this small batch is within the bound."""
    c = _case(16, 128, 4, SPLIT_SEQS, SEED)
    _check_rows(_run(c, "cuda", num_splits=None), _want(16, 128, 4, SPLIT_SEQS, SEED), 128, "split=None")


@gpu
def test_unsupported_shape_with_splits_takes_reference_on_gpu():
    c = _case(16, 96, 4, SPLIT_SEQS, SEED)
    out = _run(c, "cuda", num_splits=4)
    _check_rows(out, _want(16, 96, 4, SPLIT_SEQS, SEED), 96, "gpu reference D=96 split=4")
    assert torch.equal(out, _run(c, "cuda"))


@gpu
def test_num_splits_heuristic():
    assert ops.paged_extend_num_splits(4, 8, 512, 4, 4096, 16) == 1
    assert ops.paged_extend_num_splits(1, 8, 5, 4, 4096, 16) > 1
    for B in (1, 8, 32, 4096):
        for q in (1, 5, 512, 8192):
            for ctx in (1, 64, 4096, 1 << 20, 2 ** 31 - 1):
                for G in (1, 4, 8):
                    assert 1 <= ops.paged_extend_num_splits(B, 8, q, G, ctx, 16) <= 16
    assert "paged_extend_num_splits" in ops.__all__
