"""Edges of the gfx950 paged decode attention and KV-cache append (ops/csrc/attention_decode.hip),
checked per (sequence, head) against a float64 oracle written here, independent of ops/reference.py.

Metric: ``_row_err`` = max_d |out - want| / max_d |want| for every (sequence, head) row, so a long
row with small outputs is not hidden behind a short row with large ones. Bound: ``ROW_BOUND`` =
2**-7. Rounding an exact value to bf16 moves it by at most 2**-8 of its magnitude, hence by at most
2**-8 of its row's maximum; the fp32 dot products (64 or 128 terms), the fp32 online softmax and
the hardware exp2 are far below that, so the bound is the rounding floor times two. The floor is
measured on the oracle itself (rounded to bf16, scored against the unrounded one), never on the
kernel.

Every case is built once on the CPU and its oracle is computed once (``_case`` / ``_want`` are
cached). The tests without a ``gpu`` mark run anywhere and guard the test data: the oracle agrees
with the CPU fallback of ``ops.paged_attention_decode``, and every case that is meant to be
sensitive really is: dropping the last token of its longest sequence moves the oracle by at least
2 * ROW_BOUND, so the same slip in the kernel fails the GPU test.

Measured on one MI355X, worst ``_row_err`` over each test's cases (bound 7.81e-3, bf16 rounding
floor of the oracle 3.69e-3): per-row matrix 3.77e-3 (page 48, D 128, G 8); large logits 3.18e-3;
every tail length 3.42e-3; running max 3.23e-3 (rising scores, one split), and 0 against the spiked
token's own V row; default split policy (1024 tokens, 4 splits) 2.85e-3; append-then-decode round
trip 2.99e-3. The kernel sits on the rounding floor everywhere; no case came near the bound.
"""
import functools
import math

import pytest
import torch

from ray_community_amd import ops
from ray_community_amd.models.kv_cache import PagedKVCache

gpu = pytest.mark.gpu

ROW_BOUND = 2.0 ** -7
HK = 2
NAN = float("nan")


# ------------------------------------------------------------------------------ oracle and metric
def _attend(q, k, v, G, scale):
    """float64 attention of one token: q [Hq, D], k / v [n, Hk, D] -> [Hq, D]; kv head = h // G."""
    out = torch.zeros_like(q)
    for h in range(q.shape[0]):
        s = (k[:, h // G] @ q[h]) * scale
        p = torch.exp(s - s.max())
        out[h] = (p / p.sum()) @ v[:, h // G]
    return out


def _oracle(q, k_cache, v_cache, table, lens, Hq, Hk, D, scale):
    """Paged single-token attention in float64 on the CPU: token i of sequence b lives in slot
    table[b, i // page] * page + i % page. Returns [B, Hq*D]; zeros where the length is 0."""
    page = k_cache.shape[1]
    kf = k_cache.detach().cpu().double().reshape(-1, Hk, D)
    vf = v_cache.detach().cpu().double().reshape(-1, Hk, D)
    qf = q.detach().cpu().double()[:, : Hq * D].reshape(-1, Hq, D)
    table = table.tolist()
    lens = lens.tolist() if torch.is_tensor(lens) else list(lens)
    out = torch.zeros(len(lens), Hq, D, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        slots = [table[b][i // page] * page + i % page for i in range(n)]
        out[b] = _attend(qf[b], kf[slots], vf[slots], Hq // Hk, scale)
    return out.reshape(len(lens), Hq * D)


def _rows(t, D):
    t = t.detach().cpu().double()
    return t.reshape(t.shape[0], -1, D)


def _row_err(out, want, D):
    """[B, Hq] tensor of max_d |out - want| / max_d |want|. Rows whose ``want`` is all zero are
    skipped (reported as 0): they must be asserted exactly zero separately."""
    a, b = _rows(out, D), _rows(want, D)
    num, den = (a - b).abs().amax(-1), b.abs().amax(-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))


def _check_rows(out, want, D, label):
    """The assertion every comparison below makes: bf16, finite, all-zero rows of ``want`` exactly
    zero, and every other row within ROW_BOUND. Prints and returns the worst row error."""
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == tuple(want.shape)
    assert torch.isfinite(out).all()
    dead = _rows(want, D).abs().amax(-1) == 0
    assert (_rows(out, D)[dead] == 0).all()
    worst = _row_err(out, want, D).max().item()
    print(f"{label}: max row err {worst:.3e} (bound {ROW_BOUND:.3e})")
    assert worst < ROW_BOUND
    return worst


# ------------------------------------------------------------------------------------ case data
def _paged(Ks, Vs, page, perm, width=None):
    """Lay logical per-sequence K / V ([n, HK, D] bf16 each) out in caches that are NaN everywhere
    except the live slots, taking physical blocks in the order ``perm``. Unused block-table entries
    hold the id of a valid block that stays all NaN, so reading one poisons the output."""
    D = Ks[0].shape[-1]
    need = [-(-k.shape[0] // page) for k in Ks]
    assert len(perm) > sum(need)
    pad = perm[sum(need)]
    table = torch.full((len(Ks), max(need + [1]) if width is None else width), pad, dtype=torch.int32)
    k_cache = torch.full((len(perm), page, HK, D), NAN, dtype=torch.bfloat16)
    v_cache = torch.full((len(perm), page, HK, D), NAN, dtype=torch.bfloat16)
    nxt = 0
    for b, (k, v) in enumerate(zip(Ks, Vs)):
        blocks = perm[nxt: nxt + need[b]]
        nxt += need[b]
        table[b, : need[b]] = torch.tensor(blocks, dtype=torch.int32)
        slots = torch.tensor([blocks[i // page] * page + i % page for i in range(k.shape[0])], dtype=torch.long)
        k_cache.view(-1, HK, D)[slots] = k
        v_cache.view(-1, HK, D)[slots] = v
    assert torch.isnan(k_cache[pad]).all() and torch.isnan(v_cache[pad]).all()
    return k_cache, v_cache, table


def _pack(q, Ks, Vs, page, perm, D, G, sensitive, width=None):
    k_cache, v_cache, table = _paged(Ks, Vs, page, perm, width)
    return dict(q=q, k=k_cache, v=v_cache, table=table, lens=[k.shape[0] for k in Ks], Hq=HK * G, D=D, G=G, page=page,
                Ks=Ks, Vs=Vs, sensitive=sensitive)


# seed 1000*page + 10*D + G fails the sensitivity condition here (1.9 x ROW_BOUND): reseeded (7.2 x)
RESEEDED = {(32, 64, 1): 32642}


def _matrix_case(page, D, G, q_mul=1.0):
    """The construction of tests/test_attention_decode_gpu.py::_case with its seeds and draw order:
    lengths [0, 1, page-1, page, page+1, 5*page+3], random K / V / fused qkv row (q leads)."""
    lens = [0, 1, page - 1, page, page + 1, 5 * page + 3]
    num_blocks = sum(-(-n // page) for n in lens) + 5
    g = torch.Generator().manual_seed(RESEEDED.get((page, D, G), 1000 * page + 10 * D + G))
    perm = torch.randperm(num_blocks, generator=g).tolist()
    Ks, Vs = [], []
    for n in lens:
        kv = [torch.randn(HK, D, generator=g) for _ in range(2 * n)]  # k, v, k, v, ... per token
        Ks.append(torch.stack(kv[0::2]).bfloat16() if n else torch.zeros(0, HK, D, dtype=torch.bfloat16))
        Vs.append(torch.stack(kv[1::2]).bfloat16() if n else torch.zeros(0, HK, D, dtype=torch.bfloat16))
    qkv = torch.randn(len(lens), (HK * G + 2 * HK) * D, generator=g)
    qkv[:, : HK * G * D] *= q_mul
    # q scaled by 8 makes the softmax nearly one-hot: such a case is blind to dropped tokens (they
    # carry no weight) and is exempt from the sensitivity condition
    return _pack(qkv.bfloat16(), Ks, Vs, page, perm, D, G, sensitive=q_mul == 1.0)


def _tail_case(page, D):
    """One sequence for every length 0 .. 2*page+17, q = 0 (every live token weighs 1/n) and
    V[i, :, d] = [d == i % D]: out[b, h, d] = #{i < n : i % D == d} / n exactly."""
    G = 2
    lens = list(range(2 * page + 18))
    g = torch.Generator().manual_seed(77 * page + D)
    Ks = [torch.randn(n, HK, D, generator=g).bfloat16() for n in lens]
    Vs = []
    for n in lens:
        v = torch.zeros(n, HK, D)
        v[torch.arange(n), :, torch.arange(n) % D] = 1.0
        Vs.append(v.bfloat16())
    perm = torch.randperm(sum(-(-n // page) for n in lens) + 3, generator=g).tolist()
    c = _pack(torch.zeros(len(lens), HK * G * D, dtype=torch.bfloat16), Ks, Vs, page, perm, D, G, sensitive=True)
    want = torch.zeros(len(lens), HK * G, D, dtype=torch.float64)
    for n in lens[1:]:
        want[n] = torch.bincount(torch.arange(n) % D, minlength=D).double() / n
    c["closed_form"] = want.reshape(len(lens), -1)
    return c


RM_TOKENS, RM_SLOPE, RM_SPIKE = 640, 0.05, 30.0
RM_POSITIONS = (0, 15, 16, 63, 64, 639)


def _rm_scores(kind, pos):
    """Designed score (natural units, before the per-head factor) of each of the 640 tokens."""
    i = torch.arange(RM_TOKENS, dtype=torch.float64)
    if kind == "up":
        return RM_SLOPE * i
    if kind == "down":
        return RM_SLOPE * (RM_TOKENS - 1 - i)
    s = torch.ones(RM_TOKENS, dtype=torch.float64)
    s[pos] += RM_SPIKE
    return s


def _running_max_case(D, G, kind, pos=None):
    """One sequence of 40 pages of 16 whose scores are designed, not random: q[h] = c_h * ones(D)
    with c_h in {1, 1.125, 1.25, 1.375} and every K row a (coarse, residual) bf16 pair repeated D/2
    times, so q.k * scale reproduces ``_rm_scores`` to about 2**-16 relative in every head."""
    x = _rm_scores(kind, pos) * math.sqrt(D) / (D // 2)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.double()).to(torch.bfloat16)
    k = torch.empty(RM_TOKENS, D, dtype=torch.bfloat16)
    k[:, 0::2], k[:, 1::2] = hi[:, None], lo[:, None]
    g = torch.Generator().manual_seed(31 * D + G)
    v = torch.randn(RM_TOKENS, HK, D, generator=g).bfloat16()
    q = (1.0 + (torch.arange(HK * G) % 4) / 8.0)[:, None].expand(HK * G, D).reshape(1, -1).bfloat16()
    perm = torch.randperm(RM_TOKENS // 16 + 2, generator=g).tolist()
    # only a rising score, or a spike on the last token, gives the last token any weight
    return _pack(q, [k[:, None, :].expand(-1, HK, -1).contiguous()], [v], 16, perm, D, G,
                 sensitive=kind == "up" or pos == RM_TOKENS - 1)


def _split_case():
    """B = 2, lens [1024, 37], page 16, table width 64: the default policy gives 4 splits."""
    D, G, lens = 128, 4, [1024, 37]
    g = torch.Generator().manual_seed(4)
    Ks = [torch.randn(n, HK, D, generator=g).bfloat16() for n in lens]
    Vs = [torch.randn(n, HK, D, generator=g).bfloat16() for n in lens]
    q = torch.randn(2, (HK * G + 2 * HK) * D, generator=g).bfloat16()
    perm = torch.randperm(64 + 3 + 4, generator=g).tolist()
    return _pack(q, Ks, Vs, 16, perm, D, G, sensitive=True, width=64)


PAGES, DS, GS = (16, 32, 48, 64), (64, 128), (1, 2, 4, 8)
RM_KINDS = [("up", None), ("down", None)] + [("spike", p) for p in RM_POSITIONS]
CASES = {f"matrix-{p}-{D}-{G}": functools.partial(_matrix_case, p, D, G) for p in PAGES for D in DS for G in GS}
CASES["large-logits-16-128-4"] = functools.partial(_matrix_case, 16, 128, 4, 8.0)
CASES.update({f"tail-{p}-{D}": functools.partial(_tail_case, p, D) for p in (16, 48) for D in DS})
CASES.update({f"runmax-{D}-{G}-{kind}{'' if pos is None else pos}": functools.partial(_running_max_case, D, G, kind, pos)
              for D, G in ((128, 4), (64, 8)) for kind, pos in RM_KINDS})
CASES["split-1024"] = _split_case


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


def _scale(c):
    return c["D"] ** -0.5


@functools.lru_cache(maxsize=None)
def _want(name):
    """The float64 oracle of a case, computed once and shared."""
    c = _case(name)
    return _oracle(c["q"], c["k"], c["v"], c["table"], c["lens"], c["Hq"], HK, c["D"], _scale(c))


def _want_without_last(name):
    """Oracle rows of the longest sequence of a case, in full and with its last token removed."""
    c = _case(name)
    b = max(range(len(c["lens"])), key=lambda i: c["lens"][i])
    short = _oracle(c["q"][b: b + 1], c["k"], c["v"], c["table"][b: b + 1], [c["lens"][b] - 1], c["Hq"], HK, c["D"],
                    _scale(c))
    return b, _want(name)[b: b + 1], short


def _run(c, device="cuda", **kw):
    lens = torch.tensor(c["lens"], dtype=torch.int32)
    t = [x.to(device) for x in (c["q"], c["k"], c["v"], c["table"], lens)]
    if device == "cuda":
        assert ops.paged_decode_supported(c["page"], c["D"], c["Hq"], HK)  # the kernel, not the fallback
    out = ops.paged_attention_decode(*t, c["Hq"], HK, c["D"], **kw)
    if device == "cuda":
        torch.cuda.synchronize()
    return out.cpu()


# --------------------------------------------------------------- CPU tests: guard the test data
def test_bound_is_twice_the_bf16_rounding_floor():
    """The reference for ROW_BOUND: the oracle rounded to bf16 against itself is within 2**-8."""
    worst = 0.0
    for name in ("matrix-16-128-4", "matrix-64-64-1", "split-1024", "runmax-128-4-up"):
        w = _want(name)
        worst = max(worst, _row_err(w.bfloat16(), w, _case(name)["D"]).max().item())
    print(f"bf16 rounding floor {worst:.3e}")
    assert 0 < worst <= 2.0 ** -8 and ROW_BOUND == 2 * 2.0 ** -8


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_cpu_fallback(name):
    c = _case(name)
    out = _run(c, device="cpu")
    _check_rows(out, _want(name).bfloat16(), c["D"], f"fallback {name}")
    assert (out[[i for i, n in enumerate(c["lens"]) if n == 0]] == 0).all()


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("tail")))
def test_tail_oracle_is_the_closed_form(name):
    assert (_want(name) - _case(name)["closed_form"]).abs().max().item() < 1e-12


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("runmax")))
def test_running_max_scores_are_as_designed(name):
    """From the bf16 K and q actually used: strictly monotone, or flat with one spike of >= 30."""
    c = _case(name)
    for h in range(c["Hq"]):
        s = (c["Ks"][0][:, h // c["G"]].double() @ c["q"].double().reshape(c["Hq"], c["D"])[h]) * _scale(c)
        d = s[1:] - s[:-1]
        if "-up" in name:
            assert (d > 0.04).all() and (d < 0.08).all()
        elif "-down" in name:
            assert (d < -0.04).all() and (d > -0.08).all()
        else:
            pos = int(name.rsplit("spike", 1)[1])
            rest = torch.cat([s[:pos], s[pos + 1:]])
            assert rest.max() - rest.min() < 1e-3 and s[pos] - rest.max() >= RM_SPIKE - 1e-3


SENSITIVE = sorted(n for n in CASES if not n.startswith(("large-logits", "runmax")))
SENSITIVE += ["runmax-128-4-up", "runmax-64-8-up", "runmax-128-4-spike639", "runmax-64-8-spike639"]


@pytest.mark.parametrize("name", SENSITIVE)
def test_cases_are_sensitive_to_a_dropped_token(name):
    """Removing the last token of the longest sequence moves the oracle by >= 2 * ROW_BOUND in that
    sequence, so a kernel that loses it cannot pass. Large-logits cases are exempt: their softmax is
    nearly one-hot and blind to dropped tokens; so are the falling and early-spike score designs."""
    c = _case(name)
    assert c["sensitive"]
    _, full, short = _want_without_last(name)
    r = _row_err(short, full, c["D"]).max().item()
    print(f"{name}: dropped last token moves the oracle by {r:.3e} = {r / ROW_BOUND:.1f} x ROW_BOUND")
    assert r >= 2 * ROW_BOUND


def test_insensitive_cases_are_marked():
    blind = [n for n in CASES if not _case(n)["sensitive"]]
    assert sorted(blind) == sorted(set(CASES) - set(SENSITIVE))


@pytest.mark.parametrize("name", ["matrix-16-128-4", "matrix-64-64-1", "tail-48-64", "runmax-128-4-up",
                                  "runmax-64-8-spike639", "split-1024"])
def test_check_rejects_a_dropped_token(name):
    """The drop-last oracle, rounded to bf16, standing in for the op's output fails ``_check_rows``."""
    c = _case(name)
    b, _, short = _want_without_last(name)
    fake = _want(name).clone()
    fake[b] = short[0]
    with pytest.raises(AssertionError):
        _check_rows(fake.bfloat16(), c.get("closed_form", _want(name)), c["D"], f"dropped {name}")
    _check_rows(_want(name).bfloat16(), c.get("closed_form", _want(name)), c["D"], f"intact {name}")


# ---------------------------------------------------------------------- 10. append, then decode
class _Cfg:
    num_layers, num_kv_heads, head_dim = 1, HK, 128


RT_LENS = [1, 33, 80]
RT_CHUNKS = [(0, 1), (1, 7), (2, 20), (1, 16), (2, 30), (1, 10), (2, 30)]  # (sequence, tokens), interleaved


def _dense(q, Ks, Vs, G, scale):
    """float64 attention over the original, never-paged K / V of every sequence."""
    Hq = HK * G
    return torch.stack([_attend(q[b].double().reshape(Hq, -1), k.double(), v.double(), G, scale)
                        for b, (k, v) in enumerate(zip(Ks, Vs))]).reshape(len(Ks), -1)


@functools.lru_cache(maxsize=None)
def _round_trip_data():
    G, D = 4, _Cfg.head_dim
    g = torch.Generator().manual_seed(10)
    Ks = [torch.randn(n, HK, D, generator=g).bfloat16() for n in RT_LENS]
    Vs = [torch.randn(n, HK, D, generator=g).bfloat16() for n in RT_LENS]
    q = torch.randn(len(RT_LENS), HK * G * D, generator=g).bfloat16()
    return G, D, q, Ks, Vs, _dense(q, Ks, Vs, G, D ** -0.5)


def _round_trip(device):
    """Grow three sequences in interleaved chunks through PagedKVCache.allocate, writing every chunk
    with ops.kv_cache_append_, then decode with the cache's own block table and lengths."""
    G, D, q, Ks, Vs, _ = _round_trip_data()
    Hq = HK * G
    cache = PagedKVCache(_Cfg, num_blocks=12, page_size=16, device=device)
    cache.k[0].fill_(NAN)
    cache.v[0].fill_(NAN)
    done = [0] * len(RT_LENS)
    for s, t in RT_CHUNKS:
        slots = torch.tensor(cache.allocate(s, t), dtype=torch.int32, device=device)
        rows = torch.cat([torch.full((t, Hq * D), NAN, dtype=torch.bfloat16),  # the q columns are not the append's
                          Ks[s][done[s]: done[s] + t].reshape(t, -1), Vs[s][done[s]: done[s] + t].reshape(t, -1)], 1)
        ops.kv_cache_append_(cache.k[0], cache.v[0], rows.to(device), slots, Hq, HK, D)
        done[s] += t
    assert done == RT_LENS
    ids = list(range(len(RT_LENS)))
    table, lens = cache.block_table(ids), cache.context_lens(ids)
    assert lens.tolist() == RT_LENS
    long_row = table[2, :5].tolist()
    assert long_row != list(range(long_row[0], long_row[0] + 5))  # the blocks of a sequence interleave with others'
    return ops.paged_attention_decode(q.to(device), cache.k[0], cache.v[0], table, lens, Hq, HK, D).cpu()


def test_round_trip_on_the_cpu_fallback():
    G, D, q, Ks, Vs, want = _round_trip_data()
    _check_rows(_round_trip("cpu"), want.bfloat16(), D, "round trip, fallback")
    short = _dense(q, Ks[:2] + [Ks[2][:-1]], Vs[:2] + [Vs[2][:-1]], G, D ** -0.5)
    r = _row_err(short, want, D)[2].max().item()
    print(f"round trip: dropped last token moves the oracle by {r:.3e} = {r / ROW_BOUND:.1f} x ROW_BOUND")
    assert r >= 2 * ROW_BOUND
    with pytest.raises(AssertionError):
        _check_rows(short.bfloat16(), want, D, "round trip, dropped")


@gpu
def test_append_then_decode_round_trip():
    _, D, _, _, _, want = _round_trip_data()
    assert ops.paged_decode_supported(16, D, HK * 4, HK)
    _check_rows(_round_trip("cuda"), want, D, "round trip")


# ------------------------------------------------------------------------------------ GPU tests
@gpu
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("page", PAGES)
def test_matrix_per_row(page, D, G):
    name = f"matrix-{page}-{D}-{G}"
    _check_rows(_run(_case(name)), _want(name), D, name)


@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
def test_large_logits_per_row(num_splits):
    name = "large-logits-16-128-4"
    _check_rows(_run(_case(name), num_splits=num_splits), _want(name), 128, f"{name} splits={num_splits}")


@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("page", [16, 48])
def test_every_tail_length_exact(page, D, num_splits):
    """Every ``live`` in 1..16 on a first, second and third page; a lost or doubled token changes a
    column by 1/n."""
    c = _case(f"tail-{page}-{D}")
    out = _run(c, num_splits=num_splits)
    _check_rows(out, c["closed_form"], D, f"tail-{page}-{D} splits={num_splits}")
    assert (out[0] == 0).all()


@gpu
@pytest.mark.parametrize("kind,pos", RM_KINDS)
@pytest.mark.parametrize("D,G", [(128, 4), (64, 8)])
def test_running_max_under_control(D, G, kind, pos):
    """640 tokens: with one split every wave loops 10 times and the running max moves on every step
    (up), on none after the first (down), or once, at a chosen token (spike). 41 splits leave one
    empty."""
    name = f"runmax-{D}-{G}-{kind}{'' if pos is None else pos}"
    c = _case(name)
    for num_splits in (1, 3, 40, 41):
        out = _run(c, num_splits=num_splits)
        _check_rows(out, _want(name), D, f"{name} splits={num_splits}")
        if kind == "spike":
            v_row = c["Vs"][0][pos].double().repeat_interleave(G, dim=0).reshape(1, -1)  # [1, Hq*D]
            _check_rows(out, v_row, D, f"{name} splits={num_splits} vs V[{pos}]")


@gpu
def test_default_split_policy_splits():
    c = _case("split-1024")
    assert c["table"].shape == (2, 64)
    assert ops.lib().rca_attn_decode_num_splits(2, HK, 1024, 16) == 4
    a = _run(c, num_splits=None)
    _check_rows(a, _want("split-1024"), c["D"], "split-1024 default splits")  # the 37-token row: 3 pages, 4 splits
    assert torch.equal(a, _run(c, num_splits=None))


@gpu
def test_num_splits_policy_properties():
    """Host function only: nothing is launched."""
    f = ops.lib().rca_attn_decode_num_splits
    bases = [(1, 1), (1, 2), (2, 2), (1, 8), (8, 8), (32, 8), (64, 8), (128, 8), (1024, 8), (65535, 64)]
    ctxs = [1, 15, 16, 17, 63, 64, 255, 256, 257, 511, 512, 1000, 1024, 4096, 8191, 8192, 65536, 2 ** 31 - 1]
    for page in (16, 32, 48, 64, 128, 1024):
        floor = 2 * max(4, -(-256 // page))
        last_base = None
        for B, Hk in sorted(bases, key=lambda t: t[0] * t[1]):
            row = [f(B, Hk, ctx, page) for ctx in ctxs]
            assert all(1 <= n <= 16 for n in row)
            assert all(n == 1 for n, ctx in zip(row, ctxs) if -(-ctx // page) < floor)
            assert row == sorted(row)  # non-decreasing in the context
            assert last_base is None or all(n <= m for n, m in zip(row, last_base))  # non-increasing in B * Hk
            last_base = row
    assert f(1, 1, 2 ** 31 - 1, 16) == 16 and f(2, 2, 1024, 16) > 1
    for bad in ((0, 8, 4096, 16), (8, 0, 4096, 16), (8, 8, 0, 16), (8, 8, 4096, 0), (-1, 8, 4096, 16),
                (8, -3, 4096, 16), (8, 8, -4096, 16), (8, 8, 4096, -16)):
        assert f(*bad) == 1


# -------------------------------------------------------------------- 8. metamorphic, bitwise
META = ["matrix-16-128-4", "matrix-48-64-8"]


@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("name", META)
def test_physical_block_order_does_not_matter(name, num_splits):
    c = _case(name)
    g = torch.Generator().manual_seed(99)
    perm = torch.randperm(c["k"].shape[0] + 7, generator=g).tolist()
    k2, v2, t2 = _paged(c["Ks"], c["Vs"], c["page"], perm)
    assert not torch.equal(t2, c["table"])
    assert torch.equal(_run(c, num_splits=num_splits), _run(dict(c, k=k2, v=v2, table=t2), num_splits=num_splits))


@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("name", META)
def test_a_sequence_alone_equals_its_batched_row(name, num_splits):
    c = _case(name)
    batched = _run(c, num_splits=num_splits)
    for b, n in enumerate(c["lens"]):
        alone = _run(dict(c, q=c["q"][b: b + 1], table=c["table"][b: b + 1], lens=[n]), num_splits=num_splits)
        assert torch.equal(alone[0], batched[b]), f"sequence {b} (length {n})"


@gpu
@pytest.mark.parametrize("num_splits", [1, 3])
def test_equal_queries_in_a_kv_group_give_equal_rows(num_splits):
    c = _case("matrix-16-128-4")
    G, D, Hq = 4, 128, c["Hq"]
    q = c["q"].clone()
    heads = q[:, : Hq * D].view(-1, HK, G, D)  # every head of a kv group gets the group's first q row
    heads[:] = heads[:, :, :1].clone()
    out = _run(dict(c, q=q), num_splits=num_splits).reshape(-1, HK, G, D)
    assert out[5].abs().max() > 0
    for g in range(1, G):
        assert torch.equal(out[:, :, g], out[:, :, 0])
    assert not torch.equal(out[:, 0], out[:, 1])


# ---------------------------------------------------------------------------- 9. append, wider
@gpu
@pytest.mark.parametrize("T", [1, 37, 300])
@pytest.mark.parametrize("D,G", [(64, 1), (64, 8), (128, 2)])
def test_kv_cache_append_strided_rows(D, G, T):
    Hq, page, num_blocks = HK * G, 16, 24
    W = (Hq + 2 * HK) * D
    g = torch.Generator().manual_seed(1000 * D + 10 * G + T)
    wide = torch.randn(T, W + 64, generator=g).bfloat16()
    slots = torch.randperm(num_blocks * page, generator=g)[:T].to(torch.int32)  # out of order, distinct
    if T > 1:
        slots[[0, 5, T - 1]] = -1
    skipped = int((slots < 0).sum())

    k_want = torch.full((num_blocks * page, HK * D), -7.0, dtype=torch.bfloat16)
    v_want = k_want.clone()
    for t in range(T):  # the plain copy, token by token
        s = int(slots[t])
        if s >= 0:
            k_want[s] = wide[t, 32 + Hq * D: 32 + (Hq + HK) * D]
            v_want[s] = wide[t, 32 + (Hq + HK) * D: 32 + W]

    qkv = wide.cuda()[:, 32: 32 + W]
    # the conditions under which ops.kv_cache_append_ takes the kernel and not the reference copy
    assert qkv.is_cuda and qkv.dtype == torch.bfloat16 and ops.paged_decode_supported(page, D, Hq, HK)
    assert qkv.stride(1) == 1 and qkv.stride(0) == W + 64 and qkv.stride(0) % 8 == 0 and qkv.data_ptr() % 16 == 0
    k = torch.full((num_blocks, page, HK, D), -7.0, dtype=torch.bfloat16, device="cuda")
    v = k.clone()
    ops.kv_cache_append_(k, v, qkv, slots.cuda(), Hq, HK, D)
    torch.cuda.synchronize()
    k, v = k.cpu().view(-1, HK * D), v.cpu().view(-1, HK * D)
    assert torch.equal(k, k_want) and torch.equal(v, v_want)
    written = torch.zeros(num_blocks * page, dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    assert int(written.sum()) == T - skipped
    assert (k[~written] == -7.0).all() and (v[~written] == -7.0).all()  # untouched slots keep the sentinel
    assert not (k[written] == -7.0).all(dim=1).any() and not (v[written] == -7.0).all(dim=1).any()
