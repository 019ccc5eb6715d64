"""Plain PyTorch fp32 references of every HIP op (numerics oracle for tests, CPU execution path)."""
from __future__ import annotations

import torch


def rms_norm_ref(x, w, eps=1e-5, residual=None):
    s = x if residual is None else (x.float() + residual.float()).to(x.dtype)
    sf = s.float()
    r = torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + eps)
    y = (sf * r).to(x.dtype).float() * w.float()
    return y.to(x.dtype), s


def swiglu_ref(gu):
    F = gu.shape[-1] // 2
    g, u = gu[..., :F].float(), gu[..., F:].float()
    return (torch.nn.functional.silu(g).to(gu.dtype).float() * u).to(gu.dtype)


def rope_cos_sin(max_pos: int, head_dim: int, theta: float = 500000.0, device=None):
    """[max_pos, head_dim/2, 2] float32 table of (cos, sin) for the rotate-half convention."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    cs = torch.stack([f.cos(), f.sin()], dim=-1).float()
    return cs.to(device) if device is not None else cs


def rope_ref(x, cs, positions):
    """x: [T, H, D] ; cs [max_pos, D/2, 2]; positions [T] -> rotated x (rotate-half convention)."""
    D = x.shape[-1]
    half = D // 2
    c = cs[positions, :, 0][:, None, :]
    s = cs[positions, :, 1][:, None, :]
    xf = x.float()
    a, b = xf[..., :half], xf[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1).to(x.dtype)


def cross_entropy_ref(logits, labels, ignore_index=-100, reduction="mean"):
    return torch.nn.functional.cross_entropy(logits.float(), labels, ignore_index=ignore_index, reduction=reduction)


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, grad_mul=1.0, clip=1.0):
    g = g.float() * grad_mul * clip
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    p.sub_(lr * ((m / bc1) / ((v / bc2).sqrt() + eps) + wd * p))
    return p


def split_master(master):
    """fp32 master -> (hi, lo): hi = the bit pattern rounded half-up in magnitude to 16 bits (a bf16
    tensor: the model weight; equal to RNE except at exact ties), lo = the low 16 bits (int16
    storage). ``join_master(hi, lo)`` reconstructs ``master`` bit-exactly (loss_optim.hip)."""
    M = master.float().contiguous().view(torch.int32)
    hi = ((M + 0x8000) >> 16) & 0xFFFF
    lo = M & 0xFFFF
    to16 = lambda x: (x - ((x >> 15) << 16)).to(torch.int16)  # 0..65535 -> same 16 bits as int16
    return to16(hi).view(torch.bfloat16), to16(lo)


def join_master(hi, lo):
    """Inverse of ``split_master``: the fp32 master from the bf16 weight and its low halves."""
    h = hi.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    l_ = lo.contiguous().to(torch.int32) & 0xFFFF
    up = h - (l_ >> 15)
    return ((up << 16) | l_).view(torch.float32)


def gae_ref(rewards, values, terminateds, dones, gamma, lam, last_values=None, next_values=None):
    """rewards/values/...: [B, T] -> (advantages, value_targets) in fp64-accurate float32."""
    B, T = rewards.shape
    r = rewards.double()
    v = values.double()
    adv = torch.zeros_like(r)
    for b in range(B):
        A = 0.0
        for t in range(T - 1, -1, -1):
            if next_values is not None:
                nv = float(next_values[b, t])
            elif t + 1 < T:
                nv = float(v[b, t + 1])
            else:
                nv = float(last_values[b]) if last_values is not None else 0.0
            d = float(r[b, t]) + gamma * (0.0 if terminateds[b, t] else nv) - float(v[b, t])
            c = gamma * lam * (0.0 if dones[b, t] else 1.0)
            A = d + c * A
            adv[b, t] = A
    return adv.float(), (adv + v).float()


def image_normalize_ref(u8, mean, std, dtype=torch.bfloat16):
    x = u8.float() / 255.0
    m = torch.tensor(mean, dtype=torch.float32).view(1, 1, 1, -1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 1, 1, -1)
    return ((x - m) / s).permute(0, 3, 1, 2).contiguous().to(dtype)


def crop_resize_normalize_ref(u8, boxes, flips, size, mean, std, dtype=torch.float32):
    """Per image: crop box (y0, x0, h, w) -> bilinear resize (align_corners=False) -> optional
    horizontal flip -> /255, mean/std. uint8 [N, H, W, C] -> [N, C, Ho, Wo]."""
    import torch.nn.functional as F

    outs = []
    m = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)
    for n in range(u8.shape[0]):
        y0, x0, h, w = (int(v) for v in boxes[n])
        crop = u8[n, y0:y0 + h, x0:x0 + w, :].float().permute(2, 0, 1)[None]
        r = F.interpolate(crop, size=tuple(size), mode="bilinear", align_corners=False, antialias=False)[0]
        if flips is not None and bool(flips[n]):
            r = r.flip(-1)
        outs.append((r / 255.0 - m) / s)
    return torch.stack(outs).to(dtype)


def attention_ref(q, k, v, causal: bool = True, scale=None):
    """fp32 attention on ``[B, S, H, D]`` tensors (GQA by head repetition); returns q's dtype."""
    B, S, Hq, D = q.shape
    Hk = k.shape[2]
    scale = D ** -0.5 if scale is None else scale
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    if Hk != Hq:
        kf = kf.repeat_interleave(Hq // Hk, dim=1)
        vf = vf.repeat_interleave(Hq // Hk, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        m = torch.ones(S, k.shape[1], dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(m, float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), vf)
    return o.transpose(1, 2).to(q.dtype)


def vtrace_ref(log_rhos, rewards, values, next_values, terminateds, dones, gamma=0.99, clip_rho=1.0, clip_c=1.0,
               clip_pg=1.0):
    """Sequential fp32 V-trace (see ops/csrc/rl_data.hip vtrace_kernel for the recurrences)."""
    lr, r, v, nv = (torch.as_tensor(x, dtype=torch.float32) for x in (log_rhos, rewards, values, next_values))
    term = torch.as_tensor(terminateds).bool()
    done = torch.as_tensor(dones).bool()
    B, T = r.shape
    ir = lr.exp()
    rho, c, rpg = ir.clamp(max=clip_rho), ir.clamp(max=clip_c), ir.clamp(max=clip_pg)
    disc = gamma * (~term).float()
    vs = torch.zeros(B, T)
    pg = torch.zeros(B, T)
    acc = torch.zeros(B)
    for t in range(T - 1, -1, -1):
        cut = done[:, t] | (t + 1 >= T)
        vnext_in = v[:, t + 1] + acc if t + 1 < T else nv[:, t]
        vs_next = torch.where(cut, nv[:, t], vnext_in)
        d = rho[:, t] * (r[:, t] + disc[:, t] * nv[:, t] - v[:, t])
        k = gamma * c[:, t] * (~done[:, t]).float()
        acc = d + k * acc
        vs[:, t] = v[:, t] + acc
        pg[:, t] = rpg[:, t] * (r[:, t] + disc[:, t] * vs_next - v[:, t])
    return vs, pg


FP8_MAX = 448.0  # largest finite OCP e4m3 (torch.float8_e4m3fn) value


def kv_quantize_fp8_ref(x):
    """Quantise rows ``x[..., D]`` for the fp8 KV cache: returns ``(fp8 [..., D] float8_e4m3fn,
    scale [...] float32)``. The scale of a row is the smallest power of two ``s`` with
    ``max|x| / s <= 448``, clamped to ``[2^-126, 2^127]``, and 1 for an all-zero row; the stored
    element is the round-to-nearest-even e4m3 of ``x / s`` (an exact fp32 quotient of at most 448,
    so nothing saturates). Non-finite rows give unspecified values."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    mant, exp = torch.frexp(amax)  # amax = mant * 2^exp, mant in [0.5, 1); 448 = 0.875 * 2^9
    k = exp - 9 + (mant > 0.875).to(exp.dtype)
    k = torch.where(amax == 0, torch.zeros_like(k), k.clamp(-126, 127))
    scale = ((k + 127).to(torch.int32) << 23).view(torch.float32)
    return (xf / scale.unsqueeze(-1)).to(torch.float8_e4m3fn), scale


def kv_dequantize_fp8_ref(fp8, scale, dtype=torch.bfloat16):
    """``fp8 [..., D]`` times ``scale [...]`` in ``dtype``: exact in bf16 and fp32 (3 mantissa bits
    times a power of two) wherever the product is a normal number of ``dtype``."""
    return (fp8.float() * scale.unsqueeze(-1).float()).to(dtype)


def quantize_weight_fp8_ref(w):
    """Quantise a linear's weight ``[N, K]`` to fp8, one power-of-two scale per output row:
    ``kv_quantize_fp8_ref`` on the rows of ``w`` (a zero row gets scale 1). Returns ``(q [N, K]
    float8_e4m3fn, s [N] float32)``; ``kv_dequantize_fp8_ref(q, s)`` is exact in bf16 and fp32."""
    if w.dim() != 2:
        raise ValueError("quantize_weight_fp8_ref: weight must be [N, K]")
    return kv_quantize_fp8_ref(w)


def linear_w8_ref(x, qweight, scale):
    """``x [..., K] @ (qweight [N, K] * scale [N]).T`` with the weight dequantised (exactly) to
    ``x.dtype``: the reference of ``ops.linear_w8``."""
    if qweight.dtype == torch.uint8:
        qweight = qweight.view(torch.float8_e4m3fn)
    return torch.nn.functional.linear(x, kv_dequantize_fp8_ref(qweight, scale, x.dtype))


def lora_add_ref(y, x, A, B, scale, idx):
    """Per-row LoRA update, in place on ``y [M, N]``: with ``a = idx[m] >= 0`` the adapter slot of row
    ``m`` (``A [S, R, K]``, ``B [S, N, R]``, ``scale [S]`` fp32),

        t[m, :] = bf16(sum_k A[a, :, k] * x[m, k])
        y[m, n] = y.dtype(float(y[m, n]) + scale[a] * sum_r B[a, n, r] * t[m, r])

    both sums in fp32. A row with ``idx[m] < 0`` is not touched. The contract of ``ops.lora_add_``
    and its path for CPU tensors, other dtypes and shapes outside the kernel's contract."""
    idx = idx.reshape(-1).long()
    for s in torch.unique(idx[idx >= 0]).tolist():
        rows = (idx == s).nonzero().reshape(-1).to(y.device)
        t = (x[rows].float() @ A[s].float().t()).bfloat16().float()
        y[rows] = (y[rows].float() + scale[s].float() * (t @ B[s].float().t())).to(y.dtype)
    return y


def kv_cache_append_ref(k_cache, v_cache, qkv, slot_mapping, Hq, Hk, D, k_scale=None, v_scale=None):
    """Copy the K and V heads of each token of the fused (already rotated) ``qkv``
    ``[T, (Hq+2Hk)*D]`` into the paged caches ``[num_blocks, page_size, Hk, D]`` at slot
    ``slot_mapping[t]`` (= block * page_size + offset); ``-1`` skips the token. In place. With
    ``k_scale`` / ``v_scale`` (``[num_blocks, page_size, Hk]`` fp32) the caches are fp8 and every
    head row is quantised by ``kv_quantize_fp8_ref``."""
    T = qkv.shape[0]
    keep = slot_mapping >= 0
    slots = slot_mapping[keep].long()
    k = qkv[:, Hq * D: (Hq + Hk) * D].reshape(T, Hk, D)[keep]
    v = qkv[:, (Hq + Hk) * D: (Hq + 2 * Hk) * D].reshape(T, Hk, D)[keep]
    if k_scale is not None:
        k8, ks = kv_quantize_fp8_ref(k)
        v8, vs = kv_quantize_fp8_ref(v)
        # float8 tensors have no indexed assignment everywhere: write their bytes
        k_cache.view(torch.uint8).view(-1, Hk, D)[slots] = k8.view(torch.uint8)
        v_cache.view(torch.uint8).view(-1, Hk, D)[slots] = v8.view(torch.uint8)
        k_scale.view(-1, Hk)[slots] = ks
        v_scale.view(-1, Hk)[slots] = vs
        return
    k_cache.view(-1, Hk, D)[slots] = k.to(k_cache.dtype)
    v_cache.view(-1, Hk, D)[slots] = v.to(v_cache.dtype)


def _dequantized_caches(q, k_cache, v_cache, k_scale, v_scale):
    """The fp8 caches as exact caches of ``q``'s dtype (fp32 for other dtypes than bf16). Dead
    slots may hold anything, NaN included: the callers never read them."""
    dtype = torch.bfloat16 if q.dtype == torch.bfloat16 else torch.float32
    return kv_dequantize_fp8_ref(k_cache, k_scale, dtype), kv_dequantize_fp8_ref(v_cache, v_scale, dtype)


def paged_attention_decode_ref(q, k_cache, v_cache, block_table, context_lens, Hq, Hk, D, scale=None, k_scale=None,
                               v_scale=None):
    """fp32 single-token attention over a paged cache: per sequence, gather its pages through
    ``block_table``, truncate to ``context_lens[b]`` tokens, softmax attention with GQA by head
    repetition. ``q`` is ``[B, >= Hq*D]`` (the q heads lead a fused qkv row). Returns
    ``[B, Hq*D]`` in ``q``'s dtype; a sequence of length 0 gives zeros. With ``k_scale`` /
    ``v_scale`` the caches are fp8 and are dequantised first."""
    if k_scale is not None:
        k_cache, v_cache = _dequantized_caches(q, k_cache, v_cache, k_scale, v_scale)
    B = q.shape[0]
    page = k_cache.shape[1]
    scale = float(D ** -0.5 if scale is None else scale)
    G = Hq // Hk
    out = torch.zeros(B, Hq * D, dtype=torch.float32, device=q.device)
    lens = context_lens.tolist()
    for b in range(B):
        n = int(lens[b])
        if n <= 0:
            continue
        blocks = block_table[b, : (n + page - 1) // page].long()
        k = k_cache[blocks].reshape(-1, Hk, D)[:n].float().repeat_interleave(G, dim=1)  # [n, Hq, D]
        v = v_cache[blocks].reshape(-1, Hk, D)[:n].float().repeat_interleave(G, dim=1)
        qb = q[b, : Hq * D].reshape(Hq, D).float()
        p = torch.softmax(torch.einsum("hd,nhd->hn", qb, k) * scale, dim=-1)
        out[b] = torch.einsum("hn,nhd->hd", p, v).reshape(Hq * D)
    return out.to(q.dtype)


def paged_attention_extend_ref(q, k_cache, v_cache, block_table, context_lens, cu_q_lens, Hq, Hk, D, scale=None,
                               k_scale=None, v_scale=None):
    """fp32 causal attention of a ragged batch of query chunks over a paged cache. Sequence ``b``
    owns rows ``cu_q_lens[b] .. cu_q_lens[b+1]-1`` of ``q`` (``[T, >= Hq*D]``); ``context_lens[b]``
    counts its cached tokens including these ``n_b``, so query ``i`` sits at position
    ``context_lens[b] - n_b + i`` and attends keys ``0 .. position``, gathered through
    ``block_table``. Returns ``[T, Hq*D]`` in ``q``'s dtype; a sequence with ``n_b = 0``
    contributes no rows, and rows no sequence owns are zero. With ``k_scale`` / ``v_scale`` the
    caches are fp8 and are dequantised first."""
    if k_scale is not None:
        k_cache, v_cache = _dequantized_caches(q, k_cache, v_cache, k_scale, v_scale)
    T = q.shape[0]
    page = k_cache.shape[1]
    scale = float(D ** -0.5 if scale is None else scale)
    G = Hq // Hk
    out = torch.zeros(T, Hq * D, dtype=torch.float32, device=q.device)
    lens = context_lens.tolist()
    cu = cu_q_lens.tolist()
    for b in range(len(lens)):
        q0, q1 = int(cu[b]), int(cu[b + 1])
        n, ctx = q1 - q0, int(lens[b])
        if n <= 0 or ctx <= 0:
            continue
        blocks = block_table[b, : (ctx + page - 1) // page].long()
        k = k_cache[blocks].reshape(-1, Hk, D)[:ctx].float().repeat_interleave(G, dim=1)  # [ctx, Hq, D]
        v = v_cache[blocks].reshape(-1, Hk, D)[:ctx].float().repeat_interleave(G, dim=1)
        qb = q[q0:q1, : Hq * D].reshape(n, Hq, D).float()
        s = torch.einsum("ihd,nhd->hin", qb, k) * scale
        pos = torch.arange(ctx - n, ctx, device=q.device)
        hidden = torch.arange(ctx, device=q.device)[None, :] > pos[:, None]  # [n, ctx]
        p = torch.softmax(s.masked_fill(hidden[None], float("-inf")), dim=-1)
        p = torch.nan_to_num(p)  # a query before position 0 sees nothing: zeros
        out[q0:q1] = torch.einsum("hin,nhd->ihd", p, v).reshape(n, Hq * D)
    return out.to(q.dtype)


# ------------------------------------------------------------------------------------ sampling
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit words: ``counter`` is four arrays,
    ``key`` two; returns the four output words."""
    import numpy as np

    mask = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & mask for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & mask for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & mask, (k1 + np.uint64(_PHILOX_W1)) & mask
    return c0, c1, c2, c3


def _u64_array(values):
    """``values`` (ints of any sign or size, a sequence or a tensor of them) as numpy uint64, mod 2**64."""
    import numpy as np

    if torch.is_tensor(values):
        values = values.detach().cpu().reshape(-1).tolist()
    return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in values], dtype=np.uint64)


def philox_uniforms(seeds, steps):
    """The sampler's random number per row, float64 ``[B]`` on the CPU: ``u = ((r >> 8) + 0.5) * 2**-24``
    with ``r`` word 0 of Philox4x32-10 at counter ``(step & 0xffffffff, step >> 32, 0, 0)`` and key
    ``(seed & 0xffffffff, (seed >> 32) & 0xffffffff)``. ``u`` lies strictly inside (0, 1) and depends
    on nothing but (seed, step). It has 25 significant bits, one more than fp32 holds (rounded to
    fp32 its top value would be 1.0), so it is kept, here and in the kernel, in float64, where it
    is exact."""
    import numpy as np

    seeds, steps = _u64_array(seeds), _u64_array(steps)
    zero = np.zeros_like(steps)
    r = philox4x32_10((steps, steps >> np.uint64(32), zero, zero), (seeds, seeds >> np.uint64(32)))[0]
    u = ((r >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return torch.from_numpy(u)


def _f32(v) -> float:
    """``v`` rounded to fp32 (the precision the sampler's per-row parameters travel in)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def sample_kept_ref(x, temperature, top_k, top_p, min_p):
    """One row of the sampler: the weights ``w = exp((x - max x) / temperature)`` (computed in fp32,
    returned as float64) and the boolean kept set under the tie-inclusive ``top_k`` / ``top_p`` /
    ``min_p`` filters of ``sample_logits_ref``. ``x``: 1-D logits; ``temperature > 0``."""
    x = x.detach().float().cpu()
    V = x.shape[0]
    w32 = torch.exp((x - x.max()) / torch.tensor(_f32(temperature), dtype=torch.float32))
    w = w32.double()
    keep = torch.ones(V, dtype=torch.bool)
    top_k = int(top_k)
    if 0 < top_k < V:
        keep &= x >= x.topk(top_k).values[-1]
    if _f32(top_p) < 1.0:
        # mass of the survivors strictly above each survivor, by distinct value
        vals, inv = torch.unique(x[keep], return_inverse=True)  # ascending
        mass = torch.zeros(vals.shape[0], dtype=torch.float64).index_add_(0, inv, w[keep])
        above = mass.flip(0).cumsum(0).flip(0) - mass
        ok = above[inv] < _f32(top_p) * mass.sum()
        keep[keep.clone()] = ok
    if _f32(min_p) > 0.0:
        keep &= w32 >= torch.tensor(_f32(min_p), dtype=torch.float32)
    return w, keep


def sample_logits_ref(logits, temperature, top_k, top_p, min_p, seeds, steps, uniforms=None):
    """Reference of ``ops.sample_logits``: next token per row of ``logits`` ``[B, V]``; every
    parameter is a sequence (or tensor) of ``B`` values. Returns int64 ``[B]`` on ``logits.device``.

    Per row, with logits ``x``: ``temperature == 0`` returns the lowest index attaining the maximum
    and ignores the rest. Otherwise ``w_i = exp((x_i - max x) / temperature)`` in fp32 from the
    stored logit, and a token is kept if it passes all of (each tie-inclusive, so the kept set
    does not depend on any ordering of equal logits):
      * ``top_k > 0``: ``x_i >=`` the ``top_k``-th largest value (0 or ``>= V``: all);
      * ``top_p < 1``: among the ``top_k`` survivors, with ``S_i`` the total ``w`` of survivors with
        ``x_j > x_i`` and ``W`` the survivors' total, ``S_i < top_p * W`` (the smallest prefix of
        the descending order reaching mass ``top_p``, plus ties);
      * ``min_p > 0``: ``w_i >= min_p`` (probability at least ``min_p`` times the maximum one).
    With ``C`` the total ``w`` of the kept set, the result is the smallest kept index, in
    vocabulary order, whose inclusive running sum of kept ``w`` exceeds ``u * C`` (the last kept
    index if rounding leaves none). ``u`` is ``uniforms[row]`` if given, else
    ``philox_uniforms(seeds, steps)[row]``. Everything after the ``exp`` is float64 here.
    Temperature, ``top_p`` and ``min_p`` are taken at fp32 precision. Rows with a NaN or without a
    finite logit are out of contract."""
    B, V = logits.shape
    if uniforms is None:
        uniforms = philox_uniforms(seeds, steps)
    u = torch.as_tensor(uniforms).detach().double().cpu().reshape(-1)
    x_all = logits.detach().float().cpu()
    temperature, top_k, top_p, min_p = (v.detach().cpu().tolist() if torch.is_tensor(v) else list(v)
                                         for v in (temperature, top_k, top_p, min_p))
    out = torch.empty(B, dtype=torch.int64)
    for b in range(B):
        x = x_all[b]
        if not temperature[b] > 0:
            out[b] = int(torch.nonzero(x == x.max())[0]) if V else 0
            continue
        w, keep = sample_kept_ref(x, temperature[b], top_k[b], top_p[b], min_p[b])
        w = w * keep
        run = w.cumsum(0)
        hit = torch.nonzero(keep & (run > u[b] * w.sum()))
        out[b] = int(hit[0]) if hit.numel() else int(torch.nonzero(keep)[-1])
    return out.to(logits.device)


def _host_ints(values):
    """``values`` (a sequence or a tensor of ints, any shape) as nested Python lists."""
    return values.detach().cpu().tolist() if torch.is_tensor(values) else [
        list(v) if isinstance(v, (list, tuple)) else v for v in values]


def penalize_logits_ref(logits, tokens, ranges, repetition, presence, frequency):
    """Reference of ``ops.penalize_logits``: fp32 ``[B, V]`` on ``logits.device``; every parameter
    is a sequence (or tensor) of ``B`` values, taken at fp32 precision.

    Row ``b`` has the history ``tokens[start:end]`` with ``(start, prompt_end, end) = ranges[b]``,
    of which ``tokens[prompt_end:end]`` were produced; ids outside ``[0, V)`` are ignored. With
    ``x`` the stored logit as fp32, ``seen_i`` "token ``i`` occurs in the history" and ``c_i`` its
    number of occurrences among the produced tokens, each step one IEEE fp32 operation:
      1. ``y = x``; if ``seen_i``: ``y = x * (fp32(1) / fp32(repetition))`` if ``x > 0`` else ``x * repetition``;
      2. ``y = y - frequency * float(c_i)`` (the product rounded, then the difference);
      3. if ``c_i > 0``: ``y = y - presence``.
    A token outside the history keeps the exact fp32 image of its logit, and so does every token
    of a row with neutral parameters (1, 0, 0)."""
    B, V = logits.shape
    x_all = logits.detach().float().cpu()
    tokens = torch.as_tensor(_host_ints(tokens), dtype=torch.long).reshape(-1)
    ranges = _host_ints(ranges)
    repetition, presence, frequency = (v.detach().cpu().tolist() if torch.is_tensor(v) else list(v)
                                       for v in (repetition, presence, frequency))
    out = torch.empty(B, V, dtype=torch.float32)
    one = torch.tensor(1.0, dtype=torch.float32)
    for b in range(B):
        start, prompt_end, end = (int(v) for v in ranges[b])
        rep, pres, freq = (torch.tensor(float(v), dtype=torch.float32)
                           for v in (repetition[b], presence[b], frequency[b]))
        hist, made = tokens[start:end], tokens[prompt_end:end]
        hist, made = hist[(hist >= 0) & (hist < V)], made[(made >= 0) & (made < V)]
        seen = torch.zeros(V, dtype=torch.bool)
        seen[hist] = True
        c = torch.bincount(made, minlength=V)
        x = x_all[b]
        y = torch.where(seen, torch.where(x > 0, x * (one / rep), x * rep), x)
        y = y - freq * c.float()
        out[b] = torch.where(c > 0, y - pres, y)
    return out.to(logits.device)


def token_logprobs_ref(logits, tokens, top_n=0):
    """Reference of ``ops.token_logprobs``: ``(lp fp32 [B], top_ids int64 [B, top_n], top_lp fp32
    [B, top_n])`` on ``logits.device``.

    Per row, with ``x`` the stored logits as fp32 and ``m = max x``: ``w_i = exp(x_i - m)`` in fp32,
    ``S = sum w_i`` and everything after it in float64, ``lp_i = (x_i - m) - log S``, rounded to
    fp32 at the end. ``lp`` is ``lp_i`` at the row's token; ``top_ids`` are the ``top_n`` largest
    logits in descending order, equal logits by ascending index (a stable descending sort), and
    ``top_lp`` their ``lp_i``. Past ``V`` entries the tail is ``-1`` / ``-inf``."""
    B, V = logits.shape
    top_n = int(top_n)
    x = logits.detach().float().cpu()
    tokens = torch.as_tensor(tokens).detach().cpu().long().reshape(-1)
    top_ids = torch.full((B, top_n), -1, dtype=torch.int64)
    top_lp = torch.full((B, top_n), float("-inf"), dtype=torch.float32)
    if B == 0 or V == 0:
        return torch.empty(B, dtype=torch.float32).to(logits.device), top_ids.to(logits.device), top_lp.to(logits.device)
    m = x.max(dim=1, keepdim=True).values
    d = x - m
    lp_all = d.double() - torch.exp(d).double().sum(dim=1, keepdim=True).log()
    lp = lp_all.gather(1, tokens[:, None])[:, 0].float()
    n = min(top_n, V)
    if n:
        order = torch.sort(x, dim=1, descending=True, stable=True).indices[:, :n]
        top_ids[:, :n] = order
        top_lp[:, :n] = lp_all.gather(1, order).float()
    return lp.to(logits.device), top_ids.to(logits.device), top_lp.to(logits.device)
