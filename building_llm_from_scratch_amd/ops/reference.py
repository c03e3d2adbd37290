"""Plain-PyTorch implementations of every fused op.

These define the numerical contract of the HIP kernels in ``csrc/`` (same signatures, fp32
internal math) and are the execution path for CPU tensors (unit tests, gloo multi-process
tests, the BASELINE config #1 CPU run).  GPU tensors never reach this module: the
dispatchers in ``ops/__init__.py`` route them to the compiled extension and fail loudly if
it is missing.

Reference ops these replace (all eager PyTorch in the reference):
  RMSNorm   Models/Llama/common_components.py:54-70
  LayerNorm Models/GPT2/GPT2.py:79-80 (nn.LayerNorm)
  RoPE      common_components.py:6-35 (rotate-half)
  attention GPT2.py:38-46, Llama3.py:131-155 (materialised [B,H,T,T] scores + softmax)
  SwiGLU    common_components.py:110-124;  GELU(erf) GPT2.py:58-62
  CE        train.py:88-92 (F.cross_entropy, ignore_index=-100)
  AdamW     torch.optim.AdamW(lr, wd=0.1) build_components.py:250-258
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

# ---------------------------------------------------------------------------
# counter-based dropout RNG (identical bit-for-bit to csrc/common.h::drop_bits16):
# one 32-bit hash per PAIR of element indices, 16 bits per element, 16-bit threshold
# ---------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def _mix32(x: torch.Tensor) -> torch.Tensor:
    """lowbias32 integer hash on int64 tensors holding uint32 values."""
    x = x & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    x = x ^ (x >> 16)
    return x


def drop_threshold16(p: float) -> int:
    return min(int(p * 65536.0), 65536)


def drop_inv_keep(p: float) -> float:
    """Scale of kept elements: 1 / P(keep) for the quantised 16-bit threshold."""
    t = drop_threshold16(p)
    return 0.0 if t >= 65536 else 65536.0 / (65536.0 - t)


def drop_keep_mask(seed: int, offset: int, numel: int, p: float, device=None) -> torch.Tensor:
    """keep[i] = bits16(seed, offset + i) >= p * 2^16."""
    idx = torch.arange(numel, dtype=torch.int64, device=device) + offset
    pair = idx >> 1
    s = _mix32(torch.full_like(pair, seed & _M32) + ((pair >> 32) * 0x9E3779B9 & _M32))
    h = _mix32((pair & _M32) ^ s)
    bits = torch.where((idx & 1) == 1, h >> 16, h & 0xFFFF)
    return bits >= drop_threshold16(p)


# ---------------------------------------------------------------------------
# token sampler (identical bit-for-bit to csrc/common.h::sample_uniform; the contract of
# csrc/sample.hip in fp64)
# ---------------------------------------------------------------------------
def _sample_row_keys(seed: int, stream: torch.Tensor, ctr: torch.Tensor):
    """The two 32-bit row keys of (seed, stream[b], ctr[b]) as int64 tensors [B]."""
    stream, ctr = stream.to(torch.int64), ctr.to(torch.int64)
    seed &= 0xFFFFFFFFFFFFFFFF
    words = [torch.full_like(stream, seed & _M32), torch.full_like(stream, seed >> 32),
             stream & _M32, (stream >> 32) & _M32, ctr & _M32]
    a, b = torch.full_like(stream, 0x9E3779B9), torch.full_like(stream, 0x85EBCA6B)
    for w in words:
        a = _mix32(a ^ w)
        b = _mix32(b + w)
    return a, b


def sample_uniform(seed: int, stream: torch.Tensor, ctr: torch.Tensor, V: int) -> torch.Tensor:
    """u[b, i] of the sampler's counter hash as fp64 [B, V]: an odd multiple of 2^-24, strictly
    inside (0, 1) and exact in fp32."""
    a, b = _sample_row_keys(seed, stream.reshape(-1), ctr.reshape(-1))
    i = torch.arange(V, dtype=torch.int64, device=a.device)
    h = _mix32(_mix32(i[None, :] ^ a[:, None]) + b[:, None])
    return (((h >> 9) << 1) | 1).to(torch.float64) * 2.0 ** -24


def sample_rows_detail(logits, stream, ctr, seed: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                       detail: bool = True):
    """The sampler's contract in fp64 -> (tokens int64 [B], thr fp64 [B], details).

    Row b: NaN logits count as -inf and +inf as the largest fp32; temperature 0 is the argmax
    (lowest index on ties).  Otherwise top-k keeps ``l >= v_k`` (k-th largest value with
    multiplicity, ties kept; 0 or >= V: off), then top-p keeps, inside that set, ``l >= v_p``:
    the largest value whose upward mass ``sum{w_i : l_i >= v}``, ``w = exp((l - max) / T)``,
    reaches ``top_p`` of the set's mass (1: off).  The token is the argmax over the kept set of
    ``l / T - log(-log(u))`` (lowest index on ties), ``u = sample_uniform``.  ``thr`` is the
    smallest kept value, -inf when no filter is on (and at temperature 0).  ``details[b]``
    (``detail``): ``keys`` (fp64 [V], -inf outside the kept set), ``gap`` (top key minus the
    runner-up; inf with one candidate), ``ratios`` (cumulative mass over the set's mass at the
    end of every group of equal values, from the top; empty unless top-p is on) and ``kept``
    (bool [V])."""
    B, V = logits.shape
    ninf = float("-inf")
    l = torch.nan_to_num(logits.detach().to(torch.float64), nan=ninf, neginf=ninf,
                         posinf=float(torch.finfo(torch.float32).max))
    T = float(torch.tensor(float(temperature), dtype=torch.float32))   # the kernel's fp32 parameter
    thr = torch.full((B,), ninf, dtype=torch.float64, device=l.device)

    def first_max(x):                            # the lowest index of a row's maximum
        return (x == x.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)

    if T == 0.0:
        kept = torch.ones(B, V, dtype=torch.bool, device=l.device)
        info = [{"keys": l[b], "gap": float("inf"), "ratios": l.new_zeros(0), "kept": kept[b]} for b in range(B)]
        return first_max(l), thr, info if detail else None
    live = l.max(dim=1).values > ninf            # a row of -inf only has nothing to filter
    kept = torch.ones(B, V, dtype=torch.bool, device=l.device)
    srt = gcum = None
    if 0 < top_k < V:
        vk = torch.where(live, torch.topk(l, top_k, dim=1).values[:, -1], thr)
        kept = l >= vk[:, None]
        thr = vk
    if top_p < 1.0:
        srt, order = torch.sort(l, dim=1, descending=True, stable=True)
        mx = torch.where(live, srt[:, 0], torch.zeros_like(srt[:, 0]))
        w = torch.where(kept.gather(1, order), torch.exp((srt - mx[:, None]) / T), torch.zeros_like(srt))
        cum = w.cumsum(dim=1)
        last = torch.ones(B, V, dtype=torch.bool, device=l.device)     # the end of a group of equal values
        last[:, :-1] = srt[:, :-1] != srt[:, 1:]
        # mass down to the end of each position's group: cum is non-decreasing, so that is the
        # smallest group-end value at or after the position
        gcum = torch.where(last, cum, torch.full_like(cum, float("inf"))).flip(1).cummin(dim=1).values.flip(1)
        total = cum[:, -1:]
        first = (gcum >= top_p * total).to(torch.int8).argmax(dim=1)
        vp = torch.where(live, srt.gather(1, first[:, None])[:, 0], thr)
        kept = kept & (l >= vp[:, None])
        thr = vp
    u = sample_uniform(seed, stream, ctr, V).to(l.device)
    keys = torch.where(kept, l / T - torch.log(-torch.log(u)), torch.full_like(l, ninf))
    tokens = first_max(keys)
    if not detail:
        return tokens, thr, None
    info = []
    for b in range(B):
        top2 = torch.topk(keys[b], min(2, V)).values
        gap = float(top2[0] - top2[1]) if V > 1 and int(kept[b].sum()) > 1 else float("inf")
        ratios = l.new_zeros(0)
        if gcum is not None and bool(live[b]):
            ends = last[b] & (w[b] > 0)
            ratios = cum[b][ends] / total[b]
        info.append({"keys": keys[b], "gap": gap, "ratios": ratios, "kept": kept[b]})
    return tokens, thr, info


def sample_rows(logits, stream, ctr, seed: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                eos_id: int = -1, next_idx=None, out=None, finished=None, thr=None):
    """``sample_rows_detail`` with the kernel's device-side state updates: the token goes to
    ``next_idx[b]``, ``out[b, ctr[b]]`` (column clamped into out) and, when it equals
    ``eos_id >= 0``, sets ``finished[b]``; ``thr[b]`` = smallest kept value (untouched at
    temperature 0); ``ctr[b] += 1``."""
    if top_k < 0 or not (0.0 < top_p <= 1.0) or not temperature >= 0.0:
        raise ValueError(f"sample_rows: top_k {top_k} must be >= 0, top_p {top_p} in (0, 1], temperature "
                         f"{temperature} >= 0")
    tokens, t, _ = sample_rows_detail(logits, stream, ctr, seed, temperature, top_k, top_p, detail=False)
    if next_idx is not None:
        next_idx.view(-1).copy_(tokens)
    if out is not None:
        col = ctr.to(torch.int64).clamp(0, out.shape[1] - 1)
        out[torch.arange(out.shape[0], device=out.device), col] = tokens
    if finished is not None and eos_id >= 0:
        finished |= tokens == eos_id
    if thr is not None and float(temperature) > 0.0:
        thr.copy_(t.to(thr.dtype))
    ctr += 1
    return tokens


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------
def rmsnorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
    y = (xf * rstd[:, None] * w.float()).to(x.dtype)
    return y, rstd


def rmsnorm_bwd(dy, x, w, rstd, dx_acc: Optional[torch.Tensor] = None):
    xf, dyf, wf = x.float(), dy.float(), w.float()
    xhat = xf * rstd[:, None]
    dw = (dyf * xhat).sum(0)
    g = dyf * wf
    d = x.shape[-1]
    dx = rstd[:, None] * (g - xhat * (g * xhat).sum(-1, keepdim=True) / d)
    if dx_acc is not None:
        dx = dx + dx_acc.float()
    return dx.to(x.dtype), dw


def layernorm_fwd(x, w, b, eps: float):
    xf = x.float()
    mean = xf.mean(-1)
    var = (xf - mean[:, None]).pow(2).mean(-1)
    rstd = torch.rsqrt(var + eps)
    y = ((xf - mean[:, None]) * rstd[:, None] * w.float() + b.float()).to(x.dtype)
    return y, mean, rstd


def layernorm_bwd(dy, x, w, mean, rstd, dx_acc: Optional[torch.Tensor] = None):
    xf, dyf, wf = x.float(), dy.float(), w.float()
    xhat = (xf - mean[:, None]) * rstd[:, None]
    dw = (dyf * xhat).sum(0)
    db = dyf.sum(0)
    g = dyf * wf
    d = x.shape[-1]
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).sum(-1, keepdim=True) / d)
    if dx_acc is not None:
        dx = dx + dx_acc.float()
    return dx.to(x.dtype), dw, db


def dropout_add(x, a, p: float, seed: int, offset: int):
    """x + dropout(a)."""
    if p <= 0.0:
        return (x.float() + a.float()).to(x.dtype)
    keep = drop_keep_mask(seed, offset, a.numel(), p, a.device).view_as(a)
    return (x.float() + a.float() * keep * drop_inv_keep(p)).to(x.dtype)


def dropout_bwd(dy, p: float, seed: int, offset: int):
    if p <= 0.0:
        return dy
    keep = drop_keep_mask(seed, offset, dy.numel(), p, dy.device).view_as(dy)
    return (dy.float() * keep * drop_inv_keep(p)).to(dy.dtype)


# ---------------------------------------------------------------------------
# RoPE (rotate-half, non-interleaved) on the packed qkv buffer [N, (H+2G)*hd]
# ---------------------------------------------------------------------------
def rope_tables(head_dim: int, context_length: int, theta_base: float, freq_config=None,
                device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 cos/sin [T, hd/2] (reference Llama3.py:74-104 incl. 3.1 smoothing)."""
    inv_freq = 1.0 / (theta_base ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if freq_config is not None:
        fc = freq_config if isinstance(freq_config, dict) else freq_config.to_dict()
        low_wl = fc["original_context_length"] / fc["low_freq_factor"]
        high_wl = fc["original_context_length"] / fc["high_freq_factor"]
        wavelen = 2 * math.pi / inv_freq
        adj = torch.where(wavelen > low_wl, inv_freq / fc["factor"], inv_freq)
        smooth = (fc["original_context_length"] / wavelen - fc["low_freq_factor"]) / (
            fc["high_freq_factor"] - fc["low_freq_factor"])
        smoothed = (1 - smooth) * (inv_freq / fc["factor"]) + smooth * inv_freq
        med = (wavelen <= low_wl) & (wavelen >= high_wl)
        inv_freq = torch.where(med, smoothed, adj)
    pos = torch.arange(context_length, dtype=torch.float64)
    ang = pos[:, None] * inv_freq[None, :]
    return torch.cos(ang).float().to(device), torch.sin(ang).float().to(device)


def rope_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, T: int, n_heads: int,
          n_kv: int, head_dim: int, inverse: bool = False, pos_offset: int = 0) -> torch.Tensor:
    """In-place RoPE on the q and k heads of qkv [N, (H+2G)*hd]; row r has position
    (r % T) + pos_offset.  ``inverse`` applies the transpose rotation (backward)."""
    N = qkv.shape[0]
    half = head_dim // 2
    v = qkv.view(N, n_heads + 2 * n_kv, head_dim)
    qk = v[:, :n_heads + n_kv, :].float()
    pos = (torch.arange(N, device=qkv.device) % T) + pos_offset
    c = cos[pos][:, None, :]
    s = sin[pos][:, None, :]
    if inverse:
        s = -s
    x1, x2 = qk[..., :half], qk[..., half:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    v[:, :n_heads + n_kv, :] = out.to(qkv.dtype)
    return qkv


def rope_pos_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_ids: torch.Tensor, n_heads: int,
              n_kv: int, head_dim: int, inverse: bool = False) -> torch.Tensor:
    """``rope_`` of a packed variable-length batch: row r is rotated at ``pos_ids[r]``.  Each run
    of consecutive positions 0, 1, 2, ... is one sequence and goes through ``rope_``."""
    pos = [int(p) for p in pos_ids.tolist()]
    r = 0
    while r < len(pos):
        e = r + 1
        while e < len(pos) and pos[e] == pos[e - 1] + 1:
            e += 1
        rope_(qkv[r:e], cos, sin, e - r, n_heads, n_kv, head_dim, inverse, pos_offset=pos[r])
        r = e
    return qkv


# ---------------------------------------------------------------------------
# attention on the packed qkv buffer
# ---------------------------------------------------------------------------
def _split_qkv(qkv, B, T, H, G, hd):
    v = qkv.view(B, T, H + 2 * G, hd)
    q = v[:, :, :H].permute(0, 2, 1, 3).float()
    k = v[:, :, H:H + G].permute(0, 2, 1, 3).float()
    vv = v[:, :, H + G:].permute(0, 2, 1, 3).float()
    return q, k, vv


def _attn_dropout_keep(B, H, T, p, seed, offset, device):
    return drop_keep_mask(seed, offset, B * H * T * T, p, device).view(B, H, T, T)


def flash_attn_fwd(qkv, B: int, T: int, H: int, G: int, hd: int, causal: bool = True,
                   dropout_p: float = 0.0, seed: int = 0, offset: int = 0):
    """Returns o [B*T, H*hd] (qkv dtype) and lse [B, H, T] fp32 in log2 units of the
    *scaled* scores (lse2 = log2 sum_k exp2(s_k * scale * log2e))."""
    q, k, v = _split_qkv(qkv, B, T, H, G, hd)
    rep = H // G
    k = k.repeat_interleave(rep, dim=1)
    v = v.repeat_interleave(rep, dim=1)
    scale = 1.0 / math.sqrt(hd)
    s = (q @ k.transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    if dropout_p > 0.0:
        keep = _attn_dropout_keep(B, H, T, dropout_p, seed, offset, qkv.device)
        p = p * keep * drop_inv_keep(dropout_p)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * T, H * hd).to(qkv.dtype)
    return o, lse * (1.0 / math.log(2.0))


def varlen_bounds(cu) -> list:
    """Host row offsets [B + 1] of a packed variable-length batch from ``cu`` (tensor or list)."""
    return [int(c) for c in (cu.tolist() if isinstance(cu, torch.Tensor) else cu)]


def flash_attn_varlen_fwd(qkv, cu, max_len: int, H: int, G: int, hd: int, attn=None):
    """Causal attention over a packed batch: sequence b is rows [cu[b], cu[b+1]) of qkv
    [N, (H+2G)*hd].  Returns o [N, H*hd] and lse [H * N] fp32 (log2 units), the [H, len_b] block
    of sequence b at H * cu[b].  One call of ``attn`` (default: ``flash_attn_fwd`` above) per
    sequence on its row slice."""
    attn = attn or flash_attn_fwd
    cb = varlen_bounds(cu)
    N = qkv.shape[0]
    o = torch.zeros(N, H * hd, dtype=qkv.dtype, device=qkv.device)
    lse = torch.zeros(H * N, dtype=torch.float32, device=qkv.device)
    for r0, r1 in zip(cb[:-1], cb[1:]):
        if r1 > r0:
            ob, lb = attn(qkv[r0:r1], 1, r1 - r0, H, G, hd, True)
            o[r0:r1] = ob
            lse[H * r0:H * r1] = lb.reshape(-1)
    return o, lse


def flash_attn_varlen_bwd(qkv, o, lse2, do, cu, pos_ids, max_len: int, H: int, G: int, hd: int, rope=None,
                          attn_bwd=None):
    """Backward of ``flash_attn_varlen_fwd`` -> dqkv [N, (H+2G)*hd]; with ``rope`` = (cos, sin)
    dq / dk come back un-rotated at the positions ``pos_ids`` (each row's index in its sequence)."""
    attn_bwd = attn_bwd or flash_attn_bwd
    cb = varlen_bounds(cu)
    dqkv = torch.zeros_like(qkv)
    for r0, r1 in zip(cb[:-1], cb[1:]):
        if r1 > r0:
            L = r1 - r0
            dqkv[r0:r1] = attn_bwd(qkv[r0:r1], o[r0:r1], lse2[H * r0:H * r1].view(1, H, L), do[r0:r1], 1, L, H, G,
                                   hd, True)
    if rope is not None:
        rope_pos_(dqkv, rope[0], rope[1], pos_ids, H, G, hd, inverse=True)
    return dqkv


def flash_attn_bwd(qkv, o, lse2, do, B: int, T: int, H: int, G: int, hd: int, causal: bool = True,
                   dropout_p: float = 0.0, seed: int = 0, offset: int = 0):
    """Returns dqkv [B*T, (H+2G)*hd] (qkv dtype); P is recomputed from lse."""
    q, k, v = _split_qkv(qkv, B, T, H, G, hd)
    rep = H // G
    kx = k.repeat_interleave(rep, dim=1)
    vx = v.repeat_interleave(rep, dim=1)
    scale = 1.0 / math.sqrt(hd)
    s = (q @ kx.transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.exp(s - (lse2 * math.log(2.0))[..., None])
    dO = do.view(B, T, H, hd).permute(0, 2, 1, 3).float()
    O = o.view(B, T, H, hd).permute(0, 2, 1, 3).float()
    if dropout_p > 0.0:
        keep = _attn_dropout_keep(B, H, T, dropout_p, seed, offset, qkv.device)
        pd = p * keep * drop_inv_keep(dropout_p)
    else:
        keep = None
        pd = p
    dv = pd.transpose(-1, -2) @ dO
    dpd = dO @ vx.transpose(-1, -2)
    dp = dpd * keep * drop_inv_keep(dropout_p) if keep is not None else dpd
    delta = (dO * O).sum(-1, keepdim=True)          # = rowsum(P * dP) incl. dropout
    ds = p * (dp - delta) * scale
    dq = ds @ kx
    dk = ds.transpose(-1, -2) @ q
    dk = dk.view(B, G, rep, T, hd).sum(2)
    dv = dv.view(B, G, rep, T, hd).sum(2)
    out = torch.empty(B, T, H + 2 * G, hd, dtype=qkv.dtype, device=qkv.device)
    out[:, :, :H] = dq.permute(0, 2, 1, 3).to(qkv.dtype)
    out[:, :, H:H + G] = dk.permute(0, 2, 1, 3).to(qkv.dtype)
    out[:, :, H + G:] = dv.permute(0, 2, 1, 3).to(qkv.dtype)
    return out.view(B * T, (H + 2 * G) * hd)


# ---------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------
def swiglu_fwd(gu: torch.Tensor) -> torch.Tensor:
    F = gu.shape[-1] // 2
    g, u = gu[:, :F].float(), gu[:, F:].float()
    return (g * torch.sigmoid(g) * u).to(gu.dtype)


def swiglu_bwd(gu: torch.Tensor, dact: torch.Tensor) -> torch.Tensor:
    F = gu.shape[-1] // 2
    g, u, d = gu[:, :F].float(), gu[:, F:].float(), dact.float()
    sg = torch.sigmoid(g)
    silu = g * sg
    dg = d * u * (sg * (1 + g * (1 - sg)))
    du = d * silu
    return torch.cat([dg, du], dim=-1).to(gu.dtype)


def gelu_fwd(f: torch.Tensor) -> torch.Tensor:
    x = f.float()
    return (0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))).to(f.dtype)


def gelu_bwd(f: torch.Tensor, dg: torch.Tensor) -> torch.Tensor:
    x = f.float()
    cdf = 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))
    pdf = torch.exp(-0.5 * x * x) * 0.3989422804014327
    return (dg.float() * (cdf + x * pdf)).to(f.dtype)


# ---------------------------------------------------------------------------
# cross entropy over [N, V] logits (mean over targets != ignore_index)
# ---------------------------------------------------------------------------
def ce_fwd(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100):
    """Returns per-row loss [N] fp32 (0 for ignored rows) and lse [N] fp32 (natural log)."""
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    valid = targets != ignore_index
    t = torch.where(valid, targets, torch.zeros_like(targets))
    tgt = lf.gather(1, t[:, None]).squeeze(1)
    loss = torch.where(valid, lse - tgt, torch.zeros_like(lse))
    return loss, lse


def ce_bwd_(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor, scale: torch.Tensor,
            ignore_index: int = -100) -> torch.Tensor:
    """In place: logits <- (softmax(logits) - onehot(target)) * scale, rows with an ignored
    target set to 0.  ``scale`` is a 1-element fp32 tensor (dloss / n_valid)."""
    lf = logits.float()
    p = torch.exp(lf - lse[:, None])
    valid = targets != ignore_index
    t = torch.where(valid, targets, torch.zeros_like(targets))
    p[torch.arange(p.shape[0], device=p.device), t] -= 1.0
    p = p * valid[:, None].float() * scale.float()
    logits.copy_(p.to(logits.dtype))
    return logits


# ---------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------
def embedding_fwd(idx: torch.Tensor, wte: torch.Tensor, wpe: Optional[torch.Tensor], T: int,
                  dropout_p: float = 0.0, seed: int = 0, offset: int = 0) -> torch.Tensor:
    x = wte.index_select(0, idx.reshape(-1))
    if wpe is not None:
        pos = torch.arange(idx.numel(), device=idx.device) % T
        x = (x.float() + wpe.index_select(0, pos).float()).to(wte.dtype)
    if dropout_p > 0.0:
        keep = drop_keep_mask(seed, offset, x.numel(), dropout_p, x.device).view_as(x)
        x = (x.float() * keep * drop_inv_keep(dropout_p)).to(x.dtype)
    return x


def embedding_bwd(idx, dx, grad_wte: Optional[torch.Tensor], grad_wpe: Optional[torch.Tensor], T: int,
                  accumulate: bool = False):
    """grad_wte[idx[n]] += dx[n]; grad_wpe[n % T] += dx[n] (fp32 sums, written in grad dtype)."""
    flat = idx.reshape(-1)
    if grad_wte is not None:
        acc = torch.zeros(grad_wte.shape, dtype=torch.float32, device=dx.device)
        acc.index_add_(0, flat, dx.float())
        if accumulate:
            acc += grad_wte.float()
        grad_wte.copy_(acc.to(grad_wte.dtype))
    if grad_wpe is not None:
        pos = torch.arange(flat.numel(), device=dx.device) % T
        acc = torch.zeros(grad_wpe.shape, dtype=torch.float32, device=dx.device)
        acc.index_add_(0, pos, dx.float())
        if accumulate:
            acc += grad_wpe.float()
        grad_wpe.copy_(acc.to(grad_wpe.dtype))


# ---------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------
def sq_norm(t: torch.Tensor) -> torch.Tensor:
    return t.float().pow(2).sum()


def adamw_step_(param: torch.Tensor, master: Optional[torch.Tensor], grad: torch.Tensor,
                exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, lr: float, beta1: float, beta2: float,
                eps: float, weight_decay: float, step: int, grad_scale: Optional[torch.Tensor] = None):
    """torch.optim.AdamW semantics (decoupled wd, bias correction) on one flat buffer.
    ``grad_scale`` (1-element fp32 tensor) multiplies the gradient first (clip coef and/or
    fp16 loss-scale inverse).  ``master`` is the fp32 copy when ``param`` is low precision."""
    p32 = master if master is not None else param
    g = grad.float()
    if grad_scale is not None:
        g = g * grad_scale.float()
    p32.mul_(1.0 - lr * weight_decay)
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
    p32.addcdiv_(exp_avg, denom, value=-lr / bc1)
    if master is not None:
        param.copy_(master.to(param.dtype))


def attn_decode(q, kcache, vcache, L: int):
    """Reference for the KV-cache decode kernel: q [B,H,hd], cache [B,G,Tmax,hd] -> [B,H*hd]."""
    B, H, hd = q.shape
    G = kcache.shape[1]
    k = kcache[:, :, :L].float().repeat_interleave(H // G, dim=1)   # [B,H,L,hd]
    v = vcache[:, :, :L].float().repeat_interleave(H // G, dim=1)
    s = torch.einsum("bhd,bhld->bhl", q.float(), k) / math.sqrt(hd)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhl,bhld->bhd", p, v).reshape(B, H * hd).to(q.dtype)


def attn_decode_append_rows(qkv, kcache, vcache, pos, H: int, G: int):
    """Reference for the per-row decode step: qkv [B, (H+2G)*hd] (one token per row), cache
    [B,G,Tmax,hd], pos int [B].  Row b's k / v go into cache row pos[b] and its query attends over
    keys 0..pos[b] -> [B, H*hd]."""
    B, hd = qkv.shape[0], kcache.shape[3]
    rows = qkv.view(B, H + 2 * G, hd)
    out = torch.empty(B, H * hd, dtype=qkv.dtype, device=qkv.device)
    for b, p in enumerate(int(p) for p in pos.tolist()):
        kcache[b, :, p] = rows[b, H:H + G]
        vcache[b, :, p] = rows[b, H + G:]
        out[b] = attn_decode(rows[b:b + 1, :H], kcache[b:b + 1], vcache[b:b + 1], p + 1)[0]
    return out


def attn_extend_rows(qkv, kcache, vcache, pos, Q: int, H: int, G: int):
    """Reference for Q tokens per row over the cache: qkv [B*Q, (H+2G)*hd], row b*Q + j = token j of
    batch row b at position pos[b] + j.  By definition Q consecutive per-row decode steps at
    ``pos``, ``pos + 1``, ...: token j's k / v go into cache row pos[b] + j and its query attends
    over keys 0..pos[b]+j -> [B*Q, H*hd]."""
    B = kcache.shape[0]
    rows = qkv.view(B, Q, -1)
    out = torch.empty(B, Q, H * kcache.shape[3], dtype=qkv.dtype, device=qkv.device)
    for j in range(Q):
        out[:, j] = attn_decode_append_rows(rows[:, j].contiguous(), kcache, vcache, pos + j, H, G)
    return out.view(B * Q, -1)


def spec_advance(idx, samp, hist, h0, pos, ctr, nsteps, finished, out, eos_id: int, ngram: int,
                 accept: bool = True):
    """One step of speculative decoding's bookkeeping (prompt lookup), in place; ``K = Q - 1``.

    ``idx`` int64 [B, Q]: the step's input tokens (the last emitted token, then K drafts);
    ``samp`` int64 [B, Q]: what the sampler chose from the step's Q logits rows; ``hist`` int32
    [B, Lh]: corpus row b = ``h0[b]`` hint tokens, then the row's sequence (position p at
    ``hist[b, h0[b] + p]``); ``h0`` / ``pos`` / ``ctr`` / ``nsteps`` int32 [B]; ``finished`` bool
    [B]; ``out`` int64 [B, new].

    Accept (``accept``, rows that are not finished): a = the number of leading j in 1..K with
    ``idx[b, j] == samp[b, j - 1]``; e = min(a + 1, new - ctr[b]), cut to j + 1 at the first
    ``samp[b, j] == eos_id`` with j < e (``eos_id >= 0``), which finishes the row; ``samp[b, :e]``
    goes to ``out[b, ctr[b]:ctr[b] + e]`` and to ``hist`` at positions pos[b] + 1 ..; pos and ctr
    advance by e, nsteps by 1; the row finishes when ctr reaches new.  A finished row changes
    nothing.

    Draft (every row): n = h0[b] + pos[b] + 1, c = hist[b, :n].  With the largest i in
    [0, n - ngram - 1] such that c[i : i + ngram] == c[n - ngram : n] and per = n - i - ngram,
    draft j = c[i + ngram + ((j - 1) mod per)]; without one (or n <= ngram) every draft is c[n - 1].
    ``idx[b] = [c[n - 1], draft 1, ..., draft K]``."""
    B, Q = idx.shape
    K, new = Q - 1, out.shape[1]
    for b in range(B):
        if accept and not bool(finished[b]):
            s = [int(v) for v in samp[b].tolist()]
            d = [int(v) for v in idx[b].tolist()]
            a = 0
            while a < K and d[a + 1] == s[a]:
                a += 1
            c, p = int(ctr[b]), int(pos[b])
            e = min(a + 1, new - c)
            fin = False
            if eos_id >= 0:
                for j in range(e):
                    if s[j] == eos_id:
                        e, fin = j + 1, True
                        break
            for j in range(e):
                out[b, c + j] = s[j]
                hist[b, int(h0[b]) + p + 1 + j] = s[j]
            pos[b] += e
            ctr[b] += e
            nsteps[b] += 1
            if fin or c + e >= new:
                finished[b] = True
        n = int(h0[b]) + int(pos[b]) + 1
        c = [int(v) for v in hist[b, :n].tolist()]
        best = -1
        if n > ngram:
            tail = c[n - ngram:]
            for i in range(n - ngram - 1, -1, -1):
                if c[i:i + ngram] == tail:
                    best = i
                    break
        row = [c[n - 1]] * Q
        if best >= 0:
            per = n - best - ngram
            for j in range(1, Q):
                row[j] = c[best + ngram + (j - 1) % per]
        idx[b] = torch.tensor(row, dtype=idx.dtype, device=idx.device)


def kv_cache_fill_varlen(qkv, cu, kcache, vcache, rows=None):
    """Reference for the cache prefill from a packed batch: sequence b is rows [cu[b], cu[b+1]) of
    qkv [N, (H+2G)*hd]; cache rows (b, g, t < len_b) <- the k / v of row cu[b] + t.  ``rows``
    (host ints, one per sequence): sequence b goes to cache row ``rows[b]`` instead of row b."""
    G, hd = kcache.shape[1], kcache.shape[3]
    packed = qkv.view(qkv.shape[0], -1, hd)
    H = packed.shape[1] - 2 * G
    cb = varlen_bounds(cu)
    dst = range(len(cb) - 1) if rows is None else [int(r) for r in rows]
    for b, r0, r1 in zip(dst, cb[:-1], cb[1:]):
        kcache[b, :, :r1 - r0] = packed[r0:r1, H:H + G].transpose(0, 1)
        vcache[b, :, :r1 - r0] = packed[r0:r1, H + G:].transpose(0, 1)


# ------------------------------------------------------------------ FP8 KV cache (csrc/attn_decode_fp8.hip oracle)
# The format: a head row x (its last dimension, read as fp32) is stored as e4m3fn bytes and one
# fp32 scale.  a = max |x|; s = a / 448, or 1 when a = 0; byte_i = e4m3fn_rne(x_i / s); both
# divisions are correctly rounded fp32 divisions (formed here in fp64 and rounded once: the fp64
# quotient of two fp32 numbers is far enough from every fp32 rounding boundary that the second
# rounding changes nothing).  |x_i / s| <= 448 (1 + 2^-23), which the cast rounds to 448, so it
# never saturates.  Dequantised value = float(byte_i) * s.  A block's fp8 cache is
# (K8, V8, Ks, Vs): bytes [B, G, Tmax, hd] and scales [B, G, Tmax].
FP8_MAX = 448.0


def kv_quantize_rows(x):
    """x [..., hd] (bf16 / fp16 / fp32) -> (bytes [..., hd] float8_e4m3fn, scales [...] fp32)."""
    x64 = x.float().double()
    a = x64.abs().amax(dim=-1)
    s = torch.where(a > 0, a / FP8_MAX, torch.ones_like(a)).float()
    q = (x64 / s.double()[..., None]).float().to(torch.float8_e4m3fn)
    return q, s


def kv_dequantize(q, s, dtype=torch.float32):
    """bytes [..., hd] float8_e4m3fn and scales [...] fp32 -> [..., hd] of ``dtype`` (exact in fp32)."""
    return (q.float() * s[..., None]).to(dtype)


def attn_decode_append_rows_fp8(qkv, k8, v8, kscale, vscale, pos, H: int, G: int):
    """``attn_decode_append_rows`` on an fp8 cache: row b's new k / v are quantised into cache row
    pos[b] (bytes and scales), and its query attends over the dequantised keys 0..pos[b], the new
    one included in its quantised form: a function of the cache contents after the append."""
    B, hd = qkv.shape[0], k8.shape[3]
    rows = qkv.view(B, H + 2 * G, hd)
    out = torch.empty(B, H * hd, dtype=qkv.dtype, device=qkv.device)
    for b, p in enumerate(int(p) for p in pos.tolist()):
        k8[b, :, p], kscale[b, :, p] = kv_quantize_rows(rows[b, H:H + G])
        v8[b, :, p], vscale[b, :, p] = kv_quantize_rows(rows[b, H + G:])
        kd = kv_dequantize(k8[b:b + 1, :, :p + 1], kscale[b:b + 1, :, :p + 1])
        vd = kv_dequantize(v8[b:b + 1, :, :p + 1], vscale[b:b + 1, :, :p + 1])
        out[b] = attn_decode(rows[b:b + 1, :H], kd, vd, p + 1)[0]
    return out


def kv_cache_fill_varlen_fp8(qkv, cu, k8, v8, kscale, vscale, rows=None):
    """``kv_cache_fill_varlen`` into an fp8 cache: rows (b, g, t < len_b) and their scales <- the
    quantised k / v of packed row cu[b] + t; nothing else is written.  ``rows``: as there."""
    G, hd = k8.shape[1], k8.shape[3]
    packed = qkv.view(qkv.shape[0], -1, hd)
    H = packed.shape[1] - 2 * G
    cb = varlen_bounds(cu)
    dst = range(len(cb) - 1) if rows is None else [int(r) for r in rows]
    for b, r0, r1 in zip(dst, cb[:-1], cb[1:]):
        for c8, cs, src in ((k8, kscale, packed[r0:r1, H:H + G]), (v8, vscale, packed[r0:r1, H + G:])):
            q, s = kv_quantize_rows(src.transpose(0, 1))
            c8[b, :, :r1 - r0] = q
            cs[b, :, :r1 - r0] = s


# ------------------------------------------------------------------ fp8 decode weights (csrc/linear_w8.hip oracle)
def linear_w8(x, q, s, bias=None, residual=None):
    """Reference for the fp8-weight projection, in fp64: x [M, K], q [N, K] float8_e4m3fn and
    s [N] fp32 (``kv_quantize_rows`` of a weight's rows) ->
    ``y[m, n] = s[n] * sum_k x[m, k] q[n, k] + bias[n] + residual[m, n]`` in x's dtype."""
    v = (x.double() @ q.double().t()) * s.double()
    if bias is not None:
        v = v + bias.double()
    if residual is not None:
        v = v + residual.double()
    return v.to(x.dtype)


# ------------------------------------------------------------------ MXFP4 decode weights (csrc/linear_w4.hip oracle)
# The format (OCP MX): a row x (its last dimension, read as fp32) is cut into blocks of 32
# consecutive elements; a block is 32 e2m1 codes and one E8M0 scale byte.
#   scale: a = max |x| over the block; e = the smallest integer with a <= 6 * 2^e, found from
#       a = m * 2^p, m in [0.5, 1) (frexp, no floating-point log2): e = p - 3 if m <= 0.75, else
#       p - 2; clamped to [-126, 127]; a == 0 gives e = 0.  The byte is e + 127, so byte << 23 is
#       the fp32 2^e bit for bit, and 255 is never written.  The largest element is never clipped
#       (the floor(log2 a) - 2 rule saturates a maximum in (6, 8) * 2^e by up to 25 %).
#   code: sign bit (8) + 3 bits; magnitudes MX4_VALUES[0..7]; x / 2^e (exact) is rounded to the
#       nearest magnitude, ties to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2,
#       2.5 -> 2, 3.5 -> 4, 5 -> 4.  A value that rounds to zero gets code 0 whatever its sign.
#   storage: two codes to a byte, element 2 i in the low nibble.
#   dequantised value: magnitude * 2^e, exact in fp32 and bf16 (in fp16 while 2^-13 <= 2^e <= 2^13).
#   error: |x - dequantised| <= max(|x| / 4, 2^e / 4) per element -- the magnitudes from 1 up are at
#       most a quarter of the smaller neighbour apart from a midpoint, the ones below 1 are 0.5 apart.
MX4_BLOCK = 32
MX4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx4_quantize_rows(x):
    """x [..., K] (bf16 / fp16 / fp32, K a multiple of 32) -> (codes uint8 [..., K/2], scale uint8
    [..., K/32]) in the MXFP4 format above.  Torch ops only: the same values give the same bytes on
    the CPU and on the GPU.  Per element ``|x - mx4_dequantize(...)| <= max(|x| / 4, 2^e / 4)``
    with e the block's exponent.  A non-finite x raises ValueError."""
    K = x.shape[-1]
    if x.dim() < 1 or K < MX4_BLOCK or K % MX4_BLOCK:
        raise ValueError(f"mx4_quantize_rows: the last dimension must be a positive multiple of {MX4_BLOCK}, "
                         f"got {tuple(x.shape)}")
    xf = x.float()
    if not bool(torch.isfinite(xf).all()):
        raise ValueError("mx4_quantize_rows: x has non-finite values")
    xb = xf.reshape(*x.shape[:-1], K // MX4_BLOCK, MX4_BLOCK)
    a = xb.abs().amax(dim=-1)
    m, p = torch.frexp(a)
    e = torch.where(m <= 0.75, p - 3, p - 2).clamp(-126, 127)
    e = torch.where(a > 0, e, torch.zeros_like(e)).to(torch.int32)
    two_e = ((e + 127) << 23).view(torch.float32)
    v = (xb / two_e[..., None]).abs()
    code = ((v > 0.25).to(torch.uint8) + (v >= 0.75).to(torch.uint8) + (v > 1.25).to(torch.uint8)
            + (v >= 1.75).to(torch.uint8) + (v > 2.5).to(torch.uint8) + (v >= 3.5).to(torch.uint8)
            + (v > 5.0).to(torch.uint8))
    code = code + (((xb < 0) & (code > 0)).to(torch.uint8) << 3)
    code = code.reshape(*x.shape[:-1], K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).contiguous(), (e + 127).to(torch.uint8)


def mx4_dequantize(codes, scale, dtype=torch.float32):
    """codes uint8 [..., K/2] and scale uint8 [..., K/32] -> [..., K] of ``dtype`` (exact in fp32)."""
    K = codes.shape[-1] * 2
    c = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(*codes.shape[:-1], K // MX4_BLOCK, MX4_BLOCK)
    mag = torch.tensor(MX4_VALUES, dtype=torch.float32, device=codes.device)[(c & 7).long()]
    mag = torch.where((c & 8) != 0, -mag, mag)
    two_e = (scale.to(torch.int32) << 23).view(torch.float32)
    return (mag * two_e[..., None]).reshape(*codes.shape[:-1], K).to(dtype)


def linear_w4(x, codes, scale, bias=None, residual=None):
    """Reference for the MXFP4-weight projection, in fp64: x [M, K], codes [N, K/2] and scale
    [N, K/32] (``mx4_quantize_rows`` of a weight's rows) ->
    ``y[m, n] = sum_k x[m, k] w[n, k] + bias[n] + residual[m, n]`` in x's dtype, w the dequantised
    weight; for fp16 x it is rounded to fp16 first, as the kernel's conversion does (exact while
    2^-13 <= 2^e <= 2^13)."""
    w = mx4_dequantize(codes, scale)
    if x.dtype == torch.float16:
        w = w.to(torch.float16)
    v = x.double() @ w.double().t()
    if bias is not None:
        v = v + bias.double()
    if residual is not None:
        v = v + residual.double()
    return v.to(x.dtype)


# ------------------------------------------------------------------ LoRA (csrc/lora.hip oracle)
def lora_down(x, ws, c0, lens, ocol, R: int, scale: float = 1.0):
    """out[:, ocol_i : ocol_i + r_i] = scale * x[:, c0_i : c0_i + len_i] @ w_i[:, :len_i]^T"""
    out = torch.zeros(x.shape[0], R, dtype=torch.float32, device=x.device)
    for w, c, n, o in zip(ws, c0, lens, ocol):
        out[:, o:o + w.shape[0]] = x[:, c:c + n].float() @ w[:, :n].float().t()
    return (out * scale).to(x.dtype)


def lora_up_(y, t, us, c0, toff, scale: float, base=None, bias=None):
    """y[:, c0_i : c0_i + len_i] = base + bias + scale * t[:, toff_i : toff_i + r_i] @ u_i
    (u_i [r_i, len_i]; base / bias optional)"""
    for u, c, o in zip(us, c0, toff):
        r, n = u.shape
        v = scale * (t[:, o:o + r].float() @ u.float())
        if base is not None:
            v = v + base[:, c:c + n].float()
        if bias is not None:
            v = v + bias[c:c + n].float()
        y[:, c:c + n] = v.to(y.dtype)
    return y


def lora_wgrad(p, q, gs, pa, qb, scale: float, accumulate: bool):
    """g_i[a][b] (+)= scale * sum_n p[n][pa_i + a] q[n][qb_i + b]  (g_i [r_i, len_i], may be a view)"""
    for g, a0, b0 in zip(gs, pa, qb):
        r, n = g.shape
        v = scale * (p[:, a0:a0 + r].float().t() @ q[:, b0:b0 + n].float())
        if accumulate:
            v = v + g.float()
        g.copy_(v.to(g.dtype))


def lora_pack_t(As):
    """[sum r_i, K] = concat_i A_i^T"""
    return torch.cat([a.t() for a in As], 0).contiguous()
