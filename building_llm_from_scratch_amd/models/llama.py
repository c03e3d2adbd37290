"""Llama-2 / Llama-3 / 3.1 / 3.2 (one GQA module; MHA is GQA with n_kv_groups == n_heads).

Parity (reference, read-only):
  * module / state-dict names: ``tok_emb``, ``trf_blocks.{i}.att.W_query|W_key|W_value|out_proj``,
    ``trf_blocks.{i}.ff.fc1|fc2|fc3``, ``trf_blocks.{i}.norm1|norm2``, ``final_norm``, ``out_head``
    plus the ``att.mask|cos|sin`` buffers (Llama3.py:108-204, Llama2.py:61-190);
  * math: pre-RMSNorm (eps 1e-5, fp32 weight in checkpoints), rotate-half RoPE with the 3.1
    by-parts smoothing, causal GQA, SwiGLU ``fc3(silu(fc1 x) * fc2 x)``, untied head
    (common_components.py:6-124, Llama3.py:131-181).

MI355X execution (per block, N = B*T rows, all bf16 with fp32 accumulation):
  rmsnorm[HIP] -> QKV GEMM (fused [Wq;Wk;Wv], hipBLASLt) -> RoPE in place[HIP] ->
  flash-attention fwd (GQA-native, no repeat_interleave)[HIP MFMA] -> out-proj GEMM with
  the residual add in the epilogue (addmm beta=1) -> rmsnorm[HIP] -> gate/up GEMM (fused
  [fc1;fc2]) -> SwiGLU[HIP] -> down GEMM + residual.  Backward mirrors it and writes all
  weight gradients into the unit's flat gradient buffer.  The final norm's unit runs the head
  and the loss of models/head.py.
"""
from __future__ import annotations

import sys
import types

import torch
import torch.nn as nn

from .. import ops
from . import head
from .base import BaseLM, UnitCompute, cached_attention, pack_sequences
from .head import HeadComputeMixin
from .linear import FusedLinear, KaugCtx


class _Module(types.ModuleType):
    """``MIN_CHUNK_ROWS`` lived here before models/head.py: reading it here still gives
    ``head.MIN_CHUNK_ROWS`` (test modules of that time import it at collection), but it cannot be
    set here (AttributeError): that would patch a name nobody reads."""
    MIN_CHUNK_ROWS = property(lambda self: head.MIN_CHUNK_ROWS)


sys.modules[__name__].__class__ = _Module


# ---------------------------------------------------------------------------
# reference-named containers (parameters become views into flat unit buffers)
# ---------------------------------------------------------------------------
class RMSNorm(nn.Module):
    def __init__(self, emb_dim, eps=1e-5, dtype=None, device=None):
        super().__init__()
        self.eps = eps
        self.emb_dim = emb_dim
        self.weight = nn.Parameter(torch.ones(emb_dim, dtype=dtype, device=device))

    def reset_parameters(self):   # (seeded per-unit init of a meta-built model, base.py:init_unit_)
        with torch.no_grad():
            self.weight.fill_(1.0)

    def forward(self, x):  # reference-style eager path (used only by tests / users)
        xf = x.float()
        y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)
        return (y * self.weight.float()).to(x.dtype)


class GroupedQueryAttention(nn.Module):
    def __init__(self, d_in, d_out, context_length, num_heads, num_kv_groups, rope_base=10_000,
                 rope_config=None, dtype=None, device=None):
        super().__init__()
        assert d_out % num_heads == 0 and num_heads % num_kv_groups == 0
        self.d_out = d_out
        self.num_heads = num_heads
        self.head_dim = d_out // num_heads
        self.num_kv_groups = num_kv_groups
        self.group_size = num_heads // num_kv_groups
        kw = dict(bias=False, dtype=dtype, device=device)
        self.W_query = nn.Linear(d_in, d_out, **kw)
        self.W_key = nn.Linear(d_in, num_kv_groups * self.head_dim, **kw)
        self.W_value = nn.Linear(d_in, num_kv_groups * self.head_dim, **kw)
        self.out_proj = nn.Linear(d_out, d_out, **kw)


# reference Llama2.py names this MultiHeadAttention
class MultiHeadAttention(GroupedQueryAttention):
    def __init__(self, d_in, d_out, context_length, num_heads, dtype=None, device=None):
        super().__init__(d_in, d_out, context_length, num_heads, num_heads, dtype=dtype, device=device)


class FeedForward(nn.Module):
    def __init__(self, cfg, device=None):
        super().__init__()
        kw = dict(bias=False, dtype=cfg["dtype"], device=device)
        self.fc1 = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], **kw)
        self.fc2 = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], **kw)
        self.fc3 = nn.Linear(cfg["hidden_dim"], cfg["emb_dim"], **kw)


class TransformerBlock(nn.Module):
    def __init__(self, cfg, device=None):
        super().__init__()
        self.att = GroupedQueryAttention(cfg["emb_dim"], cfg["emb_dim"], cfg["context_length"],
                                         cfg["n_heads"], cfg["n_kv_groups"], cfg["rope_base"],
                                         cfg["rope_freq"], dtype=cfg["dtype"], device=device)
        self.ff = FeedForward(cfg, device=device)
        self.norm1 = RMSNorm(cfg["emb_dim"], eps=1e-5, dtype=cfg["dtype"], device=device)
        self.norm2 = RMSNorm(cfg["emb_dim"], eps=1e-5, dtype=cfg["dtype"], device=device)


# ---------------------------------------------------------------------------
# unit computes
# ---------------------------------------------------------------------------
class LlamaEmbedCompute(UnitCompute):
    name = "tok_emb"

    def __init__(self, rctx, model):
        super().__init__(rctx)
        self.m = model

    def layout(self):
        return [[self.m.tok_emb.weight]]

    def forward(self, idx, save, replay=None):
        rc = self.rctx
        W = self.unit.data(self.m.tok_emb.weight)
        x = ops.embedding_fwd(idx.reshape(-1), W, None, rc.T)
        return x.view(rc.B, rc.T, -1), (idx.reshape(-1) if save else None)

    def backward(self, dx, saved):
        g = self.unit.grad(self.m.tok_emb.weight)
        if g is not None:
            ops.embedding_bwd(saved, dx.view(-1, dx.shape[-1]), g, None, self.rctx.T, self.rctx.accumulate)
        return None

    def infer(self, idx, pos):
        W = self.unit.data(self.m.tok_emb.weight)
        return ops.embedding_fwd(idx.reshape(-1).contiguous(), W, None, idx.shape[1])

    def infer_dev(self, idx, pos_t):
        W = self.unit.data(self.m.tok_emb.weight)
        return ops.embedding_fwd(idx.reshape(-1).contiguous(), W, None, 1)

    infer_rows = infer_dev          # per-row positions: no learned positions to look up

    def infer_ragged(self, idx, seq):
        return self.infer_dev(idx, None)


class LlamaBlockCompute(UnitCompute):
    def __init__(self, rctx, block: TransformerBlock, i: int):
        super().__init__(rctx)
        self.block = block
        self.name = f"trf_blocks.{i}"
        self.index = i
        a, f = block.att, block.ff
        self.qkv = FusedLinear([a.W_query, a.W_key, a.W_value])
        self.o = FusedLinear([a.out_proj])
        self.gu = FusedLinear([f.fc1, f.fc2])
        self.down = FusedLinear([f.fc3])

    def layout(self):
        b = self.block
        return (self.qkv.layout() + self.o.layout() + self.gu.layout() + self.down.layout()
                + [[b.norm1.weight], [b.norm2.weight]])

    def bind(self, unit):
        super().bind(unit)
        for fl in (self.qkv, self.o, self.gu, self.down):
            fl.bind(unit)

    def forward(self, x, save, replay=None, recompute=False):
        """``recompute``: the activation-checkpoint re-run inside backward — the block output
        is not needed there, so the down projection GEMM (1/6 of the block's forward FLOPs) is
        skipped; only its LoRA intermediate, if any, is rebuilt."""
        rc, cfg, u, b = self.rctx, self.rctx.cfg, self.unit, self.block
        B, T = rc.B, rc.T
        N, d = B * T, cfg.emb_dim
        H, G, hd = cfg.n_heads, cfg.n_kv_groups, cfg.head_dim
        eps = cfg.norm_eps
        cos, sin = rc.rope
        sq = rc.seq
        x2d = x.reshape(N, d)
        keep = rc.block_mode(self.index) == "none" or recompute  # the recompute's outputs live one block
        # LoRA with a frozen base: the norms / SwiGLU write straight into the K-augmented
        # [x | s t] operand of the next projection (FusedLinear.kaug_input / forward_kaug)
        xq = self.qkv.kaug_input(x2d, d)
        if xq is not None:
            h1, r1 = ops.rmsnorm_fwd_into(x2d, u.data(b.norm1.weight), eps, xq[:, :d])
            qkv, xa_qkv = self.qkv.forward_kaug(xq, d)
            self._rope(qkv)
        else:
            h1, r1 = ops.rmsnorm_fwd(x2d, u.data(b.norm1.weight), eps)
            # K4: RoPE in the GEMM epilogue (position = row % T: not for a packed batch)
            qkv = self.qkv.forward_rope(h1, cos, sin, T, H, G, hd) if sq is None else None
            if qkv is not None:
                xa_qkv = None
            else:
                qkv, xa_qkv = self.qkv.forward(h1)
                self._rope(qkv)
        if sq is not None:   # packed batch: sequence b is rows [cu[b], cu[b+1])
            o, lse = ops.flash_attn_varlen_fwd(qkv, sq.cu, sq.max_len, H, G, hd, bounds=sq.bounds)
        else:
            o, lse = ops.flash_attn_fwd(qkv, B, T, H, G, hd, causal=True)
        x2, xa_o = self.o.forward(o, residual=x2d)
        xg = self.gu.kaug_input(x2, d)
        fused = None
        if xg is not None:
            h2, r2 = ops.rmsnorm_fwd_into(x2, u.data(b.norm2.weight), eps, xg[:, :d])
            gu, xa_gu = self.gu.forward_kaug(xg, d)
        else:
            h2, r2 = ops.rmsnorm_fwd(x2, u.data(b.norm2.weight), eps)
            if not (recompute and not self.down.has_lora and RECOMPUTE_FUSED):
                fused = self.gu.forward_swiglu(h2)     # gate/up GEMM with the SwiGLU epilogue
            if fused is not None:
                (gu, act), xa_gu = fused, None
            else:
                gu, xa_gu = self.gu.forward(h2)
        if recompute and not self.down.has_lora and RECOMPUTE_FUSED:
            # backward rebuilds act inside the SwiGLU backward kernel (swiglu_bwd_act)
            act, x3, xa_dn = None, None, None
        else:
            F = gu.shape[1] // 2
            xd = None if (fused is not None or recompute) else self.down.kaug_input(gu, F)
            if xd is not None:
                act = ops.swiglu_fwd_into(gu, xd[:, :F])
                x3, xa_dn = self.down.forward_kaug(xd, F, residual=x2)
            else:
                if fused is None:
                    act = ops.swiglu_fwd(gu)
                if recompute:
                    x3, xa_dn = None, self.down.lora_state(act)
                else:
                    x3, xa_dn = self.down.forward(act, residual=x2)
        saved = None
        if save:
            if not keep:
                # h1 / h2 are dropped (rebuilt in backward): keep only the s t columns of their
                # K-augmented buffers, not the whole [x | s t]
                xa_qkv, xa_gu = (v.compact() if isinstance(v, KaugCtx) else v for v in (xa_qkv, xa_gu))
            saved = dict(x=x2d, r1=r1, qkv=qkv, o=o, lse=lse, x2=x2, r2=r2, gu=gu,
                         xa=(xa_qkv, xa_o, xa_gu, xa_dn))
            # selective: act is rebuilt by the SwiGLU backward (swiglu_bwd_act), h1/h2 by rmsnorm
            if act is not None and (keep or self.down.has_lora or not RECOMPUTE_FUSED):
                saved["act"] = act
            if keep:
                saved.update(h1=h1, h2=h2)
        return (x3.view(B, T, d) if x3 is not None else None), saved

    def _rope(self, qkv):
        """RoPE in place: position row % T, or each row's index in its sequence (packed batch)."""
        rc, cfg = self.rctx, self.rctx.cfg
        cos, sin = rc.rope
        if rc.seq is not None:
            return ops.rope_pos_(qkv, cos, sin, rc.seq.pos_ids, cfg.n_heads, cfg.n_kv_groups, cfg.head_dim)
        return ops.rope_(qkv, cos, sin, rc.T, cfg.n_heads, cfg.n_kv_groups, cfg.head_dim)

    def infer_dev(self, x2d, pos_t, kv):
        """Decode step with the position in device memory (RoPE reads it, the decode kernel
        appends K/V at it): capturable in a HIP graph and replayed once per generated token."""
        cfg, u, b = self.rctx.cfg, self.unit, self.block
        H, G, hd, eps = cfg.n_heads, cfg.n_kv_groups, cfg.head_dim, cfg.norm_eps
        cos, sin = self.rctx.rope
        h1, _ = ops.rmsnorm_fwd(x2d, u.data(b.norm1.weight), eps)
        qkv, _ = self.qkv.forward(h1)
        ops.rope_dev_(qkv, cos, sin, H, G, hd, pos_t)
        o = ops.attn_decode_append(qkv, kv[0], kv[1], pos_t, H, G)
        x2, _ = self.o.forward(o, residual=x2d)
        h2, _ = ops.rmsnorm_fwd(x2, u.data(b.norm2.weight), eps)
        gu, _ = self.gu.forward(h2)
        x3, _ = self.down.forward(ops.swiglu_fwd(gu), residual=x2)
        return x3

    def w8_groups(self):
        """The block's projection groups, in the order of its entry in ``new_decode_weights``."""
        return (self.qkv, self.o, self.gu, self.down)

    def _infer_qkv(self, x2d, weights=None):
        u, b = self.unit, self.block
        h1, _ = ops.rmsnorm_fwd(x2d, u.data(b.norm1.weight), self.rctx.cfg.norm_eps)
        if weights is not None:
            return self.qkv.forward_pack(h1, weights[0])
        return self.qkv.forward(h1)[0]

    def _infer_out(self, x2d, o, weights=None):
        """Everything after attention: out projection + residual, norm2, SwiGLU MLP + residual."""
        u, b = self.unit, self.block
        if weights is not None:
            x2 = self.o.forward_pack(o, weights[1], residual=x2d)
            h2, _ = ops.rmsnorm_fwd(x2, u.data(b.norm2.weight), self.rctx.cfg.norm_eps)
            gu = self.gu.forward_pack(h2, weights[2])
            return self.down.forward_pack(ops.swiglu_fwd(gu), weights[3], residual=x2)
        x2, _ = self.o.forward(o, residual=x2d)
        h2, _ = ops.rmsnorm_fwd(x2, u.data(b.norm2.weight), self.rctx.cfg.norm_eps)
        gu, _ = self.gu.forward(h2)
        x3, _ = self.down.forward(ops.swiglu_fwd(gu), residual=x2)
        return x3

    def infer_rows(self, x2d, pos_rows, kv, weights=None, q_per_row: int = 1, pos_b=None):
        """``infer_dev`` with a position per row (int32 [B] on the device): RoPE rotates row b at
        ``pos_rows[b]`` and the decode kernel appends and attends there.  ``weights``: the block's
        packs (``new_decode_weights``, fp8 or MXFP4); its four projections then run ``forward_pack``.
        ``q_per_row=Q > 1``: Q consecutive tokens per batch row (rows b*Q + j, ``pos_b`` int32 [B]
        = the batch rows' positions ``pos_rows[::Q]``); attention is ``ops.attn_extend_rows``."""
        cfg = self.rctx.cfg
        H, G, hd = cfg.n_heads, cfg.n_kv_groups, cfg.head_dim
        cos, sin = self.rctx.rope
        qkv = self._infer_qkv(x2d, weights)
        ops.rope_pos_(qkv, cos, sin, pos_rows, H, G, hd)
        if q_per_row != 1:
            return self._infer_out(x2d, ops.attn_extend_rows(qkv, kv[0], kv[1], pos_b, q_per_row, H, G,
                                                             pos_rows=pos_rows), weights)
        return self._infer_out(x2d, ops.attn_decode_append_rows(qkv, kv[0], kv[1], pos_rows, H, G, scales=kv[2:]),
                               weights)

    def infer_ragged(self, x2d, seq, kv, rows=None):
        """Prefill of a ragged batch (packed rows, ``seq``: its SeqPack): variable-length attention,
        and the rotated K / V of sequence b into rows 0 .. len_b - 1 of cache row b
        (``rows``, an ``ops.CacheRows``: of cache row ``rows[b]``)."""
        cfg = self.rctx.cfg
        H, G, hd = cfg.n_heads, cfg.n_kv_groups, cfg.head_dim
        cos, sin = self.rctx.rope
        qkv = self._infer_qkv(x2d)
        ops.rope_pos_(qkv, cos, sin, seq.pos_ids, H, G, hd)
        o, _ = ops.flash_attn_varlen_fwd(qkv, seq.cu, seq.max_len, H, G, hd, bounds=seq.bounds)
        ops.kv_cache_fill_varlen(qkv, seq.cu, kv[0], kv[1], scales=kv[2:], rows=rows)
        return self._infer_out(x2d, o)

    def infer(self, x2d, B, t, pos, kv):
        cfg, u, b = self.rctx.cfg, self.unit, self.block
        H, G, hd, eps = cfg.n_heads, cfg.n_kv_groups, cfg.head_dim, cfg.norm_eps
        cos, sin = self.rctx.rope
        h1, _ = ops.rmsnorm_fwd(x2d, u.data(b.norm1.weight), eps)
        qkv, _ = self.qkv.forward(h1)
        ops.rope_(qkv, cos, sin, t, H, G, hd, pos_offset=pos)
        o = cached_attention(qkv, B, t, pos, H, G, hd, kv)
        x2, _ = self.o.forward(o, residual=x2d)
        h2, _ = ops.rmsnorm_fwd(x2, u.data(b.norm2.weight), eps)
        gu, _ = self.gu.forward(h2)
        x3, _ = self.down.forward(ops.swiglu_fwd(gu), residual=x2)
        return x3

    def _mlp_lora_fusion(self, xa_dn, xa_gu, F):
        """What the SwiGLU backward takes over from the MLP's LoRA groups, decided here once from
        what their forwards saved: ``(lowrank, wgrad)``.  ``lowrank``: the down projection hands
        its dX back as base + s u P and the SwiGLU backward forms it (ops.swiglu_bwd_lowrank).
        ``wgrad`` = (gB_gate, gB_up, gA_down^T), only with ``lowrank``: that pass also sums the
        gate/up dB and the down dA (ops.swiglu_bwd_lowrank_wgrad: both groups K-augmented, rank 16
        per member, all three trainable); else None."""
        dn, gu = self.down, self.gu
        if not dn.lowrank_dx_ok(xa_dn, F):
            return False, None
        if not (LORA_SWIGLU_WGRAD and isinstance(xa_gu, KaugCtx) and dn.lora_R == 16 and gu.lora_r == [16, 16]
                and gu.lora_c0 == [0, F] and gu.lora_len == [F, F] and gu.lora_off == [0, 16]
                and ops.swiglu_bwd_lowrank_wgrad_ok(16, F)):
            return True, None
        u = self.unit
        gBg, gBu = (u.grad(sp.lora_B) for sp in gu.lora_specs)
        gAd = u.grad(dn.lora_specs[0].lora_A)
        if gBg is None or gBu is None or gAd is None or not (gBg.dtype == gBu.dtype == gAd.dtype):
            return True, None
        return True, (gBg, gBu, gAd.t())

    def backward(self, dy, s):
        rc, cfg, u, b = self.rctx, self.rctx.cfg, self.unit, self.block
        B, T = rc.B, rc.T
        N, d = B * T, cfg.emb_dim
        H, G, hd = cfg.n_heads, cfg.n_kv_groups, cfg.head_dim
        eps, acc = cfg.norm_eps, rc.accumulate
        cos, sin = rc.rope
        xa_qkv, xa_o, xa_gu, xa_dn = s["xa"]
        dy2 = dy.reshape(N, d)
        w1, w2 = u.data(b.norm1.weight), u.data(b.norm2.weight)
        # ---- MLP
        wgrad = None
        if "act" in s or self.down.has_lora:
            F = s["gu"].shape[1] // 2
            lowrank, wgrad = self._mlp_lora_fusion(xa_dn, xa_gu, F)
            # the wgrad kernel rebuilds act itself: no SwiGLU forward for the down dA
            act = s["act"] if "act" in s else (s["gu"][:, :F] if wgrad else ops.swiglu_fwd(s["gu"]))
            d_act = self.down.backward(dy2, act, xa_dn, accumulate=acc, lowrank_dx=lowrank,
                                       lora_A_done=wgrad is not None)
            del act
            if wgrad:
                # K-augmented LoRA MLP: dact = base + s u P, the gate/up dB and the down dA summed in
                # the same pass over the rows
                d_gu = ops.swiglu_bwd_lowrank_wgrad(s["gu"], *d_act, xa_gu.st, *wgrad, accumulate=acc)
            elif lowrank:                    # K-augmented LoRA: dact = base + s u P inside the kernel
                d_gu = ops.swiglu_bwd_lowrank(s["gu"], *d_act)
            else:
                d_gu = ops.swiglu_bwd(s["gu"], d_act)
            del d_act
        else:
            # recompute without act: dX GEMM first, then one SwiGLU backward pass that also
            # rebuilds act in place of d_act, then the down projection's dW from it
            act = self.down.input_grad(dy2)
            d_gu = ops.swiglu_bwd_act(s["gu"], act)
            self.down.backward(dy2, act, None, need_dx=False, accumulate=acc)
            del act
        h2 = s["h2"] if "h2" in s else ops.rmsnorm_fwd(s["x2"], w2, eps)[0]
        dh2 = self.gu.backward(d_gu, h2, xa_gu, accumulate=acc, lora_B_done=wgrad is not None)
        del d_gu, h2
        dx2, _ = ops.rmsnorm_bwd(dh2, s["x2"], w2, s["r2"], dy2, u.grad(b.norm2.weight), acc)
        del dh2
        # ---- attention
        d_o = self.o.backward(dx2, s["o"], xa_o, accumulate=acc)
        sq = rc.seq
        if sq is not None:
            dqkv = ops.flash_attn_varlen_bwd(s["qkv"], s["o"], s["lse"], d_o, sq.cu, sq.pos_ids, sq.max_len, H, G, hd,
                                             rope=(cos, sin), bounds=sq.bounds)
        else:
            dqkv = ops.flash_attn_bwd(s["qkv"], s["o"], s["lse"], d_o, B, T, H, G, hd, causal=True,
                                      rope=(cos, sin))  # inverse RoPE fused into the kernels' epilogues
        del d_o
        h1 = s["h1"] if "h1" in s else ops.rmsnorm_fwd(s["x"], w1, eps)[0]
        dh1 = self.qkv.backward(dqkv, h1, xa_qkv, accumulate=acc)
        del dqkv, h1
        dx, _ = ops.rmsnorm_bwd(dh1, s["x"], w1, s["r1"], dx2, u.grad(b.norm1.weight), acc)
        return dx.view(B, T, d)


# False: the gate/up dB and down dA of a LoRA MLP as separate lora_wgrad passes (A/B)
LORA_SWIGLU_WGRAD = True


# False: the checkpoint recompute runs its SwiGLU forward as a separate pass (A/B)
RECOMPUTE_FUSED = True


class LlamaHeadCompute(HeadComputeMixin, UnitCompute):
    name = "final"

    def __init__(self, rctx, model):
        super().__init__(rctx)
        self.m = model
        self.head = FusedLinear([model.out_head])

    def layout(self):
        return [[self.m.final_norm.weight]] + self.head.layout()

    def _norm_fwd(self, x2d):
        h, r = ops.rmsnorm_fwd(x2d, self.unit.data(self.m.final_norm.weight), self.rctx.cfg.norm_eps)
        return h, (r,)

    def _norm_bwd(self, dh, ns):
        x2d, r = ns
        w = self.m.final_norm.weight
        dx, _ = ops.rmsnorm_bwd(dh, x2d, self.unit.data(w), r, None, self.unit.grad(w), self.rctx.accumulate)
        return dx


# ---------------------------------------------------------------------------
class LlamaModel(BaseLM):
    """Llama-2 / 3 / 3.1 / 3.2 (reference Llama2Model, Llama3Model)."""

    def __init__(self, cfg, use_actv_ckpt=False, device=None):
        super().__init__(cfg, use_actv_ckpt)
        dt = cfg["dtype"]
        self.tok_emb = nn.Embedding(cfg["vocab_size"], cfg["emb_dim"], dtype=dt, device=device)
        self.trf_blocks = nn.Sequential(*[TransformerBlock(cfg, device) for _ in range(cfg["n_layers"])])
        self.final_norm = RMSNorm(cfg["emb_dim"], eps=1e-5, dtype=dt, device=device)
        self.out_head = nn.Linear(cfg["emb_dim"], cfg["vocab_size"], bias=False, dtype=dt, device=device)
        self._register_state_dict_hook(_llama_state_dict_hook)
        self._register_load_state_dict_pre_hook(_llama_load_pre_hook)
        self.include_buffers_in_state_dict = True

    def build_computes(self):
        rc = self._rctx
        return ([LlamaEmbedCompute(rc, self)]
                + [LlamaBlockCompute(rc, b, i) for i, b in enumerate(self.trf_blocks)]
                + [LlamaHeadCompute(rc, self)])

    def _pack(self, in_idx, targets, seq_lens):
        # whole MIN_CHUNK_ROWS row counts keep every weight gradient on the token-major dW kernel
        return pack_sequences(in_idx, targets, seq_lens, head.MIN_CHUNK_ROWS, self._anchor.device,
                              self.computes[-1].ignore_index)

    def _after_flatten(self, device):
        cfg = self.cfg
        self._rctx.rope = ops.rope_tables(cfg.head_dim, cfg.context_length, cfg.rope_base,
                                          cfg.rope_freq, device=device)


Llama3Model = LlamaModel
Llama2Model = LlamaModel


def _llama_buffers(cfg):
    """Reference per-block buffers: mask [T,T] fp32 (triu ones), cos/sin [T, hd] (halves
    duplicated) — bf16 for Llama-3.x, fp32 for Llama-2 (Llama3.py:59-70, Llama2.py:83-88)."""
    T, hd = cfg.context_length, cfg.head_dim
    mask = torch.triu(torch.ones(T, T), diagonal=1)
    c, s = ops.rope_tables(hd, T, cfg.rope_base, cfg.rope_freq)
    cos = torch.cat([c, c], dim=1)
    sin = torch.cat([s, s], dim=1)
    if cfg.name != "llama2":
        cos, sin = cos.to(cfg.dtype), sin.to(cfg.dtype)
    return mask, cos, sin


def _llama_state_dict_hook(module, state_dict, prefix, local_metadata):
    # RMSNorm weights are fp32 in the reference's checkpoints
    for k in list(state_dict.keys()):
        if k.endswith("norm1.weight") or k.endswith("norm2.weight") or k.endswith("final_norm.weight"):
            state_dict[k] = state_dict[k].float()
    if getattr(module, "include_buffers_in_state_dict", False):
        mask, cos, sin = _llama_buffers(module.cfg)
        for i in range(module.cfg.n_layers):
            p = f"{prefix}trf_blocks.{i}.att."
            state_dict[p + "mask"] = mask
            state_dict[p + "cos"] = cos
            state_dict[p + "sin"] = sin
    return state_dict


def _llama_load_pre_hook(state_dict, prefix, *args, **kwargs):
    for k in list(state_dict.keys()):
        if k.startswith(prefix) and (k.endswith(".att.mask") or k.endswith(".att.cos") or k.endswith(".att.sin")):
            del state_dict[k]
