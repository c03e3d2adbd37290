"""Final norm + LM head + fused cross-entropy (reference train.py:88-92), shared by the GPT-2 and
Llama head units: the norm is the model's (``_norm_fwd`` / ``_norm_bwd``: RMSNorm in
models/llama.py, LayerNorm in models/gpt2.py), everything from the normed rows to the loss is here.

Training forward (``forward_loss`` with ``save``): the head GEMM, CE forward, CE backward and
both head gradient GEMMs run chunk by chunk over the tokens, so the [N, V] logits never exist
at once (Llama-3-8B, 24k tokens: 6.3 GB of bf16 logits -> 2 GiB chunks, 3 of them; 6 chunks
of 1 GiB measured +5 ms / step, profiles/r2_llama3_8b_fsdp_full_v3.md), for a plain head and for
a LoRA head on a frozen base (one loop, ``_chunked_head_ce``).  The loss gradient is taken for
dloss = ``rctx.loss_scale`` (1, or the fp16 loss scale the trainer announces before the forward)
and rescaled by dloss / loss_scale in backward (dh and dW, one pass each; exactly 1 when the
announced scale is the dloss that arrives).  Taking it at the loss scale matters in fp16: softmax
tails p / nvalid below fp16's smallest subnormal would round to 0 before any later scaling could
lift them.  Any other head, and a forward that saves nothing, runs the whole logits through
``FusedLinear`` and ``ops.ce_fwd``.
"""
from __future__ import annotations

import os
from collections import namedtuple

import torch

from .. import ops
from .linear import _dgrad_wt_ok, _weight_grad, mm_nt, zero_buffer

# logits chunk budget of the fused head + CE (bytes of one [rows, V] chunk)
LOGIT_CHUNK_BYTES = int(os.environ.get("BLLM_LOGIT_CHUNK_MB", "2048")) * 2 ** 20
MIN_CHUNK_ROWS = 256  # chunk rows are a multiple of this (token-major dW kernel K granule)


def chunk_rows(V: int, elem_size: int) -> int:
    """Rows of one logits chunk of width V: what fits LOGIT_CHUNK_BYTES, in whole MIN_CHUNK_ROWS."""
    return max(MIN_CHUNK_ROWS, LOGIT_CHUNK_BYTES // (V * elem_size) // MIN_CHUNK_ROWS * MIN_CHUNK_ROWS)


# saved by the chunked head + CE: dh and the head's gradients exist already, taken for dloss =
# loss_scale (gW: the head weight's, None when frozen; lora: [(parameter, gradient)])
FusedHeadState = namedtuple("FusedHeadState", "x2d ns dh gW lora loss_scale")
# saved by the unfused head: the whole logits, differentiated in backward
LogitsHeadState = namedtuple("LogitsHeadState", "x2d h ns xa logits lse targets nvalid")


class HeadComputeMixin:
    """The head unit's compute but for its norm: the unit provides ``_norm_fwd(x2d) -> (h, ns)``,
    ``_norm_bwd(dh, (x2d,) + ns) -> dx`` and ``self.head``, the head's FusedLinear."""

    ignore_index = -100
    _wpad_buf = _waug_buf = None   # persistent [W ; 0] / [W | B^T | 0] (zero_buffer)

    def bind(self, unit):
        super().bind(unit)
        self.head.bind(unit)

    def infer(self, x2d, B, t, weights=None):
        """Logits of each row's last position.  ``weights``: the head's decode pack
        (``new_decode_weights``: vocabulary rows, fp8 for both weight dtypes); the projection is ``forward_pack``."""
        last = x2d.view(B, t, -1)[:, -1, :].contiguous()
        if weights is not None:
            return self.head.forward_pack(self._norm_fwd(last)[0], weights)
        logits, _ = self.forward_logits(last, save=False)
        return logits

    def infer_rows(self, x2d, rows):
        """Logits of the packed rows ``rows`` (LongTensor on the device) only: a ragged prefill
        needs the head on each sequence's last row, not on all N."""
        logits, _ = self.forward_logits(x2d.index_select(0, rows), save=False)
        return logits

    def forward_logits(self, x, save):
        x2d = x.reshape(-1, x.shape[-1])
        h, ns = self._norm_fwd(x2d)
        logits, xa = self.head.forward(h)
        return logits, ((x2d, h, ns, xa) if save else None)

    def backward_logits(self, dlogits, saved):
        x2d, h, ns, xa = saved
        dl = dlogits.reshape(-1, dlogits.shape[-1]).to(h.dtype)
        dh = self.head.backward(dl, h, xa, accumulate=self.rctx.accumulate)
        dx = self._norm_bwd(dh, (x2d,) + ns)
        return dx.view(self.rctx.B, self.rctx.T, -1)

    def _fused_ok(self, h) -> bool:
        return not self.head.has_lora and self.head.b_params is None

    def _fused_lora_ok(self, h) -> bool:
        hd = self.head
        if not (hd.has_lora and len(hd.specs) == 1 and hd.b_params is None
                and not hd.unit.trainable(hd.W_params[0])):
            return False
        # on the GPU the rank-r parts run on csrc/lora.hip (rank % 16 <= 64, widths % 32)
        spec = hd.specs[0]
        return not h.is_cuda or ops.lora_kernel_ok_dims(h.device, h.dtype, [spec.lora_A.shape[1]],
                                                        [h.shape[1], spec.out_features])

    def _dh_gemm(self, h, rows: int, W: torch.Tensor, frozen: bool):
        """``gemm(dl, out)``: out = dl . W for one chunk.  Where the K-contiguous layout pays, on
        ONE W^T copy made here for every chunk (kept across steps for a frozen W)."""
        if not _dgrad_wt_ok(h[:rows], W):
            return lambda dl, out: torch.mm(dl, W, out=out)
        Wt = self.head.wt_copy.get(W, ops.transpose2d) if frozen else ops.transpose2d(W)
        return lambda dl, out: mm_nt(dl, Wt, out=out)

    def _chunked_head_ce(self, x, Wl, V: int, rows: int, targets, nvalid, dh, dh_gemm, grad_step):
        """The chunk loop of both fused heads: for ``rows`` rows at a time, logits = x . Wl^T, the
        CE forward and (in place) backward on their first V columns, dh = dl . W (``dh_gemm``), then
        ``grad_step(dl, s0)`` takes the head's own gradients from the chunk's dlogits; it
        accumulates from the second chunk on (s0 > 0).  Returns the mean loss."""
        scale = (self.rctx.loss_scale / nvalid).reshape(1)
        total = torch.zeros(1, dtype=torch.float32, device=x.device)
        for s0 in range(0, x.shape[0], rows):
            tc = targets[s0:s0 + rows]
            dl = mm_nt(x[s0:s0 + rows], Wl)                       # logits, then their gradient in place
            lv = dl[:, :V]                                        # (columns >= V: zero pad, stays zero)
            lrow, lse = ops.ce_fwd(lv, tc, self.ignore_index)
            total += lrow.sum()
            ops.ce_bwd_(lv, tc, lse, scale, self.ignore_index)
            dh_gemm(dl, dh[s0:s0 + rows])
            grad_step(dl, s0)
            del dl, lv
        return total[0] / nvalid

    def _fused_loss(self, x2d, h, ns, targets, nvalid):
        """Plain head.  W's rows are padded to a multiple of 256 (zero rows) on the GPU: GPT-2's
        V = 50,257 gives odd-leading-dimension logits, on which hipBLASLt falls back to slower
        non-K-contiguous kernels (2.2-2.6 ms per 16k-token chunk, 0.8-1 PF); the padded vocabulary
        keeps every head GEMM on the tile-aligned kernels and our dW kernel.  The pad rows are
        zeroed once; the V real rows are re-copied per call: the optimizer moves them."""
        W = self.head.W()                                          # [V, d]
        V, d = W.shape
        Vp = -(-V // 256) * 256
        Wp = W
        if Vp != V and W.is_cuda:
            Wp = self._wpad_buf = zero_buffer(self._wpad_buf, Vp, d, W)   # [Vp, d], rows >= V zero
            Wp[:V].copy_(W)
        Vp = Wp.shape[0]
        rows = chunk_rows(Vp, h.element_size())
        gW = gWp = None
        if self.head.unit.trainable(self.head.W_params[0]):
            gW = torch.empty(W.shape, dtype=self.head.unit.train.grad.dtype, device=W.device)
            gWp = gW if Vp == V else torch.empty(Wp.shape, dtype=gW.dtype, device=W.device)
        dh = torch.empty_like(h)

        def grad_step(dl, s0):
            if gWp is not None:
                _weight_grad(dl, h[s0:s0 + rows], gWp, accumulate=s0 > 0)
        loss = self._chunked_head_ce(h, Wp, V, rows, targets, nvalid, dh, self._dh_gemm(h, rows, Wp, False),
                                     grad_step)
        if gWp is not None and gWp is not gW:
            gW.copy_(gWp[:V])
        return loss, FusedHeadState(x2d, ns, dh, gW, [], self.rctx.loss_scale)

    def _fused_lora_loss(self, x2d, h, ns, targets, nvalid):
        """LoRA head (the reference's replace_linear_with_lora also wraps the output head; its
        base weight is frozen) on the same chunked head + CE, with the rank-r path folded into
        the logits GEMM by augmenting K (t = h A, s = alpha / r):
            logits = [h | s t | 0] . [W | B^T | 0]^T          (rows padded to 128-byte lines)
        one GEMM per chunk instead of a separate s t B pass over the [N, V] logits plus a beta = 1
        GEMM.  The dX GEMM stays at the base width, dh_W = dl . W on the cached K-contiguous W^T
        (an augmented [N, d + r] output made hipBLASLt fall back from 1.64 to 0.66-0.75 PF at
        V = 128k, tools/bench_head_k.py); u = dl B^T is a skinny hipBLASLt GEMM over each dlogits
        chunk (355 us vs 610 us for lora_down, tools/bench_head_u.py), dB = (s t)^T dl runs on
        lora_wgrad, then dh = dh_W + s u A^T and dA = s h^T u on the LoRA kernels.  With
        ops.LORA_HEAD_FUSED (default) u and dB come from one kernel reading each dl chunk once
        (``ops.lora_head_bwd_``)."""
        hd, u_ = self.head, self.head.unit
        spec = hd.specs[0]
        A, Bm, sc = u_.data(spec.lora_A), u_.data(spec.lora_B), float(spec.scaling)   # [d, r], [r, V]
        W = hd.W()
        N, d = h.shape
        V, r = W.shape[0], A.shape[1]
        rp = -(-(d + r) // 64) * 64 - d
        # [W | B^T | 0] kept across steps, pad columns zeroed once; W and B^T re-copied per call
        # (FSDP may re-materialise W, the optimizer moves B)
        Wa = self._waug_buf = zero_buffer(self._waug_buf, V, d + rp, W)
        Wa[:, :d].copy_(W)
        Wa[:, d:d + r].copy_(Bm.t())
        P = ops.lora_pack_t([A])                                            # A^T [r, d]
        ha = torch.empty(N, d + rp, dtype=h.dtype, device=h.device)
        ha[:, :d].copy_(h)
        ops.lora_down_into(h, [P], [0], [d], [0], r, sc, ha[:, d:])         # [s h A | 0]
        st = ha[:, d:d + r]
        rows = chunk_rows(V, h.element_size())
        dh_gemm = self._dh_gemm(h, rows, W, True)                           # dh_W = dl . W
        dh = torch.empty_like(h)
        ub = torch.empty(N, r, dtype=h.dtype, device=h.device)
        # (grad views only exist in backward: FSDP allocates the full gradient in pre_backward)
        gB = torch.empty(r, V, dtype=torch.float32, device=h.device) if u_.trainable(spec.lora_B) else None
        fused_bwd = ops.lora_head_bwd_ok(V, r) and Bm.is_contiguous()

        def grad_step(dl, s0):
            if gB is not None and fused_bwd:                                # u and dB in one pass over dl
                ops.lora_head_bwd_(dl, st[s0:s0 + rows], Bm, ub[s0:s0 + rows], gB, accumulate=s0 > 0)
                return
            torch.mm(dl, Bm.t(), out=ub[s0:s0 + rows])            # u = dl B^T (hipBLASLt: 5.9 TB/s here)
            if gB is not None:                                              # dB = (s t)^T dl
                ops.lora_wgrad(st[s0:s0 + rows], dl, [gB], [0], [0], 1.0, accumulate=s0 > 0)
        loss = self._chunked_head_ce(ha, Wa, V, rows, targets, nvalid, dh, dh_gemm, grad_step)
        ops.lora_up_(dh, ub, [P], [0], [0], sc, base=dh)                  # dh_W + s u A^T
        lora = []
        if gB is not None:
            lora.append((spec.lora_B, gB))
        if u_.trainable(spec.lora_A):                                     # dA = s h^T u
            gA = torch.empty(d, r, dtype=torch.float32, device=h.device)
            ops.lora_wgrad(ub, h, [gA.t()], [0], [0], sc)
            lora.append((spec.lora_A, gA))
        return loss, FusedHeadState(x2d, ns, dh, None, lora, self.rctx.loss_scale)

    def forward_loss(self, x, targets, save):
        x2d = x.reshape(-1, x.shape[-1])
        h, ns = self._norm_fwd(x2d)
        if save and (self._fused_ok(h) or self._fused_lora_ok(h)):
            nvalid = (targets != self.ignore_index).sum().to(torch.float32).clamp_(min=1.0)
            if not self._fused_ok(h):
                return self._fused_lora_loss(x2d, h, ns, targets, nvalid)
            return self._fused_loss(x2d, h, ns, targets, nvalid)
        logits, xa = self.head.forward(h)
        rows, lse = ops.ce_fwd(logits, targets, self.ignore_index)
        # a batch whose targets are all ignore_index (e.g. prompts longer than the context in
        # instruction finetuning) gives loss 0 and zero gradients (torch's mean CE gives NaN)
        nvalid = (targets != self.ignore_index).sum().to(torch.float32).clamp_(min=1.0)
        loss = rows.sum() / nvalid
        if not save:
            return loss, None
        return loss, LogitsHeadState(x2d, h, ns, xa, logits, lse, targets, nvalid)

    def backward_loss(self, dloss, saved):
        acc = self.rctx.accumulate
        if isinstance(saved, FusedHeadState):
            dls = dloss.float().reshape(1) / saved.loss_scale
            dh = saved.dh.mul_(dls)
            if saved.gW is not None:
                g = self.head.unit.fused_grad(self.head.W_params)
                if acc:
                    g.add_(saved.gW * dls)
                else:
                    torch.mul(saved.gW, dls, out=g)
            for p, gp in saved.lora:  # LoRA head: dA / dB taken for dloss = loss_scale in forward
                g = self.head.unit.grad(p)
                if acc:
                    g.add_(gp * dls)
                else:
                    g.copy_(gp * dls)
        else:
            scale = (dloss.float() / saved.nvalid).reshape(1)
            dlogits = ops.ce_bwd_(saved.logits, saved.targets, saved.lse, scale, self.ignore_index)  # in place
            dh = self.head.backward(dlogits, saved.h, saved.xa, accumulate=acc)
            del dlogits
        dx = self._norm_bwd(dh, (saved.x2d,) + saved.ns)
        return dx.view(self.rctx.B, self.rctx.T, -1)
