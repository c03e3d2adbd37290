"""Gradient accumulation: one optimizer step over K micro-batches (``--grad_accum_steps K``).

The step is the one a single batch made of the K micro-batches would have taken.  With ``n_i``
the non-ignored targets of micro-batch i (counted on the host tensors the loader yields) and
``L_i`` its mean loss, the step loss is ``L = sum_i n_i L_i / sum_i n_i`` and micro-batch i is
back-propagated with weight ``w_i = n_i / sum_i n_i``: 1/K for pretraining batches, token
weighting for instruction batches, whose ``n_i`` differ.  ``sum_i n_i = 0`` gives loss 0 and zero
gradients, like today's all-ignored batch.  The weighting is per rank; ranks are averaged by
the engines exactly as without accumulation (``grad_prescale``).

Micro-step 0 overwrites the flat gradients and the later ones add into them
(``RunCtx.accumulate``, threaded through every gradient-writing kernel), in the flat gradient
dtype: no second gradient buffer and no extra pass over the parameters.  Which micro-step issues
the gradient collectives is the engine's decision (``begin_micro_step``).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from ..data.datasets import unpad_lengths

IGNORE_INDEX = -100   # the instruction collate's masked-target id (data/datasets.py)


def micro_weights(micro_batches: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> Tuple[List[float], List[int]]:
    """(w_i, n_i) of a group: each micro-batch's share of the group's non-ignored targets."""
    counts = [int((tgt != IGNORE_INDEX).sum()) for _, tgt in micro_batches]
    total = sum(counts)
    return [n / total if total else 0.0 for n in counts], counts


def accumulate_step(model, micro_batches: Sequence[Tuple[torch.Tensor, torch.Tensor]],
                    loss_scale: Optional[float] = None, unpad: bool = False) -> torch.Tensor:
    """Forward and backward of every (input, target) micro-batch of one optimizer step; the flat
    gradients end up holding the step's gradient (times ``loss_scale``).  Returns ``L``.

    ``loss_scale`` is the fp16 loss scale: each backward is ``(L_i * w_i * scale).backward()`` and
    the fused head takes its logit gradient at the scaled magnitude (``rctx.loss_scale``).  The
    overflow test, the clip and the optimizer step are the caller's, once, on the accumulated
    gradients.  ``rctx.accumulate`` is False again when this returns or raises: the next plain
    step or evaluation overwrites."""
    k = len(micro_batches)
    if k < 1:
        raise ValueError("accumulate_step needs at least one micro-batch")
    rc = model.rctx
    eng = rc.engine
    weights, _ = micro_weights(micro_batches)
    scale = 1.0 if loss_scale is None else float(loss_scale)
    if loss_scale is not None:
        rc.loss_scale = scale
    total = None
    try:
        for i, (inp, tgt) in enumerate(micro_batches):
            eng.begin_micro_step(i, k)
            if unpad:   # each micro-batch is packed on its own
                loss = model(inp, tgt, seq_lens=unpad_lengths(tgt))
            else:
                loss = model(inp, tgt)
            (loss * (weights[i] * scale)).backward()
            part = loss.detach().float() * weights[i]
            total = part if total is None else total + part
    finally:
        eng.begin_micro_step(0, 1)
    return total
