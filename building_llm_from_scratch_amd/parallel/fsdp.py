"""Fully sharded data parallel (ZeRO-3) over units.

Reference: ``FSDP(model, auto_wrap_policy=ModuleWrapPolicy({nn.Embedding, GPT2 TransformerBlock}),
FULL_SHARD, BACKWARD_PRE, mixed_precision=<policy>)`` (build_components.py:155-174) — which
for Llama wraps only the embedding, leaving the whole block stack in one root unit (SURVEY
§2.8 defect 3), and crashes at import (defect 2).

Here every unit (embedding, each transformer block, final norm + head) is an FSDP unit for
every model family:
  * each unit's flat buffers (trainable and frozen) are padded to a multiple of world size;
    a rank keeps only its 1/world shard persistently (compute dtype) plus the optimizer's
    fp32 master / moments for that shard;
  * forward: ``all_gather_into_tensor`` of unit i+1 is issued asynchronously (RCCL's own HIP
    stream) while unit i computes (prefetch); after its forward a unit is resharded (storage
    freed) unless ``reshard_after_forward=False`` (ZeRO-2 style: keep until backward);
  * backward: the gather of unit i-1 is prefetched while unit i runs its backward; unit i's
    full gradient is reduce-scattered asynchronously into its gradient shard and freed;
  * gradient clipping: shard-local sum of squares + one scalar all-reduce;
  * checkpoint: full state dict gathered unit by unit to rank 0 with the reference key names.
Mixed precision: the flats hold the policy's ``param_dtype``; gradients are reduce-scattered
in its ``reduce_dtype`` (one cast each way when it differs, e.g. ``bf16_hybrid``: fp32 params,
bf16 collectives — reference datautils/mixed_precision.py:24-28); master weights stay fp32.

World size 1: like torch FSDP, which clamps FULL_SHARD to NO_SHARD when there is a single
rank (torch/distributed/fsdp/_init_utils.py:426-437), the shard IS the full flat: nothing is
freed, gathered or reduce-scattered (a world-1 collective is a device copy of every unit per
pass).  It is the same engine class, hooks and optimizer slots as at N>1.  ``BLLM_FORCE_COMM=1`` keeps
the sharded path at world 1 (RCCL copies) to rehearse it on one GPU.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from ..models.base import LocalEngine
from ..models.flat import ALIGN
from ..train.optim import OptSlot


def _free(t: torch.Tensor):
    st = t.untyped_storage()
    if st.size() > 0:
        st.resize_(0)


def _alloc(t: torch.Tensor, nbytes: int):
    st = t.untyped_storage()
    if st.size() != nbytes:
        st.resize_(nbytes)


class FSDPEngine(LocalEngine):
    def __init__(self, model, device, reduce_dtype: Optional[torch.dtype] = None,
                 reshard_after_forward: bool = True, pg=None, prefetch: int = 1):
        self.pg = pg
        self.world_size = dist.get_world_size(pg)
        self.rank = dist.get_rank(pg)
        self.model = model
        self.device = torch.device(device)
        self.reshard_after_forward = reshard_after_forward
        # units gathered ahead of the one computing (forward: i+1..i+prefetch, backward:
        # i-1..i-prefetch); each extra unit costs one gathered unit of memory (Llama-3-8B block:
        # 436 MB bf16) and buys slack when a gather is slower than one unit's compute.
        # prefetch 0 / None = auto: sized per batch shape from the block's gather time over xGMI
        # vs its forward compute (parallel/commplan.py:fsdp_prefetch_depth)
        self.prefetch_auto = prefetch in (0, None, "auto")
        self.prefetch = 1 if self.prefetch_auto else max(1, int(prefetch))
        self._prefetch_tokens = None
        self.grad_prescale = 1.0 / self.world_size
        self.is_cuda = self.device.type == "cuda"
        from .commstats import CommStats
        self.comm = CommStats(self.device, self.world_size)
        self.adapt_log: List[Dict] = []
        from . import force_comm
        self.no_shard = self.world_size == 1 and not force_comm()
        dtype = next(model.parameters()).dtype
        self.reduce_dtype = reduce_dtype if reduce_dtype not in (None, dtype) else None
        # A model built on the meta device is initialised unit by unit inside flatten (seeded per
        # unit: every rank computes the same values, models/base.py:init_unit_), and each unit is
        # sharded and freed before the next is allocated: no rank ever holds the whole model and
        # nothing is broadcast.  An eagerly built model (e.g. weights loaded on rank 0) is
        # broadcast unit by unit from rank 0 instead.
        meta = any(p.is_meta for p in model.parameters())
        self.deferred_init = meta
        W, r = self.world_size, self.rank

        def shard_unit(u):
            st = u.state
            st["bufs"] = []
            for fb in u.buffers():
                n = fb.numel // W
                fb.nbytes = fb.data.untyped_storage().size()
                if self.no_shard:
                    fb.shard = fb.data
                    if fb is u.train:
                        fb.grad_shard = fb.grad
                    st["bufs"].append(fb)
                    continue
                if not meta:
                    dist.broadcast(fb.data, src=0, group=pg)      # identical init on every rank
                fb.shard = fb.data[r * n:(r + 1) * n].clone()
                if fb is u.train:
                    fb.grad_shard = torch.zeros(n, dtype=fb.grad.dtype, device=device)
                    fb.grad_nbytes = fb.grad.untyped_storage().size()
                    fb.gaps = self._gaps(fb)
                    _free(fb.grad)
                _free(fb.data)
                st["bufs"].append(fb)
            st["gathered"] = self.no_shard
            st["gather_work"] = None
            st["sharded"] = not self.no_shard   # read by FusedLinear._kaug_ok (no persistent W copies)

        model.flatten(device=device, dtype=dtype, pad_to=self.world_size * ALIGN, on_unit=shard_unit)
        self.units = model.units
        self._rs_works: List = []
        self._in_backward = False
        self._micro = 0               # micro-step of the optimizer step (begin_micro_step)
        model.set_engine(self)

    @staticmethod
    def _gaps(fb):
        """Element ranges of the flat NOT covered by parameters (alignment + tail padding):
        zeroed after each full-gradient allocation so padding never carries garbage."""
        spans = sorted((off, off + shape.numel()) for off, shape in fb.index.values())
        gaps, cur = [], 0
        for s, e in spans:
            if s > cur:
                gaps.append((cur, s))
            cur = max(cur, e)
        if cur < fb.numel:
            gaps.append((cur, fb.numel))
        return gaps

    # ------------------------------------------------------------------ gather / reshard
    def _issue_gather(self, u, async_op: bool):
        st = u.state
        if self.no_shard:
            return
        if st["gathered"] or st["gather_work"] is not None:
            return
        works = []
        self.model.rctx.wait_param_ready(u.index)  # its shard may still be in the optimizer stream
        for fb in st["bufs"]:
            _alloc(fb.data, fb.nbytes)
            w = dist.all_gather_into_tensor(fb.data, fb.shard, group=self.pg, async_op=async_op)
            self.comm.issued("all_gather", w, fb.nbytes)
            works.append(w)
        if async_op:
            st["gather_work"] = works
        else:
            st["gathered"] = True

    def _wait_gather(self, u):
        st = u.state
        if st["gather_work"] is not None:
            with self.comm.waiting("all_gather"):
                for w in st["gather_work"]:
                    w.wait()
                    self.comm.completed(w)
            st["gather_work"] = None
            st["gathered"] = True
        if not st["gathered"]:
            with self.comm.waiting("all_gather"):
                self._issue_gather(u, async_op=False)

    def _reshard(self, u):
        st = u.state
        if self.no_shard:
            return
        if st["gather_work"] is not None:
            self._wait_gather(u)
        for fb in st["bufs"]:
            _free(fb.data)
        st["gathered"] = False

    def _size_prefetch(self):
        """Size the auto prefetch depth ONCE, at the first training forward, from the MAX of the
        ranks' token counts.  The depth decides how many all-gathers a rank issues before each
        reduce-scatter in backward, so it must be identical on every rank: sizing from a rank's
        own B*T (padded instruction batches differ per rank) would put the collectives of one
        RCCL group in different orders on different ranks.  Every rank reaches its first
        training forward at the same step (the loop is lockstep), so the one MAX all-reduce is
        collective-safe; later shape changes keep the depth."""
        if self._prefetch_tokens is not None:
            return
        rc = self.model.rctx
        if not (rc.grad_forward and self.model.training):
            return
        tokens = int(rc.B * rc.T)
        if not self.no_shard and self.world_size > 1:
            t = torch.tensor([tokens], dtype=torch.int64, device=self.device if self.is_cuda else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.pg)
            tokens = int(t.item())
        from .commplan import fsdp_prefetch_depth
        self._prefetch_tokens = tokens
        blocks = [u for u in self.units if u.name.startswith(("trf_blocks", "blocks"))] or self.units
        big = max(blocks, key=lambda u: sum(fb.numel for fb in u.state["bufs"]))
        numel = sum(fb.numel for fb in big.state["bufs"])
        nbytes = sum(fb.numel * fb.data.element_size() for fb in big.state["bufs"])
        self.prefetch = fsdp_prefetch_depth(nbytes, numel, tokens, self.world_size)

    # ------------------------------------------------------------------ warm-up adaptation
    MAX_PREFETCH = 4

    def adapt(self, step_ms: float) -> Optional[Dict]:
        """Called after a warm-up step with the comm stats of that step: if the exposed
        all-gather wait (MAX over ranks) exceeds ``ADAPT_FRAC`` of the step, gather one more
        unit ahead (each costs one gathered unit of HBM).  Every rank takes the same decision
        from the same MAX, so all ranks keep issuing the same collective order.  Replaces the
        link / FLOP-rate constants of ``commplan.fsdp_prefetch_depth`` with what the links did."""
        if self.no_shard:
            return None
        from .commstats import ADAPT_FRAC, max_over_ranks
        s = self.comm.summary()
        ag, step = max_over_ranks([s.get("all_gather", {}).get("ms", 0.0), step_ms], self.pg, self.device)
        rec = {"exposed_all_gather_ms": round(ag, 3), "step_ms": round(step, 2), "prefetch": self.prefetch}
        if ag > ADAPT_FRAC * step and self.prefetch < self.MAX_PREFETCH:
            self.prefetch += 1
            self.prefetch_auto = False   # measured, no longer sized from constants
            rec["prefetch_new"] = self.prefetch
        self.adapt_log.append(rec)
        return rec

    # ------------------------------------------------------------------ hooks
    def begin_micro_step(self, i: int, k: int):
        """Unsharded (``grad_shard is grad``): the kernels add in place from micro-step 1 on.
        Sharded: a unit's full gradient lives only from its ``pre_backward`` to the retire of its
        reduce-scatter, so every micro-step writes it afresh (accumulate off) and reduce-scatters
        it; the retire writes the gradient shard in micro-step 0 and adds into it afterwards.
        Holding full gradients across micro-steps would undo the sharding."""
        self._micro = i
        self.model.rctx.accumulate = self.no_shard and i > 0

    def pre_forward(self, unit):
        if self.prefetch_auto and unit.index == 0 and self._prefetch_tokens is None:
            self._size_prefetch()
        self._wait_gather(unit)
        for nxt in range(unit.index + 1, min(unit.index + 1 + self.prefetch, len(self.units))):
            self._issue_gather(self.units[nxt], async_op=True)

    def post_forward(self, unit):
        last = unit.index == len(self.units) - 1
        # (torch.is_grad_enabled() is False inside the units' autograd.Function.forward: the
        # model forward records whether it builds a backward)
        training = self.model.rctx.grad_forward and self.model.training
        if not training:  # eval / sampling: nothing is kept for a backward
            self._reshard(unit)
            return
        if self.reshard_after_forward and not last:
            self._reshard(unit)

    def pre_backward(self, unit):
        if not self._in_backward:
            self._in_backward = True
            self._rs_works = []
        self._wait_gather(unit)
        for prv in range(unit.index - 1, max(unit.index - 1 - self.prefetch, -1), -1):
            self._issue_gather(self.units[prv], async_op=True)
        fb = unit.train
        if fb is not None and not self.no_shard:
            _alloc(fb.grad, fb.grad_nbytes)
            for s, e in fb.gaps:
                fb.grad[s:e].zero_()

    def post_backward(self, unit):
        fb = unit.train
        if fb is not None and not self.no_shard:
            if self.reduce_dtype is not None or self._micro > 0:
                # reduce in the policy's dtype: cast the full gradient, reduce-scatter into a
                # reduce-dtype shard, cast back into the (param-dtype) gradient shard on retire.
                # Micro-steps after the first take the same route in any dtype: their shard is
                # added to the gradient shard on retire, so it cannot be scattered into it
                full = fb.grad.to(self.reduce_dtype) if self.reduce_dtype is not None else fb.grad
                part = torch.empty(fb.grad_shard.numel(), dtype=full.dtype, device=full.device)
                w = dist.reduce_scatter_tensor(part, full, group=self.pg, async_op=True)
                self.comm.issued("reduce_scatter", w, full.numel() * full.element_size())
                self._rs_works.append((w, fb, full, part, self._micro > 0))
            else:
                w = dist.reduce_scatter_tensor(fb.grad_shard, fb.grad, group=self.pg, async_op=True)
                self.comm.issued("reduce_scatter", w, fb.grad.numel() * fb.grad.element_size())
                self._rs_works.append((w, fb, None, None, False))
            # the full gradient is released only after the reduce-scatter completed: freeing it
            # now would hand the block back to the compute stream's allocator pool while RCCL
            # may still be reading it (288 GB leaves room to hold them until the end of backward)
            self._retire_rs(keep=2)
        self._reshard(unit)

    def _retire_rs(self, keep: int):
        """Wait for and free all but the ``keep`` most recent reduce-scatters (bounded memory
        without stalling the stream on the one just issued)."""
        while len(self._rs_works) > keep:
            w, fb, full, part, add = self._rs_works.pop(0)
            with self.comm.waiting("reduce_scatter"):
                w.wait()
            self.comm.completed(w)
            if add:
                fb.grad_shard.add_(part.to(fb.grad_shard.dtype))
            elif part is not None:
                fb.grad_shard.copy_(part)
            _free(fb.grad)

    def finish_backward(self):
        self._retire_rs(keep=0)
        self._in_backward = False

    # ------------------------------------------------------------------ optimizer
    def optimizer_slots(self, model):
        return [OptSlot(u.train.shard, u.train.grad_shard, u.name, (u.index,))
                for u in self.units if u.train is not None]

    def all_reduce_grad_sq_norm(self, sq: torch.Tensor) -> torch.Tensor:
        if not self.no_shard:
            with self.comm.waiting("all_reduce"):
                dist.all_reduce(sq, group=self.pg)
        return sq

    # the next forward starts with the embedding (1 GiB bf16 for Llama-3-8B) and the first
    # block: start their all-gathers as soon as their shards are updated, so they stream under
    # the remaining units' AdamW instead of stalling the first forward kernel
    prefetch_after_step = 2

    def after_slot_update(self, slot):
        if not self.is_cuda:
            return
        for ui in slot.units:
            if ui < self.prefetch_after_step:
                self._issue_gather(self.units[ui], async_op=True)

    # ------------------------------------------------------------------ inference
    @contextmanager
    def params_resident(self):
        """Gather every unit once for a multi-forward inference (KV-cache sampling) instead of
        re-gathering the whole model per generated token (reference X11: 200 full gathers per
        sample print)."""
        self.model.rctx.sync_all_params()
        for u in self.units:
            self._wait_gather(u)
        try:
            yield
        finally:
            for u in self.units:
                self._reshard(u)

    # ------------------------------------------------------------------ checkpoint
    @torch.no_grad()
    def load_full_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """Scatter a full (reference-named) state dict into this rank's shards, unit by unit
        (never more than one gathered unit alive).  Buffers (mask / cos / sin) are ignored:
        they are recomputed, never stored.  Call ``optimizer.reload_master()`` afterwards."""
        self.model.rctx.sync_all_params()
        names = {id(p): n for n, p in self.model.named_parameters()}
        missing = []
        W, r = self.world_size, self.rank
        for u in self.units:
            self._wait_gather(u)
            for fb in u.state["bufs"]:
                for p in fb.params:
                    k = names[id(p)]
                    if k not in sd:
                        missing.append(k)
                        continue
                    fb.view(fb.data, p).copy_(sd[k].to(dtype=fb.dtype).view(p.shape))
                if not self.no_shard:
                    n = fb.numel // W
                    fb.shard.copy_(fb.data[r * n:(r + 1) * n])
            self._reshard(u)
        if strict and missing:
            raise KeyError(f"missing keys in state dict: {missing[:8]}{'...' if len(missing) > 8 else ''}")

    def full_state_dict(self) -> Optional[Dict[str, torch.Tensor]]:
        """Gather unit by unit; rank 0 receives the reference-named CPU state dict."""
        self.model.rctx.sync_all_params()
        names = {id(p): n for n, p in self.model.named_parameters()}
        sd: Dict[str, torch.Tensor] = {}
        was_gathered = [u.state["gathered"] for u in self.units]
        for u in self.units:
            self._wait_gather(u)
            if self.rank == 0:
                for fb in u.state["bufs"]:
                    for p in fb.params:
                        sd[names[id(p)]] = fb.view(fb.data, p).detach().cpu().clone()
            self._reshard(u)
        for u, g in zip(self.units, was_gathered):
            if g:
                self._issue_gather(u, async_op=False)
        if self.rank != 0:
            return None
        ordered = {k: sd[k] for k in (n for n, _ in self.model.named_parameters()) if k in sd}
        for hook in self.model._state_dict_hooks.values():
            r = hook(self.model, ordered, "", None)
            if r is not None:
                ordered = r
        return ordered
