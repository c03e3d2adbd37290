"""Autoregressive sampling (reference generate.py:4-75).

Same contract: sliding window of ``context_size`` tokens, optional top-k threshold, temperature
+ multinomial (else greedy argmax), stop only when EVERY row emits ``eos_id``.

* :func:`generate` — recomputes the window per token like the reference, but only the last
  position goes through the LM head (``last_only=True``).
* :func:`generate_cached` — KV-cache decode: one prefill of the window, then one token per
  forward through the HIP decode-attention kernel over the cache (the window slides by
  re-prefilling, exactly reproducing the reference's conditioning).  Under FSDP the parameters
  are gathered once for the whole sample instead of once per token.  Tokens go into a
  preallocated buffer and the all-rows-eos stop test runs every ``EOS_CHECK_EVERY`` tokens (the
  output is cut at the first all-eos step, so the result is identical): the host never waits
  on the GPU per token, so each token's ~12 launches per layer queue up behind the previous
  token's kernels instead of running while the GPU idles.
* :func:`generate_ragged` — the batched form for prompts of different lengths (answering a set
  of instructions): one unpadded prefill of the packed prompts, then a decode step in which
  every row sits at its own position (``forward_cached_rows``: per-row RoPE / learned positions
  and the per-row decode-attention kernel) and stops on its own eos.  No sliding window.
* The cache may be as long as the model's context: decode attention over more than
  ``ops.DECODE_SPLIT_MIN`` (8,192) cached positions runs the split-KV kernels
  (``csrc/attn_decode_split.hip``), eagerly and inside the captured step alike.
* On the GPU the single-token step (every layer: norm, QKV GEMM, RoPE, K/V append + decode
  attention, projections, MLP, head) is captured ONCE per sample into a HIP graph
  (``torch.cuda.CUDAGraph``) with the position kept in device memory, and replayed per token:
  one graph launch instead of ~12 kernel launches per layer (the decode loop is launch-bound
  below Llama-3-8B size).  ``BLLM_DECODE_GRAPH=0`` runs it eagerly.
* ``seed=...`` switches :func:`generate_cached` / :func:`generate_ragged` from :func:`_sample`
  (one ``torch.multinomial`` over the batch from one generator) to the device sampler
  ``ops.sample_rows`` (csrc/sample.hip): temperature, top-k, top-p and a counter-based random
  stream per row, so a row's tokens depend on (seed, its stream id, its logits) and not on the
  batch it sits in.  In :func:`generate_ragged` the sampler is part of the captured step.
* ``speculative=K`` (:func:`generate_ragged`): exact speculative decoding.  A step feeds every row
  its last token and K prompt-lookup drafts (``forward_cached_rows(..., q_per_row=K + 1)``,
  ``ops.attn_extend_rows``), samples all K + 1 logits rows with the counters the plain loop would
  use and keeps the drafts the sampler confirms (``ops.spec_advance``): the plain loop's tokens in
  fewer steps, one graph replay per step (:class:`SpecDecodeGraph`).
"""
from __future__ import annotations

import os

from typing import Optional

import torch


def _sample(logits, temperature, top_k, generator):
    logits = logits.float()
    if top_k is not None:
        top, _ = torch.topk(logits, top_k)
        logits = torch.where(logits < top[:, -1:], torch.full_like(logits, float("-inf")), logits)
    if temperature > 0.0:
        probs = torch.softmax(logits / temperature, dim=-1)
        return torch.multinomial(probs, num_samples=1, generator=generator)
    return torch.argmax(logits, dim=-1, keepdim=True)


def _sampler_args(fn: str, B: int, temperature, top_k, top_p, seed, streams):
    """Entry check of the device sampler's arguments -> None (``seed is None``: :func:`_sample`
    runs) or (top_k, top_p, stream ids) in the form ``ops.sample_rows`` takes."""
    if seed is None:
        if top_p is not None or streams is not None:
            raise ValueError(f"{fn}: top_p and streams belong to the seeded device sampler; pass seed=...")
        return None
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"{fn}: seed must be an int, got {seed!r}")
    if not float(temperature) >= 0.0:
        raise ValueError(f"{fn}: temperature must be >= 0, got {temperature}")
    k = 0 if top_k is None else top_k
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError(f"{fn}: top_k must be None or an int >= 0 (0: off), got {top_k!r}")
    p = 1.0 if top_p is None else float(top_p)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"{fn}: top_p must be in (0, 1], got {top_p}")
    ids = list(range(B)) if streams is None else [int(v) for v in streams]
    if len(ids) != B or any(not -2 ** 63 <= v < 2 ** 63 for v in ids):
        raise ValueError(f"{fn}: streams must hold one 64-bit stream id per row ({B}), got {len(ids)}")
    return k, p, ids


EOS_CHECK_EVERY = int(os.environ.get("BLLM_EOS_CHECK_EVERY", "16"))


def _graph_enabled() -> bool:
    return os.environ.get("BLLM_DECODE_GRAPH", "1") != "0"


class DecodeGraph:
    """A model's single-token decode step (``forward_cached_dev``) captured into a HIP graph.
    Capture runs with the position set to the cache's LAST slot, so the warm-up / capture
    passes only write that slot, which every later decode step overwrites before reading it.
    They also READ the whole cache, which at this point is uninitialised beyond the prompt (at a
    long context most of it): their output is discarded, and the decode kernels do not care
    what the values are (NaNs included) -- they only must not be used."""

    def __init__(self, model, cache, B: int, device):
        Tmax = cache[0][0].shape[2]
        self.idx = torch.zeros(B, 1, dtype=torch.long, device=device)
        self.pos = torch.full((1,), Tmax - 1, dtype=torch.int32, device=device)
        cur = torch.cuda.current_stream(device)
        side = torch.cuda.Stream(device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):          # warm-up: hipBLASLt heuristics, allocator pool
            for _ in range(2):
                model.forward_cached_dev(self.idx, cache, self.pos)
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: the sample print runs mid-epoch while DataLoader worker / pin-memory
        # threads may make allocator or event calls; in "global" mode those would invalidate
        # (or be rejected during) this capture
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.logits = model.forward_cached_dev(self.idx, cache, self.pos)

    def step(self, idx_next: torch.Tensor, pos: int) -> torch.Tensor:
        self.idx.copy_(idx_next)
        self.pos.fill_(pos)
        self.graph.replay()
        return self.logits


@torch.no_grad()
def generate_cached(model, idx: torch.Tensor, max_new_tokens: int, context_size: int, temperature: float = 0.0,
                    top_k: Optional[int] = None, eos_id: Optional[int] = None,
                    generator: Optional[torch.Generator] = None, top_p: Optional[float] = None,
                    seed: Optional[int] = None, streams=None) -> torch.Tensor:
    """``seed`` (with ``top_p``, ``streams``: row b's stream id, default b): tokens come from
    ``ops.sample_rows`` instead of :func:`_sample`, called eagerly on each step's logits -- after
    the graph replay, not inside it: this loop feeds the step from the host (``DecodeGraph.step``
    copies the token and sets the position) and slides its window by re-prefilling.  Row b's
    counter runs over all its tokens, re-prefills included, so no uniform is used twice.  The stop
    rule and the sliding window are as without ``seed``."""
    from .. import ops
    sampler = _sampler_args("generate_cached", idx.shape[0], temperature, top_k, top_p, seed, streams)
    was_training = model.training
    model.eval()
    device = next(model.parameters()).device
    idx = idx.to(device)
    B, T0 = idx.shape
    out = torch.empty(B, T0 + max(max_new_tokens, 0), dtype=idx.dtype, device=device)
    out[:, :T0] = idx
    n = checked = T0
    if sampler is not None:
        stream_t = torch.tensor(sampler[2], dtype=torch.long).to(device)
        ctr = torch.zeros(B, dtype=torch.int32, device=device)    # row b has drawn ctr[b] tokens
        new_cols = out[:, T0:]
    eng = model.rctx.engine
    resident = eng.params_resident() if hasattr(eng, "params_resident") else _null()
    with resident:
        cache = model.new_kv_cache(B, context_size)
        cond = idx[:, -context_size:]
        logits = model.forward_cached(cond, cache, 0) if max_new_tokens > 0 else None
        pos = cond.shape[1]
        dec = None
        if max_new_tokens > 8 and _graph_enabled() and hasattr(model, "decode_graph_ok") \
                and model.decode_graph_ok(cache):
            logits = logits.clone()            # the prefill output must survive the capture
            dec = DecodeGraph(model, cache, B, device)
        for i in range(max_new_tokens):
            if sampler is not None:            # writes column ctr = i of new_cols, i.e. out[:, n]
                idx_next = ops.sample_rows(logits.contiguous(), stream_t, ctr, seed, temperature, sampler[0],
                                           sampler[1], out=new_cols)[:, None]
            else:
                idx_next = _sample(logits, temperature, top_k, generator)
                out[:, n] = idx_next[:, 0]
            n += 1
            last = i == max_new_tokens - 1
            if eos_id is not None and (n - checked >= EOS_CHECK_EVERY or last):
                # reference semantics (generate.py:68-70): stop before the first step at which
                # EVERY row sampled eos; later tokens were speculative and are dropped
                alleos = (out[:, checked:n] == eos_id).all(dim=0)
                if bool(alleos.any()):
                    n = checked + int(alleos.nonzero()[0, 0])
                    break
                checked = n
            if last:
                break
            if pos >= context_size:          # window full: slide by re-prefilling
                cond = out[:, n - context_size:n]
                logits = model.forward_cached(cond, cache, 0)
                pos = context_size
            elif dec is not None:
                logits = dec.step(idx_next, pos)
                pos += 1
            else:
                logits = model.forward_cached(idx_next, cache, pos)
                pos += 1
    model.train(was_training)
    return out[:, :n]


class RowsDecodeGraph:
    """:class:`DecodeGraph` for ``forward_cached_rows``: the positions are an int32 [B] vector in
    device memory that the replayed step reads and :meth:`step` advances there.  Captured with
    every position at the cache's last slot, as ``DecodeGraph`` does.

    ``sampler(logits, idx)`` (optional) is captured after the forward: it must pick the next token
    of every row on the device and write it into ``idx`` (``ops.sample_rows`` with
    ``next_idx=idx``); the position increment is captured too, so a token is one :meth:`replay`
    and nothing else.  It is not called during the warm-up passes, whose logits mean nothing."""

    def __init__(self, model, cache, pos: torch.Tensor, device, sampler=None, weights=None):
        B, Tmax = pos.numel(), cache[0][0].shape[2]
        kw = {} if weights is None else {"weights": weights}   # fp8 decode weights: warm-up and capture on them
        self.idx = torch.zeros(B, 1, dtype=torch.long, device=device)
        self.pos = torch.full((B,), Tmax - 1, dtype=torch.int32, device=device)
        cur = torch.cuda.current_stream(device)
        side = torch.cuda.Stream(device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                model.forward_cached_rows(self.idx, cache, self.pos, **kw)
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.logits = model.forward_cached_rows(self.idx, cache, self.pos, **kw)
            if sampler is not None:
                sampler(self.logits, self.idx)
                self.pos.add_(1)
        self.pos.copy_(pos)

    def replay(self) -> None:
        """One token of the forward + sampler graph: reads and rewrites ``idx``, advances ``pos``."""
        self.graph.replay()

    def step(self, idx_next: torch.Tensor) -> torch.Tensor:
        self.idx.copy_(idx_next)
        self.graph.replay()
        self.pos.add_(1)
        return self.logits


SPEC_NGRAM = 2      # n-gram length of the prompt-lookup drafts (ops.spec_advance)
SPEC_MAX_DRAFTS = 7  # drafts per step: the verify step's 1 + K tokens per row fit ops.attn_extend_rows


class SpecDecodeGraph:
    """One verify step of speculative decoding (:func:`generate_ragged`, ``speculative=K``), sibling
    of :class:`RowsDecodeGraph`: every row feeds Q = K + 1 tokens (its last emitted token and K
    drafts, ``idx`` int64 [B, Q]) at positions ``pos[b] ..``, and the step is

    * the position and counter vectors of the B*Q rows, ``pos[b] + j`` and ``ctr[b] + j``,
    * ``forward_cached_rows(..., q_per_row=Q)`` -> logits [B*Q, V],
    * ``ops.sample_rows`` on them with the row's stream and those counters: ``samp[b, j]`` is the
      token the plain loop would draw as the row's token number ``ctr[b] + j`` from these logits,
    * ``ops.spec_advance``: accept the confirmed drafts (tokens to ``out`` and ``hist``; ``pos``,
      ``ctr``, ``nsteps``, ``finished`` advance) and draft the next step's ``idx``.

    Everything lives on the device, so with ``capture`` the step is one HIP graph and
    :meth:`replay` one launch; without it the same calls run eagerly.  The warm-up passes run the
    forward alone with every row at the cache's last Q slots, which any later step overwrites
    before it reads them (the entry check of ``generate_ragged`` keeps the prompts below them)."""

    def __init__(self, model, cache, idx, hist, h0, pos, ctr, nsteps, finished, out, stream, seed: int,
                 temperature: float, top_k: int, top_p: float, eos_id: int, capture: bool = True):
        from .. import ops
        B, Q = idx.shape
        device = idx.device
        Tmax = cache[0][0].shape[2]
        j = torch.arange(Q, dtype=torch.int32, device=device)
        stream_rows = stream.repeat_interleave(Q)

        def step():
            pos_rows = (pos[:, None] + j).reshape(-1)
            ctr_rows = (ctr[:, None] + j).reshape(-1)
            logits = model.forward_cached_rows(idx.view(B * Q, 1), cache, pos_rows, q_per_row=Q)
            samp = ops.sample_rows(logits.contiguous(), stream_rows, ctr_rows, seed, temperature, top_k, top_p)
            ops.spec_advance(idx, samp.view(B, Q), hist, h0, pos, ctr, nsteps, finished, out, eos_id, SPEC_NGRAM)
            return logits

        self._step = step
        self.graph = None
        self.logits = None
        if not capture:
            return
        warm = torch.full((B * Q,), Tmax - Q, dtype=torch.int32, device=device) + j.repeat(B)
        cur = torch.cuda.current_stream(device)
        side = torch.cuda.Stream(device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                model.forward_cached_rows(idx.view(B * Q, 1), cache, warm, q_per_row=Q)
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.logits = step()

    def replay(self) -> None:
        """One verify step: reads and rewrites the state tensors given at construction."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self.logits = self._step()


def _spec_args(K, B: int, temperature, seed, kv_dtype, weight_dtype, draft_hints):
    """Entry check of ``generate_ragged``'s speculative arguments -> K (0: off)."""
    if K is None:
        if draft_hints is not None:
            raise ValueError("generate_ragged: draft_hints belong to speculative decoding; pass speculative=K")
        return 0
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= SPEC_MAX_DRAFTS:
        raise ValueError(f"generate_ragged: speculative must be None or an int in 1..{SPEC_MAX_DRAFTS}, got {K!r}")
    if seed is None and float(temperature) != 0.0:
        raise ValueError("generate_ragged: speculative decoding verifies drafts with the seeded device sampler; "
                         "pass seed=... or temperature=0 (one multinomial over the batch cannot be verified)")
    if kv_dtype is not None or weight_dtype is not None:
        raise ValueError("generate_ragged: speculative decoding runs on the default cache and weights "
                         "(no kv_dtype / weight_dtype)")
    if draft_hints is not None:
        if not isinstance(draft_hints, (list, tuple)) or len(draft_hints) != B:
            raise ValueError(f"generate_ragged: draft_hints must hold one entry per prompt ({B})")
        for b, h in enumerate(draft_hints):
            if h is not None and (not isinstance(h, torch.Tensor) or h.dim() != 1 or h.dtype != torch.long):
                raise ValueError(f"generate_ragged: draft hint {b} must be None or a 1-D LongTensor")
    return K


@torch.no_grad()
def generate_ragged(model, prompts, max_new_tokens: int, context_size: int, temperature: float = 0.0,
                    top_k: Optional[int] = None, eos_id: Optional[int] = None,
                    generator: Optional[torch.Generator] = None, top_p: Optional[float] = None,
                    seed: Optional[int] = None, streams=None, kv_dtype: Optional[str] = None,
                    weight_dtype=None, speculative: Optional[int] = None, draft_hints=None,
                    stats: Optional[dict] = None) -> list:
    """Batched KV-cache generation from prompts of different lengths.

    ``prompts``: a non-empty list of non-empty 1-D LongTensors.  Returns one 1-D tensor per prompt:
    the prompt followed by that row's new tokens up to, not including, its first ``eos_id``, at
    most ``max_new_tokens`` of them.  A row stops on its own eos (unlike :func:`generate_cached`,
    which stops when every row emits eos at the same step); the loop ends once every row has.

    ``max(len) + max_new_tokens <= context_size <= the model's context length`` is required
    (ValueError otherwise, before any device work): there is no sliding window here, and this
    check is what keeps every device-side position inside the KV cache and the position tables.

    One unpadded prefill of the packed prompts (``forward_prefill_ragged``), then one
    ``forward_cached_rows`` step per token, with the positions and the finished mask in device
    memory: the host reads the mask every ``EOS_CHECK_EVERY`` tokens and never waits per token.
    On the GPU the step is captured once into a HIP graph and replayed (``BLLM_DECODE_GRAPH=0``:
    eager), as in :func:`generate_cached`.

    Greedy (``temperature == 0``): row b is what ``generate_cached(model, prompts[b][None], ...)``
    gives alone, up to GEMM rounding.  Sampling without ``seed`` draws ONE multinomial over the
    [B, V] probabilities per step, so a row's draws depend on which rows share its batch.

    ``seed`` (an int) selects the device sampler ``ops.sample_rows`` instead: ``temperature``,
    ``top_k`` (None / 0: off), ``top_p`` (None / 1: off; needs ``seed``) and one counter-based
    random stream per row, ``streams[b]`` (default b), whose counter is the row's token count.
    Row b's tokens are then a function of (seed, streams[b], row b's logits): the same prompt under
    the same stream id gives the same answer in any batch, up to GEMM rounding of the logits.  The
    first token is sampled eagerly from the prefill logits; after it the captured step is forward
    + sampler, which writes the next input token, the output column and the finished mask on the
    device, so the host loop is one graph replay per token (eager mode: the same two calls).

    ``kv_dtype="fp8"`` keeps the KV cache as e4m3fn bytes with one fp32 scale per (row, kv head,
    position) (``model.new_kv_cache``): about half the cache bytes.  The prefill attention still
    runs on the exact K / V of the packed rows; what is stored, and what every later step attends
    over, is quantised, so the tokens can differ from the default cache's.  None: the cache in the
    parameter dtype, as before.

    ``weight_dtype="fp8"`` runs every decode step's projections, the head's included, on fp8
    packs of the weights (``model.new_decode_weights``: e4m3fn bytes, one scale per output
    channel, LoRA folded in; ``ops.linear_w8``), built once inside the call; a pack the caller
    built already (``model.new_decode_weights()``) is taken as it is.  The prefill runs on the
    model's own weights, so the first new token comes from exact logits; every later one from the
    quantised weights, so the tokens can differ from the default's.  The packs are extra memory,
    about half the bytes of 16-bit weights.  None: the model's weights, as before.

    ``weight_dtype="mxfp4"`` is the same on MXFP4 packs (``ops.linear_w4``: e2m1 codes, one
    power-of-two scale per 32 consecutive k, 0.53 of the fp8 bytes) for every projection group
    whose K is a multiple of 128; the other groups and the head keep their fp8 packs.  Its
    quantisation error is larger than fp8's, so more tokens can differ from the default's.

    ``speculative=K`` (1..7): exact speculative decoding with prompt-lookup drafts.  After the
    first token every step feeds each row its last token and K drafts -- the continuation of the
    latest earlier occurrence of the row's trailing ``SPEC_NGRAM`` tokens in its own text, or in
    ``draft_hints[b]`` (a 1-D LongTensor or None per prompt, searched as if it stood ahead of the
    prompt) -- through one ``forward_cached_rows(..., q_per_row=K + 1)``, runs the device sampler
    on all K + 1 logits rows with the counters the plain loop would use, and keeps the drafts the
    sampler confirms plus one more token (:class:`SpecDecodeGraph`; one graph replay per step, the
    host reads the finished mask every ``EOS_CHECK_EVERY`` steps).  A row's token number c is a
    function of (seed, stream, c, logits) either way, so the answers are those of
    ``speculative=None`` up to GEMM rounding of the logits; drafts and hints change the number
    of steps, never the tokens.  It needs the device sampler (``seed``, or ``temperature == 0``:
    greedy through ``sample_rows``), the default cache and weights, and
    ``max(len) + max_new_tokens + K <= context_size``: a verify step writes K cache rows past the
    position.  ``stats`` (a dict) receives ``steps`` (verify steps per prompt) and ``new_tokens``
    (tokens drawn per prompt, an eos included)."""
    from .. import ops
    from ..models.base import DecodeWeights, pack_prompts
    if kv_dtype not in (None, "fp8"):
        raise ValueError(f"generate_ragged: kv_dtype must be None or 'fp8', got {kv_dtype!r}")
    if weight_dtype is not None and weight_dtype not in ("fp8", "mxfp4") and not isinstance(weight_dtype, DecodeWeights):
        raise ValueError("generate_ragged: weight_dtype must be None, 'fp8', 'mxfp4' or the model's "
                         f"new_decode_weights(), got {weight_dtype!r}")
    if not isinstance(prompts, (list, tuple)) or len(prompts) == 0:
        raise ValueError("generate_ragged: prompts must be a non-empty list of 1-D token tensors")
    for b, p in enumerate(prompts):
        if not isinstance(p, torch.Tensor) or p.dim() != 1 or p.numel() == 0 or p.dtype != torch.long:
            raise ValueError(f"generate_ragged: prompt {b} must be a non-empty 1-D LongTensor")
    lens = [int(p.numel()) for p in prompts]
    new = max(int(max_new_tokens), 0)
    K = _spec_args(speculative, len(prompts), temperature, seed, kv_dtype, weight_dtype, draft_hints)
    if K and max(lens) + new + K > context_size:
        raise ValueError(f"generate_ragged: the longest prompt ({max(lens)} tokens) + max_new_tokens ({new}) + "
                         f"speculative ({K}) exceeds context_size ({context_size}): a verify step writes K cache "
                         f"rows past the position")
    if max(lens) + new > context_size:
        raise ValueError(f"generate_ragged: the longest prompt ({max(lens)} tokens) + max_new_tokens ({new}) "
                         f"exceeds context_size ({context_size}); this path has no sliding window")
    if context_size > model.cfg.context_length:
        raise ValueError(f"generate_ragged: context_size ({context_size}) exceeds the model's context length "
                         f"({model.cfg.context_length})")
    if K and seed is None:      # greedy through the device sampler: at temperature 0 it is the argmax
        seed, top_k, top_p = 0, None, None
    sampler = _sampler_args("generate_ragged", len(prompts), temperature, top_k, top_p, seed, streams)
    device = next(model.parameters()).device
    if new == 0:
        if stats is not None:
            stats["steps"], stats["new_tokens"] = [0] * len(prompts), [0] * len(prompts)
        return [p.to(device) for p in prompts]
    was_training = model.training
    model.eval()
    B = len(prompts)
    idx, seq = pack_prompts(prompts, device)
    out = torch.zeros(B, new, dtype=torch.long, device=device)
    pos = torch.tensor(lens, dtype=torch.int32).to(device)           # row b's next position
    finished = torch.zeros(B, dtype=torch.bool, device=device)
    n = checked = 0
    eng = model.rctx.engine
    resident = eng.params_resident() if hasattr(eng, "params_resident") else _null()
    with resident:
        cache = model.new_kv_cache(B, context_size) if kv_dtype is None else \
            model.new_kv_cache(B, context_size, kv_dtype=kv_dtype)
        logits = model.forward_prefill_ragged(idx, seq, cache)
        dec = None
        kw = {}
        if weight_dtype is not None:
            kw["weights"] = model.new_decode_weights(weight_dtype) if isinstance(weight_dtype, str) else weight_dtype
        if sampler is not None:
            stream_t = torch.tensor(sampler[2], dtype=torch.long).to(device)
            ctr = torch.zeros(B, dtype=torch.int32, device=device)    # row b has drawn ctr[b] tokens
            eos = -1 if eos_id is None else int(eos_id)

            def draw(lg, nxt):     # token -> nxt, out[:, ctr], finished; ctr += 1 (ctr < new: one call per column)
                return ops.sample_rows(lg.contiguous(), stream_t, ctr, seed, temperature, sampler[0], sampler[1],
                                       eos_id=eos, next_idx=nxt, out=out, finished=finished)

            nxt = torch.zeros(B, 1, dtype=torch.long, device=device)
            draw(logits, nxt)
            n = 1
            if K:
                n = _speculate(model, cache, prompts, lens, draft_hints, K, nxt, pos, ctr, finished, out, stream_t,
                               seed, temperature, sampler, eos, stats)
            if not K and new > 8 and _graph_enabled() and model.decode_graph_ok(cache):
                dec = RowsDecodeGraph(model, cache, pos, device, sampler=draw, **kw)
                dec.idx.copy_(nxt)
            while not K and n < new:
                if eos_id is not None and n - checked >= EOS_CHECK_EVERY:
                    if bool(finished.all()):   # tokens after a row's first eos are dropped below
                        break
                    checked = n
                if dec is not None:
                    dec.replay()
                else:
                    logits = model.forward_cached_rows(nxt, cache, pos, **kw)
                    pos += 1
                    draw(logits, nxt)
                n += 1
        elif new > 8 and _graph_enabled() and model.decode_graph_ok(cache):
            logits = logits.clone()            # the prefill output must survive the capture
            dec = RowsDecodeGraph(model, cache, pos, device, **kw)
        for i in range(new if sampler is None else 0):
            idx_next = _sample(logits, temperature, top_k, generator)
            out[:, i] = idx_next[:, 0]
            n = i + 1
            if n == new:
                break
            if eos_id is not None:
                finished |= idx_next[:, 0] == eos_id
                if n - checked >= EOS_CHECK_EVERY:
                    if bool(finished.all()):   # tokens after a row's first eos are dropped below
                        break
                    checked = n
            if dec is not None:
                logits = dec.step(idx_next)
            else:
                logits = model.forward_cached_rows(idx_next, cache, pos, **kw)
                pos += 1
    gen = out[:, :n]
    if eos_id is not None:
        is_eos = gen == eos_id
        keep = torch.where(is_eos.any(dim=1), is_eos.to(torch.int64).argmax(dim=1), n).tolist()
    else:
        keep = [n] * B
    model.train(was_training)
    return [torch.cat((idx[seq.bounds[b]:seq.bounds[b + 1]], gen[b, :keep[b]])) for b in range(B)]


def spec_state(prompts, lens, hints, Q: int, new: int, first, pos):
    """The device-side state of the speculative loop after the first token (``first`` [B, 1] at
    positions ``pos``, int32 [B] on the device) -> (idx int64 [B, Q] zeros, hist int32 [B, Lh],
    h0 int32 [B], nsteps int32 [B] zeros).  Corpus row b: its hint, its prompt, the first token,
    and room for the answer and one step's tokens."""
    B, device = len(prompts), first.device
    hints = [None] * B if hints is None else hints
    hl = [0 if h is None else int(h.numel()) for h in hints]
    Lh = max(h + n for h, n in zip(hl, lens)) + new + Q
    host = torch.zeros(B, Lh, dtype=torch.int32)
    for b in range(B):
        if hl[b]:
            host[b, :hl[b]] = hints[b].to("cpu", torch.int32)
        host[b, hl[b]:hl[b] + lens[b]] = prompts[b].to("cpu", torch.int32)
    hist = host.to(device)
    h0 = torch.tensor(hl, dtype=torch.int32).to(device)
    # pos[b]: the position of the row's last emitted token, which is the next step's first input
    hist[torch.arange(B, device=device), (h0 + pos).to(torch.long)] = first[:, 0].to(torch.int32)
    return (torch.zeros(B, Q, dtype=torch.long, device=device), hist, h0,
            torch.zeros(B, dtype=torch.int32, device=device))


def _speculate(model, cache, prompts, lens, hints, K: int, first, pos, ctr, finished, out, stream_t, seed,
               temperature, sampler, eos: int, stats) -> int:
    """The speculative decode loop of :func:`generate_ragged` after the first token (``first``
    [B, 1], already in ``out[:, 0]``, ``ctr`` = 1): builds the rows' corpora, drafts, and runs at
    most ``new - 1`` verify steps.  Returns the number of valid columns of ``out`` (all of them:
    every row ends finished or with ``new`` tokens)."""
    from .. import ops
    new = out.shape[1]
    idx, hist, h0, nsteps = spec_state(prompts, lens, hints, K + 1, new, first, pos)
    finished |= ctr >= new                      # new == 1: the first token was the answer
    ops.spec_advance(idx, idx.clone(), hist, h0, pos, ctr, nsteps, finished, out, eos, SPEC_NGRAM, accept=False)
    capture = new > 8 and _graph_enabled() and model.decode_graph_ok(cache)
    dec = SpecDecodeGraph(model, cache, idx, hist, h0, pos, ctr, nsteps, finished, out, stream_t, seed, temperature,
                          sampler[0], sampler[1], eos, capture=capture)
    for i in range(new - 1):
        if i and i % EOS_CHECK_EVERY == 0 and bool(finished.all()):
            break
        dec.replay()
    if stats is not None:
        stats["steps"], stats["new_tokens"] = nsteps.tolist(), ctr.tolist()
    return new


@torch.no_grad()
def generate_continuous(model, prompts, max_new_tokens, context_size: int, slots: int, eos_id: Optional[int] = None,
                        temperature: float = 0.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                        seed: Optional[int] = None, streams=None, kv_dtype: Optional[str] = None, weight_dtype=None,
                        stats: Optional[dict] = None) -> list:
    """Continuous batching: :func:`generate_ragged`'s answers for a prompt list of any length from
    ``slots`` cache rows that never idle -- a row whose answer is done is handed to the next
    waiting prompt while the others keep decoding.  Returns one 1-D tensor per prompt, the prompt
    followed by its answer, cut before the first ``eos_id``.

    ``max_new_tokens``: an int, or one int per prompt (prompt i draws at most ``n_i`` tokens; with
    ``n_i == 0`` it comes back as it is and never takes a slot).  The device sampler
    ``ops.sample_rows`` is the only sampler (there is no ``generator`` argument): prompt i draws
    from stream ``streams[i]`` (default i) with its own token counter, so its answer is a function
    of (seed, stream, its logits) and does not depend on the slot it ran in, on when it was
    admitted or on its neighbours, up to GEMM rounding of the logits.  Without ``seed`` the call
    runs ``seed = 0`` at temperature 0, the argmax.  ``kv_dtype`` / ``weight_dtype``: as in
    :func:`generate_ragged` -- every admission prefill runs on the model's own weights, every
    decode step on the packs.  No speculation here.

    One cache of ``slots`` rows x ``context_size`` positions is allocated once; where
    ``decode_graph_ok`` holds one :class:`RowsDecodeGraph` (forward + sampler + position increment)
    is captured after the first admission and replayed for the whole call, elsewhere (CPU, fp32,
    ``BLLM_DECODE_GRAPH=0``) the same loop runs the step eagerly.  Parameters stay resident.

    The schedule.  E = ``EOS_CHECK_EVERY``; d = tokens an occupied slot has drawn, known on the host
    without a read: 1 after admission, + 1 per replay; n = its prompt's budget.  Repeat:

    1. Admit.  While slots are free and prompts wait, the lowest free slot takes the next prompt in
       the caller's order.  A round's admissions are one packed prefill
       (``forward_prefill_ragged(..., rows=)``), one ``sample_rows`` over its [n, V] logits (the
       prompts' streams, counters 0) and a scatter into the slot state: next token, position =
       prompt length, counter = 1, stream id, finished flag, column 0 of the slot's output row.
    2. Run.  ``run = min(E, min over occupied slots of (n - d))`` replays (or eager steps).
    3. Look.  With ``eos_id``, the occupied slots' finished flags are read once.
    4. Retire every occupied slot with ``d == n`` or its flag set: its output row is copied out;
       the answer is the tokens before the first eos, at most n.
    5. Park.  Free slots nothing waits for keep stepping (the graph has ``slots`` rows): before
       every run their position and counter are rewritten to 0.
    6. Stop when no slot is occupied and no prompt waits.

    Invariants.  (a) A slot's position stays below ``len + n <= context_size <= `` the model's
    context (entry check; step 2 never runs a slot past d = n; a parked slot restarts from 0 and
    ``run < context_size``), so no cache row or position-table entry out of range is touched.
    (b) No answer token is overwritten: a slot writes output column d - 1 < n once, and is not
    stepped past its budget (the sampler's column clamp never acts on an occupied slot).  (c) A new
    occupant never sees its predecessor: it attends over keys 0..pos only; the admission fill
    rewrote positions below its prompt length and each later position is appended before it is
    read.  (d) The kernels, :class:`RowsDecodeGraph`, :func:`generate_ragged` and
    :func:`generate_cached` are used as they are.

    ``stats`` (a dict) receives ``replays``, ``prefills`` and per prompt ``steps`` (replays while it
    held a slot), ``slot`` (None: never took one) and ``new_tokens`` (tokens of its answer, its eos
    included when it drew one).

    ValueError before any work: ``slots < 1``; a budget list of the wrong length or a negative
    budget; an empty prompt; ``len + n_i > context_size``; ``context_size`` beyond the model's;
    a temperature without ``seed``."""
    from .. import ops
    from ..models.base import DecodeWeights, pack_prompts
    fn = "generate_continuous"
    if kv_dtype not in (None, "fp8"):
        raise ValueError(f"{fn}: kv_dtype must be None or 'fp8', got {kv_dtype!r}")
    if weight_dtype is not None and weight_dtype not in ("fp8", "mxfp4") and not isinstance(weight_dtype, DecodeWeights):
        raise ValueError(f"{fn}: weight_dtype must be None, 'fp8', 'mxfp4' or the model's new_decode_weights(), got "
                         f"{weight_dtype!r}")
    if isinstance(slots, bool) or not isinstance(slots, int) or slots < 1:
        raise ValueError(f"{fn}: slots must be an int >= 1, got {slots!r}")
    if not isinstance(prompts, (list, tuple)) or len(prompts) == 0:
        raise ValueError(f"{fn}: prompts must be a non-empty list of 1-D token tensors")
    for b, p in enumerate(prompts):
        if not isinstance(p, torch.Tensor) or p.dim() != 1 or p.numel() == 0 or p.dtype != torch.long:
            raise ValueError(f"{fn}: prompt {b} must be a non-empty 1-D LongTensor")
    P = len(prompts)
    lens = [int(p.numel()) for p in prompts]
    if isinstance(max_new_tokens, (list, tuple)):
        budgets = list(max_new_tokens)
        if len(budgets) != P:
            raise ValueError(f"{fn}: max_new_tokens must be an int or one int per prompt ({P}), got {len(budgets)}")
    else:
        budgets = [max_new_tokens] * P
    if any(isinstance(n, bool) or not isinstance(n, int) or n < 0 for n in budgets):
        raise ValueError(f"{fn}: every budget must be an int >= 0, got {max_new_tokens!r}")
    for b in range(P):
        if lens[b] + budgets[b] > context_size:
            raise ValueError(f"{fn}: prompt {b} ({lens[b]} tokens) + its budget ({budgets[b]}) exceeds context_size "
                             f"({context_size}); this path has no sliding window")
    if context_size > model.cfg.context_length:
        raise ValueError(f"{fn}: context_size ({context_size}) exceeds the model's context length "
                         f"({model.cfg.context_length})")
    if seed is None:
        if float(temperature) != 0.0:
            raise ValueError(f"{fn}: the seeded device sampler is the only one here; pass seed=... with a temperature")
        seed, top_k, top_p = 0, None, None   # greedy through the device sampler: at temperature 0 it is the argmax
    top_k, top_p, stream_ids = _sampler_args(fn, P, temperature, top_k, top_p, seed, streams)
    device = next(model.parameters()).device
    E = max(EOS_CHECK_EVERY, 1)
    eos = -1 if eos_id is None else int(eos_id)
    maxn = max(budgets)
    st = {"replays": 0, "prefills": 0, "steps": [0] * P, "slot": [None] * P, "new_tokens": [0] * P}
    gens = [None] * P                           # per prompt: its output row's first n_i columns, on the device
    waiting = [i for i in range(P) if budgets[i] > 0]
    was_training = model.training
    model.eval()
    eng = model.rctx.engine
    resident = eng.params_resident() if hasattr(eng, "params_resident") else _null()
    with resident:
        if waiting:
            cache = model.new_kv_cache(slots, context_size) if kv_dtype is None else \
                model.new_kv_cache(slots, context_size, kv_dtype=kv_dtype)
            kw = {}
            if weight_dtype is not None:
                kw["weights"] = model.new_decode_weights(weight_dtype) if isinstance(weight_dtype, str) \
                    else weight_dtype
            # the slot state, all on the device and read by the replayed step
            nxt = torch.zeros(slots, 1, dtype=torch.long, device=device)      # next input token
            pos = torch.zeros(slots, dtype=torch.int32, device=device)        # next position
            ctr = torch.zeros(slots, dtype=torch.int32, device=device)        # tokens drawn = next output column
            stream_t = torch.zeros(slots, dtype=torch.long, device=device)
            finished = torch.zeros(slots, dtype=torch.bool, device=device)
            out = torch.zeros(slots, maxn, dtype=torch.long, device=device)

            def draw(lg, nx):
                return ops.sample_rows(lg.contiguous(), stream_t, ctr, seed, temperature, top_k, top_p, eos_id=eos,
                                       next_idx=nx, out=out, finished=finished)

        dec = None
        occ = {}                                # slot -> [prompt, d]
        parked, parked_t = None, None
        head = 0
        while occ or head < len(waiting):
            # 1. admit
            free = [s for s in range(slots) if s not in occ]
            adm = []
            while free and head < len(waiting):
                adm.append((free.pop(0), waiting[head]))
                head += 1
            if adm:
                rows = [s for s, _ in adm]
                idx, seq = pack_prompts([prompts[i] for _, i in adm], device)
                logits = model.forward_prefill_ragged(idx, seq, cache, rows=rows)
                meta = torch.tensor([rows, [lens[i] for _, i in adm], [stream_ids[i] for _, i in adm]],
                                    dtype=torch.long).to(device)
                fin = torch.zeros(len(adm), dtype=torch.bool, device=device)
                tok = ops.sample_rows(logits.contiguous(), meta[2].contiguous(),
                                      torch.zeros(len(adm), dtype=torch.int32, device=device), seed, temperature,
                                      top_k, top_p, eos_id=eos, finished=fin)
                nxt.index_copy_(0, meta[0], tok[:, None])
                pos.index_copy_(0, meta[0], meta[1].to(torch.int32))
                ctr.index_fill_(0, meta[0], 1)
                stream_t.index_copy_(0, meta[0], meta[2])
                finished.index_copy_(0, meta[0], fin)
                out[:, 0].index_copy_(0, meta[0], tok)
                for s, i in adm:
                    occ[s] = [i, 1]
                    st["slot"][i] = s
                st["prefills"] += 1
                if dec is None and maxn > 8 and _graph_enabled() and model.decode_graph_ok(cache):
                    dec = RowsDecodeGraph(model, cache, pos, device, sampler=draw, **kw)
                    dec.idx.copy_(nxt)
                    nxt, pos = dec.idx, dec.pos     # the captured step reads and advances these
            # 2. run (5: free slots restart from position and counter 0)
            run = min(E, min(budgets[i] - d for i, d in occ.values()))
            if run > 0:
                free = [s for s in range(slots) if s not in occ]
                if free:
                    if free != parked:
                        parked, parked_t = free, torch.tensor(free, dtype=torch.long).to(device)
                    pos.index_fill_(0, parked_t, 0)
                    ctr.index_fill_(0, parked_t, 0)
                for _ in range(run):
                    if dec is not None:
                        dec.replay()
                    else:
                        logits = model.forward_cached_rows(nxt, cache, pos, **kw)
                        pos += 1
                        draw(logits, nxt)
                st["replays"] += run
                for v in occ.values():
                    v[1] += run
            # 3. look
            flags = finished.tolist() if eos_id is not None else None
            # 4. retire
            for s in sorted(occ):
                i, d = occ[s]
                if d == budgets[i] or (flags is not None and flags[s]):
                    gens[i] = out[s, :d].clone()
                    st["steps"][i] = d - 1
                    del occ[s]
        # the cut before each answer's first eos: one host read for the whole call
        keep = [0 if g is None else int(g.numel()) for g in gens]
        if eos_id is not None and any(keep):
            flat = (torch.cat([g for g in gens if g is not None]) == eos_id).tolist()
            o = 0
            for i in range(P):
                row = flat[o:o + keep[i]]
                o += keep[i]
                if True in row:
                    keep[i] = row.index(True)
                    st["new_tokens"][i] = keep[i] + 1
                else:
                    st["new_tokens"][i] = keep[i]
        else:
            st["new_tokens"] = list(keep)
    model.train(was_training)
    if stats is not None:
        stats.update(st)
    return [p.to(device) if g is None else torch.cat((p.to(device), g[:k])) for p, g, k in zip(prompts, gens, keep)]


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


@torch.no_grad()
def generate(model, idx: torch.Tensor, max_new_tokens: int, context_size: int, temperature: float = 0.0,
             top_k: Optional[int] = None, eos_id: Optional[int] = None,
             generator: Optional[torch.Generator] = None) -> torch.Tensor:
    was_training = model.training
    model.eval()
    device = next(model.parameters()).device
    idx = idx.to(device)
    for _ in range(max_new_tokens):
        idx_cond = idx[:, -context_size:]
        logits = model(idx_cond, last_only=True)[:, -1, :].float()
        if top_k is not None:
            top, _ = torch.topk(logits, top_k)
            logits = torch.where(logits < top[:, -1:], torch.full_like(logits, float("-inf")), logits)
        if temperature > 0.0:
            probs = torch.softmax(logits / temperature, dim=-1)
            idx_next = torch.multinomial(probs, num_samples=1, generator=generator)
        else:
            idx_next = torch.argmax(logits, dim=-1, keepdim=True)
        if eos_id is not None and bool((idx_next == eos_id).all()):
            break
        idx = torch.cat((idx, idx_next), dim=1)
    model.train(was_training)
    return idx
