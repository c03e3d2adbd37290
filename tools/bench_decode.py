#!/usr/bin/env python3
"""Sampling / decode benchmark (GPU): the Trainer's sample print (reference train.py:213-229:
200 new tokens, top-k 5, temperature 1) on random-init weights, KV-cache decode
(train/generate.py:generate_cached).  Prints ms per generated token and tokens/s.
Usage: python tools/bench_decode.py [--model llama3 --num_params 8B] [--tokens 200] [--graph 0|1]

``--ragged B1,B2,...``: answering B instructions.  The prompts are the first B records of the
synthetic Alpaca file in the ``--finetune`` prompt format, tokenised with the model's tokenizer;
``generate_ragged`` on all B (A) against B one-row ``generate_cached`` runs over the same prompts
(B, the only way before), greedy without eos, ``--tokens`` new tokens each, in one process,
interleaved A B A B, ``--repeats`` times after one warm-up of each.  Per batch size one JSON line
(and one entry of ``--out FILE``): median and range of ms per generated token (wall time over
all B x tokens tokens) and responses/s.
Usage: python tools/bench_decode.py --model llama3_2 --num_params 1B --ragged 1,8,32 --tokens 128

``--ragged ... --temperature T [--top_k K] [--top_p P] [--seed S]``: what sampling costs.  Three
``generate_ragged`` arms over the same prompts, interleaved in one process: greedy, the torch
composition (``_sample``: topk / softmax / multinomial from one generator after each replay; left
out when ``--top_p`` < 1, which it cannot do) and the device sampler (``seed=S``: csrc/sample.hip
inside the replayed step).  Median and range of ms per generated token per arm.

``--context N``: the model's context and the KV cache's length (the registry's Llama-3.1 / 3.2
contexts go to 131,072).  ``generate_cached``, greedy, ``--batch`` rows of ``--prompt`` random
tokens, ``--tokens`` new tokens, arms interleaved in one process ``--repeats`` times after one
warm-up of each.  Up to 8,192 positions the arms are the single-launch decode-attention kernel
and the split-KV kernels forced through ``ops.DECODE_SPLIT_MIN = 0``; past that the arms are
graph replay (the append op: split-KV at every position of such a cache) and the eager loop (the
plain op, which goes by the number of keys: single-launch up to 8,192 keys, split-KV beyond).  One JSON line: median and range
of ms per generated token per arm (prefill included in the wall time, and reported on its own).
Usage: python tools/bench_decode.py --model llama3_2 --num_params 1B --context 32768 --prompt 200

``--context N --kv_dtype fp8``: the cache format instead.  ``generate_ragged``, greedy, graph replay,
``--batch`` rows of ``--prompt`` random tokens: the cache in the parameter dtype against the fp8
cache, interleaved as above; ``--kv_arms fp8`` runs the fp8 arm alone (a batch whose bf16 cache
does not fit).  One JSON line: ms per generated token per arm (``kv_model``, ``kv_fp8``), and each arm's
cache bytes.
Usage: python tools/bench_decode.py --model llama3_2 --num_params 1B --context 32768 --prompt 8192 --kv_dtype fp8

``--ragged B,... --weight_dtype fp8`` (``--lora_rank R``: on a LoRA model): the decode steps on fp8
weight packs (``ops.linear_w8``) against the model's own weights, interleaved (``ragged_weights``).
Usage: python tools/bench_decode.py --model llama3_2 --num_params 1B --ragged 1,8,32 --tokens 128 --weight_dtype fp8

``--ragged B,... --speculative K1,K2,... [--hints self]``: exact speculative decoding
(``generate_ragged(speculative=K)``) against the plain loop, both greedy through the device sampler
(``seed=0``), interleaved (``ragged_speculative``).  Without hints a random-init model accepts next to
no draft: the overhead of a verify step.  ``--hints self`` adds arms whose hint is each prompt
followed by its own answer: nearly every draft accepted, the ceiling.  The answer is the one the
unhinted arm of the same K gave (``--hints plain``: the plain loop's; in bf16 a random-init model's
near-tied logits round differently in a 1-token and a (K + 1)-token step, the two answers part after
some tokens and the hint stops matching there).  Per arm: ms per generated token, verify steps
per row, accepted drafts per step and whether the tokens equal the plain loop's.
Usage: python tools/bench_decode.py --model llama3_2 --num_params 1B --ragged 1,8,32 --tokens 128 --speculative 3,7 --hints self

``--continuous S1,S2,... [--budgets LO,HI] [--weight_dtype fp8]``: continuous batching
(``generate_continuous``) against static batches over the first 4 S synthetic Alpaca prompts.
Random-init weights never emit eos on cue, so every prompt gets a seeded budget, uniform in LO..HI
(default 16,128; LO = HI: equal budgets, where continuous batching can only lose): BUDGETS STAND IN
FOR ANSWER LENGTHS.  ``static``: ``generate_ragged`` over consecutive groups of S prompts, each
group run with its largest budget and its answers cut to their own budgets -- a static batch that
stops when its longest row is done.  ``continuous``: one ``generate_continuous`` call with S slots
and the per-prompt budgets.  Both greedy through the device sampler, interleaved A B A B in one
process, ``--repeats`` times after one warm-up of each; ms per KEPT token (sum of the budgets),
median and range, and next to it the schedule's own arithmetic: the static arm's decode steps,
sum over groups of (largest budget - 1), against the continuous arm's ``replays`` and ``prefills``.
Usage: python tools/bench_decode.py --model llama3_2 --num_params 1B --continuous 8,32 --budgets 16,128"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_llm_from_scratch_amd import ops  # noqa: E402
from building_llm_from_scratch_amd.config import get_config  # noqa: E402
from building_llm_from_scratch_amd.models import build_model  # noqa: E402
from building_llm_from_scratch_amd.train import generate as G  # noqa: E402


def _alpaca_prompts(model, cfg, n):
    from building_llm_from_scratch_amd.data.datasets import format_input
    from building_llm_from_scratch_amd.data.synthetic import alpaca_records
    from building_llm_from_scratch_amd.data.tokenizer import build_tokenizer
    tok = build_tokenizer(model, cfg)
    texts = [format_input(r) + "\n\n### Response:\n" for r in alpaca_records(n)]
    return [torch.tensor(tok.encode(t), dtype=torch.long) for t in texts], getattr(tok, "name", type(tok).__name__)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _stats(times, B, tokens):
    ms = sorted(1000 * t / (B * tokens) for t in times)
    rs = sorted(B / t for t in times)
    return {"ms_per_token": round(statistics.median(ms), 4), "ms_per_token_range": [round(ms[0], 4), round(ms[-1], 4)],
            "responses_per_s": round(statistics.median(rs), 2),
            "responses_per_s_range": [round(rs[0], 2), round(rs[-1], 2)]}


def ragged(a, m, cfg):
    sizes = [int(b) for b in a.ragged.split(",")]
    prompts, tok_name = _alpaca_prompts(a.model, cfg, max(sizes))
    ctx = cfg.context_length
    rows = []
    for B in sizes:
        ps = prompts[:B]

        def run_ragged():
            return G.generate_ragged(m, ps, a.tokens, ctx)

        def run_rows():
            return [G.generate_cached(m, p[None], a.tokens, ctx) for p in ps]

        run_ragged()
        run_rows()
        ta, tb = [], []
        for _ in range(a.repeats):
            ta.append(_timed(run_ragged))
            tb.append(_timed(run_rows))
        lens = [int(p.numel()) for p in ps]
        row = {"model": f"{a.model}-{a.num_params}", "batch": B, "new_tokens": a.tokens, "repeats": a.repeats,
               "tokenizer": tok_name, "prompt_tokens": {"min": min(lens), "max": max(lens), "sum": sum(lens)},
               "graph": os.environ.get("BLLM_DECODE_GRAPH", "default"),
               "generate_ragged": _stats(ta, B, a.tokens), "generate_cached_rows": _stats(tb, B, a.tokens)}
        row["speedup"] = round(row["generate_cached_rows"]["ms_per_token"] / row["generate_ragged"]["ms_per_token"], 2)
        lo, hi = row["generate_cached_rows"]["ms_per_token_range"]
        row["ragged_inside_rows_range"] = lo <= row["generate_ragged"]["ms_per_token"] <= hi
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


def ragged_sampling(a, m, cfg):
    sizes = [int(b) for b in a.ragged.split(",")]
    prompts, tok_name = _alpaca_prompts(a.model, cfg, max(sizes))
    ctx = cfg.context_length
    top_k = a.top_k if a.top_k > 0 else None
    rows = []
    for B in sizes:
        ps = prompts[:B]
        gen = torch.Generator(device="cuda").manual_seed(a.seed)
        arms = {"greedy": lambda: G.generate_ragged(m, ps, a.tokens, ctx)}
        if a.top_p >= 1.0:
            arms["torch_sample"] = lambda: G.generate_ragged(m, ps, a.tokens, ctx, temperature=a.temperature,
                                                             top_k=top_k, generator=gen)
        arms["device_sample"] = lambda: G.generate_ragged(m, ps, a.tokens, ctx, temperature=a.temperature, top_k=top_k,
                                                          top_p=a.top_p, seed=a.seed)
        for fn in arms.values():
            fn()
        times = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, fn in arms.items():
                times[k].append(_timed(fn))
        row = {"model": f"{a.model}-{a.num_params}", "batch": B, "new_tokens": a.tokens, "repeats": a.repeats,
               "tokenizer": tok_name, "temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p,
               "graph": os.environ.get("BLLM_DECODE_GRAPH", "default")}
        for k in arms:
            st = _stats(times[k], B, a.tokens)
            row[k] = {"ms_per_token": st["ms_per_token"], "ms_per_token_range": st["ms_per_token_range"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


def ragged_weights(a, m, cfg):
    """``--ragged B,... --weight_dtype fp8``: greedy ``generate_ragged`` on the model's weights
    against the fp8 decode weights, interleaved: ``fp8`` builds the packs inside every call (what a
    single ``generate_ragged`` call pays), ``fp8_prebuilt`` takes packs built once (what every
    batch of ``generate_responses`` pays); ``pack_build_ms`` is that build.  ``--weight_dtype mxfp4``
    runs three arms instead -- model weights, fp8 prebuilt, mxfp4 prebuilt -- and reports both
    builds (``pack_build_ms`` fp8, ``pack_build_ms_mxfp4``)."""
    sizes = [int(b) for b in a.ragged.split(",")]
    prompts, tok_name = _alpaca_prompts(a.model, cfg, max(sizes))
    ctx = cfg.context_length
    kv = None if a.kv_dtype == "model" else a.kv_dtype
    m.new_decode_weights("fp8")                         # warm-up of the build
    build = [_timed(lambda: m.new_decode_weights("fp8")) for _ in range(3)]
    packs = m.new_decode_weights("fp8")
    w4 = a.weight_dtype == "mxfp4"
    if w4:
        m.new_decode_weights("mxfp4")
        build4 = [_timed(lambda: m.new_decode_weights("mxfp4")) for _ in range(3)]
        packs4 = m.new_decode_weights("mxfp4")
    rows = []
    for B in sizes:
        ps = prompts[:B]
        arms = {"model": lambda: G.generate_ragged(m, ps, a.tokens, ctx, kv_dtype=kv),
                "fp8": lambda: G.generate_ragged(m, ps, a.tokens, ctx, kv_dtype=kv, weight_dtype="fp8"),
                "fp8_prebuilt": lambda: G.generate_ragged(m, ps, a.tokens, ctx, kv_dtype=kv, weight_dtype=packs)}
        if w4:
            del arms["fp8"]
            arms["mxfp4_prebuilt"] = lambda: G.generate_ragged(m, ps, a.tokens, ctx, kv_dtype=kv, weight_dtype=packs4)
        for fn in arms.values():
            fn()
        times = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, fn in arms.items():
                times[k].append(_timed(fn))
        row = {"model": f"{a.model}-{a.num_params}", "lora_rank": a.lora_rank, "batch": B, "new_tokens": a.tokens,
               "repeats": a.repeats, "tokenizer": tok_name, "kv_dtype": a.kv_dtype,
               "graph": os.environ.get("BLLM_DECODE_GRAPH", "default"),
               "pack_build_ms": round(1000 * statistics.median(build), 2)}
        for k in arms:
            ms = sorted(1000 * t / a.tokens for t in times[k])      # per step: all B rows advance together
            row["weights_" + k] = {"ms_per_step": round(statistics.median(ms), 4),
                                   "ms_per_step_range": [round(ms[0], 4), round(ms[-1], 4)]}
        row["model_over_fp8_prebuilt"] = round(row["weights_model"]["ms_per_step"] /
                                               row["weights_fp8_prebuilt"]["ms_per_step"], 3)
        if w4:
            row["pack_build_ms_mxfp4"] = round(1000 * statistics.median(build4), 2)
            row["fp8_prebuilt_over_mxfp4_prebuilt"] = round(row["weights_fp8_prebuilt"]["ms_per_step"] /
                                                            row["weights_mxfp4_prebuilt"]["ms_per_step"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


def ragged_speculative(a, m, cfg):
    sizes = [int(b) for b in a.ragged.split(",")]
    ks = [int(k) for k in a.speculative.split(",")]
    prompts, tok_name = _alpaca_prompts(a.model, cfg, max(sizes))
    ctx = cfg.context_length
    rows = []
    for B in sizes:
        ps = prompts[:B]
        plain = [r.cpu() for r in G.generate_ragged(m, ps, a.tokens, ctx, seed=0)]     # also the warm-up
        arms = {"plain": (None, None)}
        for k in ks:
            arms[f"spec{k}"] = (k, None)
            if a.hints == "plain":
                arms[f"spec{k}_hinted"] = (k, plain)
            elif a.hints == "self":
                arms[f"spec{k}_hinted"] = (k, [r.cpu() for r in G.generate_ragged(m, ps, a.tokens, ctx, seed=0,
                                                                                   speculative=k)])
        stats = {k: {} for k in arms}

        def run(arm):
            k, hints = arms[arm]
            return G.generate_ragged(m, ps, a.tokens, ctx, seed=0, speculative=k, draft_hints=hints,
                                     stats=stats[arm] if k else None)

        same = {arm: all(torch.equal(x.cpu(), y) for x, y in zip(run(arm), plain)) for arm in arms}
        times = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k in arms:
                times[k].append(_timed(lambda: run(k)))
        row = {"model": f"{a.model}-{a.num_params}", "batch": B, "new_tokens": a.tokens, "repeats": a.repeats,
               "tokenizer": tok_name, "graph": os.environ.get("BLLM_DECODE_GRAPH", "default")}
        for k in arms:
            st = _stats(times[k], B, a.tokens)
            row[k] = {"ms_per_token": st["ms_per_token"], "ms_per_token_range": st["ms_per_token_range"],
                      "same_tokens_as_plain": same[k]}
            if arms[k][0]:
                steps, drawn = stats[k]["steps"], stats[k]["new_tokens"]
                row[k]["steps_per_row"] = round(sum(steps) / B, 2)
                row[k]["accepted_drafts_per_step"] = round(sum(d - 1 - s for d, s in zip(drawn, steps)) /
                                                           max(sum(steps), 1), 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


def continuous(a, m, cfg):
    sizes = [int(b) for b in a.continuous.split(",")]
    lo, hi = (int(v) for v in a.budgets.split(","))
    prompts, tok_name = _alpaca_prompts(a.model, cfg, 4 * max(sizes))
    ctx = cfg.context_length
    kv = None if a.kv_dtype == "model" else a.kv_dtype
    packs = m.new_decode_weights(a.weight_dtype) if a.weight_dtype != "model" else None
    rows = []
    for S in sizes:
        ps = prompts[:4 * S]
        g = torch.Generator().manual_seed(a.seed)
        budgets = torch.randint(lo, hi + 1, (len(ps),), generator=g).tolist()
        groups = [range(i, min(i + S, len(ps))) for i in range(0, len(ps), S)]
        stats = {}

        def run_static():
            res = []
            for grp in groups:
                out = G.generate_ragged(m, [ps[i] for i in grp], max(budgets[i] for i in grp), ctx, seed=0,
                                        kv_dtype=kv, weight_dtype=packs)
                res += [r[:ps[i].numel() + budgets[i]] for i, r in zip(grp, out)]
            return res

        def run_continuous():
            return G.generate_continuous(m, ps, budgets, ctx, S, seed=0, kv_dtype=kv, weight_dtype=packs, stats=stats)

        a_out, b_out = run_static(), run_continuous()         # also the warm-up of each
        same = sum(bool(torch.equal(x, y)) for x, y in zip(a_out, b_out))
        ta, tb = [], []
        for _ in range(a.repeats):
            ta.append(_timed(run_static))
            tb.append(_timed(run_continuous))
        kept = sum(budgets)

        def arm(times):
            ms = sorted(1000 * t / kept for t in times)
            return {"ms_per_kept_token": round(statistics.median(ms), 4),
                    "ms_per_kept_token_range": [round(ms[0], 4), round(ms[-1], 4)]}

        lens = [int(p.numel()) for p in ps]
        static_steps = sum(max(budgets[i] for i in grp) - 1 for grp in groups)
        row = {"model": f"{a.model}-{a.num_params}", "slots": S, "prompts": len(ps), "repeats": a.repeats,
               "note": "budgets stand in for answer lengths (random-init weights emit no eos on cue)",
               "budgets": {"lo": lo, "hi": hi, "seed": a.seed, "sum": kept, "mean": round(kept / len(ps), 1)},
               "tokenizer": tok_name, "prompt_tokens": {"min": min(lens), "max": max(lens), "sum": sum(lens)},
               "kv_dtype": a.kv_dtype, "weight_dtype": a.weight_dtype,
               "graph": os.environ.get("BLLM_DECODE_GRAPH", "default"),
               "static": dict(arm(ta), decode_steps=static_steps, prefills=len(groups)),
               "continuous": dict(arm(tb), decode_steps=stats["replays"], prefills=stats["prefills"]),
               "answers_equal": f"{same}/{len(ps)}"}
        row["step_ratio"] = round(static_steps / max(stats["replays"], 1), 3)
        row["time_ratio"] = round(row["static"]["ms_per_kept_token"] / row["continuous"]["ms_per_kept_token"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


def context_bench(a, m, cfg):
    ctx = cfg.context_length
    if a.prompt + a.tokens > ctx:
        sys.exit(f"bench_decode: prompt ({a.prompt}) + tokens ({a.tokens}) exceed --context ({ctx})")
    idx = torch.randint(0, cfg.vocab_size, (a.batch, a.prompt), device="cuda")
    default_min = ops.DECODE_SPLIT_MIN
    if ctx <= default_min:
        arms = {"single_launch": (default_min, "1"), "split": (0, "1")}
    else:
        arms = {"graph": (default_min, "1"), "eager": (default_min, "0")}

    def run(arm, tokens):
        ops.DECODE_SPLIT_MIN, os.environ["BLLM_DECODE_GRAPH"] = arms[arm]
        try:
            return G.generate_cached(m, idx, tokens, ctx)
        finally:
            ops.DECODE_SPLIT_MIN = default_min

    outs = {k: run(k, a.tokens) for k in arms}         # warm-up of each arm
    times = {k: [] for k in arms}
    prefill = []
    for _ in range(a.repeats):
        for k in arms:
            times[k].append(_timed(lambda: run(k, a.tokens)))
        prefill.append(_timed(lambda: run(next(iter(arms)), 1)))
    row = {"model": f"{a.model}-{a.num_params}", "context": ctx, "batch": a.batch, "prompt_tokens": a.prompt,
           "new_tokens": a.tokens, "repeats": a.repeats,
           "prefill_ms": round(1000 * statistics.median(prefill), 3)}
    for k in arms:
        ms = sorted(1000 * t / a.tokens for t in times[k])
        row[k] = {"ms_per_token": round(statistics.median(ms), 4), "ms_per_token_range": [round(ms[0], 4), round(ms[-1], 4)]}
    first, second = list(arms)
    row["same_tokens"] = bool(torch.equal(outs[first], outs[second]))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([row], f, indent=1)


def kv_bench(a, m, cfg):
    ctx = cfg.context_length
    if a.prompt + a.tokens > ctx:
        sys.exit(f"bench_decode: prompt ({a.prompt}) + tokens ({a.tokens}) exceed --context ({ctx})")
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (a.prompt,), generator=g) for _ in range(a.batch)]
    arms = {k: (None if k == "model" else k) for k in a.kv_arms.split(",")}

    def run(arm, tokens):
        return G.generate_ragged(m, prompts, tokens, ctx, kv_dtype=arms[arm])

    def cache_bytes(arm):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        cache = m.new_kv_cache(a.batch, ctx, kv_dtype=arms[arm])
        used = torch.cuda.max_memory_allocated() - base
        del cache
        return used

    nbytes = {k: cache_bytes(k) for k in arms}
    for k in arms:                                     # warm-up of each arm
        run(k, a.tokens)
    times = {k: [] for k in arms}
    prefill = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k in arms:
            times[k].append(_timed(lambda: run(k, a.tokens)))
            prefill[k].append(_timed(lambda: run(k, 1)))
    row = {"model": f"{a.model}-{a.num_params}", "context": ctx, "batch": a.batch, "prompt_tokens": a.prompt,
           "new_tokens": a.tokens, "repeats": a.repeats, "graph": os.environ.get("BLLM_DECODE_GRAPH", "default")}
    for k in arms:
        ms = sorted(1000 * t / a.tokens for t in times[k])
        row["kv_" + k] = {"ms_per_token": round(statistics.median(ms), 4), "ms_per_token_range": [round(ms[0], 4), round(ms[-1], 4)],
                  "prefill_ms": round(1000 * statistics.median(prefill[k]), 3), "cache_bytes": nbytes[k]}
    if len(arms) == 2:
        row["fp8_no_slower"] = row["kv_fp8"]["ms_per_token"] <= row["kv_model"]["ms_per_token_range"][1]
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([row], f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3")
    ap.add_argument("--num_params", default="8B")
    ap.add_argument("--tokens", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt", type=int, default=6)
    ap.add_argument("--graph", type=int, default=None, help="force the hipGraph decode step on/off")
    ap.add_argument("--ragged", default=None, help="comma list of batch sizes: generate_ragged vs one-row runs")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="--ragged / --context: also write the rows to this JSON file")
    ap.add_argument("--temperature", type=float, default=0.0, help="--ragged: > 0 compares the sampling paths (see above)")
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--context", type=int, default=None,
                    help="model context = KV-cache length; compares the decode-attention kernels (see above)")
    ap.add_argument("--kv_dtype", default="model", choices=["model", "fp8"],
                    help="--context: fp8 compares the KV-cache formats through generate_ragged (see above)")
    ap.add_argument("--kv_arms", default="model,fp8", help="--kv_dtype fp8: the arms to run")
    ap.add_argument("--weight_dtype", default="model", choices=["model", "fp8", "mxfp4"],
                    help="--ragged: fp8 compares the decode steps on fp8 weight packs with the model's weights")
    ap.add_argument("--lora_rank", type=int, default=0,
                    help="--weight_dtype fp8: a LoRA model (this rank on every linear, nonzero B), folded into the packs")
    ap.add_argument("--speculative", default=None,
                    help="--ragged: comma list of K, speculative decoding against the plain loop (see above)")
    ap.add_argument("--hints", default="none", choices=["none", "self", "plain"],
                    help="--speculative: adds arms hinted with each prompt and its own answer (self: the unhinted "
                         "speculative arm's, plain: the plain loop's)")
    ap.add_argument("--continuous", default=None,
                    help="comma list of slot counts S: generate_continuous against static batches of S over 4 S "
                         "prompts with seeded budgets (see above)")
    ap.add_argument("--budgets", default="16,128", help="--continuous: per-prompt budgets uniform in LO,HI (--seed)")
    a = ap.parse_args()
    ops.load_ext(required=True)
    cfg = (get_config(a.model, a.num_params) if a.context is None
           else get_config(a.model, a.num_params, context_length=a.context)).replace(dtype=torch.bfloat16)
    torch.manual_seed(0)
    m = build_model(cfg, device="cuda")
    if a.lora_rank > 0:
        from building_llm_from_scratch_amd.models.lora import replace_linear_with_lora
        for p in m.parameters():
            p.requires_grad = False
        replace_linear_with_lora(m, rank=a.lora_rank, alpha=2 * a.lora_rank, dtype=torch.bfloat16)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("lora.B"):
                    p.normal_(0.0, 0.02)
    m.flatten()
    if a.graph is not None:
        os.environ["BLLM_DECODE_GRAPH"] = str(a.graph)
    if a.continuous:
        return continuous(a, m, cfg)
    if a.ragged and a.speculative:
        return ragged_speculative(a, m, cfg)
    if a.ragged and a.weight_dtype in ("fp8", "mxfp4"):
        return ragged_weights(a, m, cfg)
    if a.ragged:
        return ragged_sampling(a, m, cfg) if a.temperature > 0 else ragged(a, m, cfg)
    if a.context is not None:
        return kv_bench(a, m, cfg) if a.kv_dtype == "fp8" else context_bench(a, m, cfg)
    idx = torch.randint(0, cfg.vocab_size, (a.batch, a.prompt), device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    G.generate_cached(m, idx, 8, cfg.context_length, temperature=1.0, top_k=5, generator=g)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = G.generate_cached(m, idx, a.tokens, cfg.context_length, temperature=1.0, top_k=5, generator=g)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = out.shape[1] - a.prompt
    print(json.dumps({"model": f"{a.model}-{a.num_params}", "batch": a.batch, "new_tokens": n,
                      "ms_per_token": round(1000 * dt / max(n, 1), 3), "tokens_per_s": round(a.batch * n / dt, 1),
                      "graph": os.environ.get("BLLM_DECODE_GRAPH", "default")}))


if __name__ == "__main__":
    main()
