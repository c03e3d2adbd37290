#!/usr/bin/env python3
"""Decode attention at op level (GPU): the single-launch kernel (csrc/attn_decode.hip, at most
8,192 keys) against the split-KV kernels (csrc/attn_decode_split.hip), on the head shapes of the
registry's models.  Both through ``torch.ops.bllm`` directly (per-row append form, every row at
position L - 1 of a cache of L positions), so ``ops.DECODE_SPLIT_MIN`` plays no part.

One process, the two kernels interleaved A B A B, ``--repeats`` timed windows each after a
warm-up; a window is ``iters`` calls between two device events, sized to ``--window_ms``.  The calls
rotate over up to 16 caches (a model's layers; fewer once one cache passes 1 GiB), as a decode
step does, so a small cache is not simply re-read from L2.  Per case one JSON line: median and
range of microseconds per call, and the rate "valid K + V bytes read once / time" (what a kernel
that reads every cached row once would move; the single-launch kernel reads them H/G times).
Before timing, the two kernels' outputs are compared on the same inputs.

``--kv fp8``: the arms are the bf16 split-KV kernel and the fp8-cache kernel (csrc/attn_decode_fp8.hip)
on the same values, quantised per row by the oracle; the fp8 arm's rate counts the bytes it has
to read, hd + 4 per row (bytes and one fp32 scale), and ``fp8_no_slower`` says whether its median
time is inside or below the range of the bf16 arm's repeats.

``--extend Q1,Q2,...``: the arms are one token per row (``ops.attn_decode_append_rows``: the
single-launch kernel up to 8,192 positions, split-KV beyond) and ``ops.attn_extend_rows`` with Q tokens
per row (csrc/attn_extend.hip), the Q tokens in the cache's last Q positions.  Per Q: the ratio to the
one-token call and ``cheaper_than_q_calls`` (ratio < Q, what the Q-token step is for); the rates count
the valid K + V bytes once.

Usage: python tools/bench_decode_attn.py [--shapes llama3_2-1B,llama3-8B,gpt2-774M] [--batch 1,32]
           [--lengths 1024,8192,32768,131072] [--repeats 5] [--kv model|fp8] [--extend 2,4,8] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_llm_from_scratch_amd import ops  # noqa: E402
from building_llm_from_scratch_amd.ops import reference as ref  # noqa: E402

SHAPES = {"llama3_2-1B": (32, 8, 64), "llama3-8B": (32, 8, 128), "gpt2-774M": (20, 20, 64)}   # H, G, hd
SINGLE_MAX = 8192


def kv_bytes(B, G, L, hd, esize=2):
    return 2 * B * G * L * hd * esize


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters      # microseconds per call


def _stats(us, nbytes):
    s = sorted(us)
    med = statistics.median(s)
    return {"us": round(med, 2), "us_range": [round(s[0], 2), round(s[-1], 2)],
            "TBps": round(nbytes / med / 1e6, 3)}


def _quantized(c):
    """The fp8 form of one bf16 cache [B, G, L, hd], a batch row at a time (the oracle works in fp64)."""
    q = torch.empty(c.shape, device=c.device, dtype=torch.float8_e4m3fn)
    s = torch.empty(c.shape[:3], device=c.device, dtype=torch.float32)
    for b in range(c.shape[0]):
        for g in range(c.shape[1]):
            q[b, g], s[b, g] = ref.kv_quantize_rows(c[b, g])
    return q, s


def case_fp8(name, B, L, a):
    H, G, hd = SHAPES[name]
    dt = torch.bfloat16
    nbytes, nbytes8 = kv_bytes(B, G, L, hd), 2 * B * G * L * (hd + 4)
    nbuf = max(1, min(16, (1 << 30) // nbytes + 1))
    caches, caches8 = [], []
    for _ in range(nbuf):
        kc = torch.empty(B, G, L, hd, device="cuda", dtype=dt).normal_()
        vc = torch.empty(B, G, L, hd, device="cuda", dtype=dt).normal_()
        (k8, ks), (v8, vs) = _quantized(kc), _quantized(vc)
        caches.append((kc, vc))
        caches8.append((k8, ks, v8, vs))
    qkv = torch.randn(B, (H + 2 * G) * hd, device="cuda").to(dt)
    pos = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
    bl = torch.ops.bllm

    def split(i):
        kc, vc = caches[i % nbuf]
        return bl.attn_decode_append_split(qkv, kc, vc, pos, H, G)

    def fp8(i):
        k8, ks, v8, vs = caches8[i % nbuf]
        return bl.attn_decode_append_rows_fp8(qkv, k8, ks, v8, vs, pos, H, G)

    arms = {"split": split, "fp8": fp8}
    d = (split(0).float() - fp8(0).float()).abs().max().item()
    assert d < 5e-2, f"{name} B {B} L {L}: the bf16 and fp8 caches differ by {d}"
    times = {k: [] for k in arms}
    iters = {}
    for k, fn in arms.items():
        _window(fn, 3)
        iters[k] = max(3, min(2000, int(a.window_ms * 1000.0 / max(_window(fn, 5), 1.0))))
    for _ in range(a.repeats):
        for k, fn in arms.items():
            times[k].append(_window(fn, iters[k]))
    row = {"shape": name, "H": H, "G": G, "hd": hd, "B": B, "L": L, "kv_bytes": nbytes, "kv_bytes_fp8": nbytes8,
           "caches": nbuf, "repeats": a.repeats, "max_abs_diff": round(d, 5)}
    row["split"] = _stats(times["split"], nbytes)
    row["fp8"] = _stats(times["fp8"], nbytes8)
    for k in arms:
        row[k]["iters"] = iters[k]
    row["fp8_over_split"] = round(row["split"]["us"] / row["fp8"]["us"], 3)
    row["fp8_no_slower"] = row["fp8"]["us"] <= row["split"]["us_range"][1]
    print(json.dumps(row), flush=True)
    return row


def case_extend(name, B, L, a):
    H, G, hd = SHAPES[name]
    dt = torch.bfloat16
    qs = [int(q) for q in a.extend.split(",")]
    nbytes = kv_bytes(B, G, L, hd)
    nbuf = max(1, min(16, (1 << 30) // nbytes + 1))
    caches = [(torch.empty(B, G, L, hd, device="cuda", dtype=dt).normal_(),
               torch.empty(B, G, L, hd, device="cuda", dtype=dt).normal_()) for _ in range(nbuf)]
    qkv = {q: torch.randn(B * q, (H + 2 * G) * hd, device="cuda").to(dt) for q in [1] + qs}
    pos = {q: torch.full((B,), L - q, dtype=torch.int32, device="cuda") for q in [1] + qs}
    pos_rows = {q: (pos[q][:, None] + torch.arange(q, dtype=torch.int32, device="cuda")).reshape(-1) for q in qs}

    def one(i):
        kc, vc = caches[i % nbuf]
        return ops.attn_decode_append_rows(qkv[1], kc, vc, pos[1], H, G)

    def extend(q):
        def fn(i):
            kc, vc = caches[i % nbuf]
            return ops.attn_extend_rows(qkv[q], kc, vc, pos[q], q, H, G, pos_rows=pos_rows[q])
        return fn

    arms = {"one": one}
    for q in qs:
        arms[f"extend{q}"] = extend(q)
    times = {k: [] for k in arms}
    iters = {}
    for k, fn in arms.items():
        _window(fn, 3)
        iters[k] = max(3, min(2000, int(a.window_ms * 1000.0 / max(_window(fn, 5), 1.0))))
    for _ in range(a.repeats):
        for k, fn in arms.items():
            times[k].append(_window(fn, iters[k]))
    row = {"shape": name, "H": H, "G": G, "hd": hd, "B": B, "L": L, "kv_bytes": nbytes, "caches": nbuf,
           "repeats": a.repeats}
    for k in arms:
        row[k] = _stats(times[k], nbytes)
        row[k]["iters"] = iters[k]
    for q in qs:
        r = row[f"extend{q}"]
        r["ratio_to_one"] = round(r["us"] / row["one"]["us"], 3)
        r["cheaper_than_q_calls"] = r["us"] < q * row["one"]["us"]
    print(json.dumps(row), flush=True)
    return row


def case(name, B, L, a):
    H, G, hd = SHAPES[name]
    dt = torch.bfloat16
    nbytes = kv_bytes(B, G, L, hd)
    nbuf = max(1, min(16, (1 << 30) // nbytes + 1))
    caches = [(torch.empty(B, G, L, hd, device="cuda", dtype=dt).normal_(),
               torch.empty(B, G, L, hd, device="cuda", dtype=dt).normal_()) for _ in range(nbuf)]
    qkv = torch.randn(B, (H + 2 * G) * hd, device="cuda").to(dt)
    pos = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
    bl = torch.ops.bllm

    def split(i):
        kc, vc = caches[i % nbuf]
        return bl.attn_decode_append_split(qkv, kc, vc, pos, H, G)

    def single(i):
        kc, vc = caches[i % nbuf]
        return bl.attn_decode_append_rows(qkv, kc, vc, pos, H, G)

    arms = {"split": split}
    if L <= SINGLE_MAX:
        arms["single"] = single
        d = (split(0).float() - single(0).float()).abs().max().item()
        assert d < 2e-2, f"{name} B {B} L {L}: the kernels differ by {d}"
    times = {k: [] for k in arms}
    iters = {}
    for k, fn in arms.items():                      # warm-up, and the window's length
        _window(fn, 3)
        iters[k] = max(3, min(2000, int(a.window_ms * 1000.0 / max(_window(fn, 5), 1.0))))
    for _ in range(a.repeats):
        for k, fn in arms.items():
            times[k].append(_window(fn, iters[k]))
    row = {"shape": name, "H": H, "G": G, "hd": hd, "B": B, "L": L, "kv_bytes": nbytes, "caches": nbuf,
           "repeats": a.repeats}
    for k in arms:
        row[k] = _stats(times[k], nbytes)
        row[k]["iters"] = iters[k]
    if "single" in row:
        row["split_over_single"] = round(row["single"]["us"] / row["split"]["us"], 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batch", default="1,32")
    ap.add_argument("--lengths", default="1024,8192,32768,131072")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=40.0)
    ap.add_argument("--kv", default="model", choices=["model", "fp8"],
                    help="fp8: the bf16 split-KV kernel against the fp8-cache kernel")
    ap.add_argument("--extend", default=None,
                    help="comma list of Q: one token per row against attn_extend_rows with Q tokens per row")
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_attn: needs a GPU")
    ops.load_ext(required=True)
    torch.manual_seed(0)
    rows = []
    for name in a.shapes.split(","):
        for B in (int(b) for b in a.batch.split(",")):
            for L in (int(x) for x in a.lengths.split(",")):
                fn = case_extend if a.extend else (case_fp8 if a.kv == "fp8" else case)
                rows.append(fn(name, B, L, a))
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
