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

Usage: python tools/bench_decode_attn.py [--shapes llama3_2-1B,llama3-8B,gpt2-774M] [--batch 1,32]
           [--lengths 1024,8192,32768,131072] [--repeats 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_llm_from_scratch_amd import ops  # noqa: E402

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
                rows.append(case(name, B, L, a))
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
