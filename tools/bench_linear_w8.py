#!/usr/bin/env python3
"""FP8-weight decode projection, op level (GPU): ``ops.linear_w8`` (csrc/linear_w8.hip) against the
library call the decode step makes today on 16-bit weights -- ``mm_nt``, ``ops.linear_residual`` or
``torch.addmm`` -- at the projection shapes of Llama-3.2-1B, Llama-3-8B and GPT2-774M, M = 1, 8, 32
rows, interleaved A B A B in one process.

Every call takes the next of C copies of its weight, C chosen so that the copies of the smaller
(fp8) arm alone hold twice the 256 MB last-level cache: no call finds its matrix on chip.  Per
shape and M one JSON line: median and range over ``--repeats`` of the microseconds per call
(``--iters`` calls between two device synchronisations), the TB/s of the packed bytes (N K, what
the fp8 kernel must read), and the ratio library / fp8.  The timings include the launch: at these
sizes it is part of what a decode step pays.

``--format mxfp4`` adds a third arm to the same rotation, ``ops.linear_w4`` (csrc/linear_w4.hip) on
the MXFP4 pack of the same weight (N K 17 / 32 bytes; C is then sized by these, the smallest), and
reports its TB/s, the ratio fp8 / mxfp4 and ``w4_below_w8_range``: whether the MXFP4 median lies
below every fp8 repeat.
Usage: python tools/bench_linear_w8.py [--models llama3_2_1B,llama3_8B,gpt2_774M] [--rows 1,8,32] [--format mxfp4]
       [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_llm_from_scratch_amd import ops  # noqa: E402
from building_llm_from_scratch_amd.models.linear import mm_nt  # noqa: E402

LLC_BYTES = 256 * 2 ** 20


def llama_shapes(d, kv, hidden, vocab):
    return [("qkv", d + 2 * kv, d, "mm"), ("o", d, d, "residual"), ("gate_up", 2 * hidden, d, "mm"),
            ("down", d, hidden, "residual"), ("head", vocab, d, "mm")]


SHAPES = {
    "llama3_2_1B": llama_shapes(2048, 512, 8192, 128256),
    "llama3_8B": llama_shapes(4096, 1024, 14336, 128256),
    "gpt2_774M": [("qkv", 3840, 1280, "mm"), ("o", 1280, 1280, "bias"), ("fc", 5120, 1280, "bias"),
                  ("proj", 1280, 5120, "bias"), ("head", 50257, 1280, "mm")],
}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(SHAPES))
    ap.add_argument("--rows", default="1,8,32")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--format", default="fp8", choices=["fp8", "mxfp4"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w4 = a.format == "mxfp4"
    ops.load_ext(required=True)
    dt, dev = torch.bfloat16, "cuda"
    rows = []
    for model in a.models.split(","):
        for name, N, K, kind in SHAPES[model]:
            C = -(-2 * LLC_BYTES // (N * K * 17 // 32 if w4 else N * K)) + 1
            W = torch.randn(C, N, K, device=dev, dtype=dt) * 0.02
            pack = ops.w8_pack(W[0])
            packs = [pack] + [pack._replace(data=pack.data.clone()) for _ in range(C - 1)]
            if w4:
                pack4 = ops.w4_pack(W[0])
                packs4 = [pack4] + [pack4._replace(data=pack4.data.clone(), scale=pack4.scale.clone())
                                    for _ in range(C - 1)]
            bias = torch.randn(N, device=dev, dtype=dt)
            for M in (int(m) for m in a.rows.split(",")):
                x = torch.randn(M, K, device=dev, dtype=dt)
                res = torch.randn(M, N, device=dev, dtype=dt)
                if kind == "residual":
                    arms = {"library": lambda i: ops.linear_residual(x, W[i % C], res),
                            "linear_w8": lambda i: ops.linear_w8(x, packs[i % C], None, res)}
                elif kind == "bias":
                    arms = {"library": lambda i: torch.addmm(bias, x, W[i % C].t()),
                            "linear_w8": lambda i: ops.linear_w8(x, packs[i % C], bias)}
                else:
                    arms = {"library": lambda i: mm_nt(x, W[i % C]),
                            "linear_w8": lambda i: ops.linear_w8(x, packs[i % C])}
                if w4:
                    b4, r4 = (bias if kind == "bias" else None), (res if kind == "residual" else None)
                    arms["linear_w4"] = lambda i: ops.linear_w4(x, packs4[i % C], b4, r4)
                for fn in arms.values():
                    timed(fn, max(10, C))
                us = {n: [] for n in arms}
                for _ in range(a.repeats):
                    for n, fn in arms.items():
                        us[n].append(timed(fn, a.iters))
                row = {"model": model, "proj": name, "N": N, "K": K, "M": M, "call": kind, "copies": C,
                       "iters": a.iters, "repeats": a.repeats}
                for n in arms:
                    row[n] = {"us_per_call": round(statistics.median(us[n]), 2),
                              "us_range": [round(min(us[n]), 2), round(max(us[n]), 2)]}
                row["packed_TBps"] = round(N * K / row["linear_w8"]["us_per_call"] * 1e-6, 3)
                row["library_over_w8"] = round(row["library"]["us_per_call"] / row["linear_w8"]["us_per_call"], 2)
                if w4:
                    row["w4_packed_TBps"] = round(N * K * 17 / 32 / row["linear_w4"]["us_per_call"] * 1e-6, 3)
                    row["w8_over_w4"] = round(row["linear_w8"]["us_per_call"] / row["linear_w4"]["us_per_call"], 2)
                    row["w4_below_w8_range"] = row["linear_w4"]["us_per_call"] < row["linear_w8"]["us_range"][0]
                print(json.dumps(row), flush=True)
                rows.append(row)
            del W, packs, pack
            if w4:
                del packs4, pack4
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
