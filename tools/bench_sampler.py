#!/usr/bin/env python3
"""Token sampler, op level (GPU): ``ops.sample_rows`` (csrc/sample.hip, one launch) against the
torch composition it replaces, on bf16 logits [B, V], interleaved A B A B in one process.

* ``top_k=5, T=1``: ``train/generate.py:_sample`` (float, topk, where, softmax, multinomial);
* ``top_k=50, top_p=0.9, T=1``: a sort-based nucleus sampler written here (float, topk, sort,
  softmax, cumsum, masked fill, multinomial, gather), the usual way without a kernel.

Per shape and setting one JSON line: median and range over ``--repeats`` of the microseconds per
call (``--iters`` calls between two device synchronisations) and the number of kernel launches
each side issues per call (counted by the profiler in a run of its own, not while timing).
Usage: python tools/bench_sampler.py [--vocab 50257,128256] [--batch 1,8,32] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_llm_from_scratch_amd import ops  # noqa: E402
from building_llm_from_scratch_amd.train.generate import _sample  # noqa: E402


def torch_top_p(logits, temperature, top_k, top_p, generator):
    v, i = torch.topk(logits.float(), top_k)                  # descending
    p = torch.softmax(v / temperature, dim=-1)
    before = p.cumsum(dim=-1) - p                              # mass above each entry
    p = p.masked_fill(before >= top_p, 0.0)
    return i.gather(1, torch.multinomial(p, num_samples=1, generator=generator))


def launches(fn):
    """Kernel launches of one call, counted by the profiler (None where it is unavailable)."""
    try:
        return _launches(fn)
    except Exception as e:   # the count is a by-product: the timings stand without it
        print(f"bench_sampler: no launch count ({type(e).__name__}: {e})", file=sys.stderr)
        return None


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", default="50257,128256")
    ap.add_argument("--batch", default="1,8,32")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.load_ext(required=True)
    rows = []
    for V in (int(v) for v in a.vocab.split(",")):
        for B in (int(b) for b in a.batch.split(",")):
            g = torch.Generator(device="cuda").manual_seed(1)
            logits = (4.0 * torch.randn(B, V, device="cuda", generator=g)).to(torch.bfloat16)
            stream = torch.arange(B, device="cuda")
            ctr = torch.zeros(B, dtype=torch.int32, device="cuda")
            for name, k, p in (("top_k=5", 5, 1.0), ("top_k=50,top_p=0.9", 50, 0.9)):
                kernel = lambda: ops.sample_rows(logits, stream, ctr, 7, 1.0, k, p)
                composed = (lambda: _sample(logits, 1.0, k, g)) if p >= 1.0 else (lambda: torch_top_p(logits, 1.0, k, p, g))
                arms = {"sample_rows": kernel, "torch": composed}
                for fn in arms.values():
                    timed(fn, 10)
                us = {n: [] for n in arms}
                for _ in range(a.repeats):
                    for n, fn in arms.items():
                        us[n].append(timed(fn, a.iters))
                row = {"V": V, "B": B, "setting": name, "dtype": "bf16", "iters": a.iters, "repeats": a.repeats}
                for n, fn in arms.items():
                    row[n] = {"us_per_call": round(statistics.median(us[n]), 2),
                              "us_range": [round(min(us[n]), 2), round(max(us[n]), 2)], "launches": launches(fn)}
                print(json.dumps(row), flush=True)
                rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
