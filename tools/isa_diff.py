#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two source trees, file by file.

A refactor of ``csrc/`` that is meant to change no kernel is proven neutral by its device code,
not by a benchmark: every ``csrc/*.hip`` of both trees is compiled with the device flags of
``tools/build_ext.py`` plus ``--cuda-device-only -S`` (release: ``-O3``; debug: ``-O1
-DBLLM_KERNEL_DEBUG=1``) and the two ``.s`` texts are compared after dropping the lines that
carry the per-translation-unit ``__hip_cuid_<hash>`` symbol.  The comparison is textual; it
knows nothing about particular instructions.

``--rename-symbols`` additionally replaces every mangled C++ symbol by the index of its first
appearance in the file before comparing, for a change that drops a template parameter of a
kernel (so its symbol changes) but must leave its instruction stream, register counts and LDS
size as they were.  Kernels are emitted in source order, so the indices of two trees line up as
long as that order is unchanged.

Usage:
    python tools/isa_diff.py BASE_TREE [NEW_TREE] [--work DIR] [-j N] [--rename-symbols]
                             [--only release|debug] [--files a.hip b.hip ...]

BASE_TREE / NEW_TREE are directories that hold ``csrc/`` (NEW_TREE defaults to this checkout;
``git worktree add DIR REV`` or ``git archive REV csrc | tar -x -C DIR`` makes one for a
revision).  Assembly is kept under --work (default ``build/isa_diff``) and reused while it is
newer than every file of its tree's ``csrc/``.  Prints one verdict per file and mode; the exit
status is 0 when all are identical.  Takes minutes: not part of the test suite.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import hashlib
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = os.environ.get("BLLM_ARCH", "gfx950")
MODES = {"release": ["-O3"], "debug": ["-O1", "-DBLLM_KERNEL_DEBUG=1"]}


def _tool(name: str, *fallbacks: str) -> str:
    for c in (os.environ.get(name.upper().replace("-", "_")), *fallbacks, shutil.which(name)):
        if c and os.path.exists(c):
            return c
    raise RuntimeError(f"{name} not found (ROCm required)")


def _compile(hipcc: str, tree: str, src: str, mode: str, out: str) -> str:
    csrc = os.path.join(tree, "csrc")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(d) for d in deps):
        return out
    cmd = [hipcc, f"--offload-arch={ARCH}", "-std=c++17", "-munsafe-fp-atomics", f"-I{csrc}"] + MODES[mode] + [
        "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"compile failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return out


def _normalise(path: str, rename: bool) -> list[str]:
    with open(path) as f:
        text = "".join(ln for ln in f if "__hip_cuid_" not in ln)
    if rename:
        table: dict[str, str] = {}
        text = re.sub(r"_Z\w+", lambda m: table.setdefault(m.group(0), f"SYM{len(table)}"), text)
    return text.split("\n")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("base")
    ap.add_argument("new", nargs="?", default=ROOT)
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "isa_diff"))
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--rename-symbols", action="store_true")
    ap.add_argument("--only", choices=sorted(MODES))
    ap.add_argument("--files", nargs="*")
    a = ap.parse_args()
    hipcc = _tool("hipcc", "/opt/rocm/bin/hipcc")
    trees = [os.path.abspath(a.base), os.path.abspath(a.new)]
    names = [sorted(f for f in os.listdir(os.path.join(t, "csrc")) if f.endswith(".hip")) for t in trees]
    files = [f for f in names[0] if f in names[1] and (not a.files or f in a.files)]
    modes = [a.only] if a.only else sorted(MODES, reverse=True)
    jobs = {}
    with cf.ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
        for t in trees:
            tdir = os.path.join(a.work, hashlib.sha1(t.encode()).hexdigest()[:10])
            for mode in modes:
                os.makedirs(os.path.join(tdir, mode), exist_ok=True)
                for f in files:
                    out = os.path.join(tdir, mode, f[:-4] + ".s")
                    jobs[(t, mode, f)] = ex.submit(_compile, hipcc, t, f, mode, out)
        for fu in jobs.values():
            fu.result()
    bad = 0
    print(f"{'file':24s}" + "".join(f"{m:>28s}" for m in modes))
    for f in files:
        row = f"{f:24s}"
        for mode in modes:
            x, y = (_normalise(jobs[(t, mode, f)].result(), a.rename_symbols) for t in trees)
            if x == y:
                row += f"{'identical (%d lines)' % len(x):>28s}"
            else:
                bad += 1
                n = sum(1 for p, q in zip(x, y) if p != q) + abs(len(x) - len(y))
                row += f"{'DIFFERS (%d lines)' % n:>28s}"
        print(row)
    for side, other in ((0, 1), (1, 0)):
        for f in names[side]:
            if f not in names[other]:
                print(f"{f:24s} only in {trees[side]}")
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except RuntimeError as e:
        print(e, file=sys.stderr)
        sys.exit(1)
