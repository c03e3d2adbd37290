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

A file that gained kernels differs as a text, so a differing file is compared a second time
kernel by kernel: the text of each function of BASE_TREE (its instructions, kernel descriptor,
resource comments and metadata entry, with the per-file numbering of local labels dropped) must
appear unchanged in NEW_TREE.  Such a file is reported as ``kernels identical (+N new)`` and
does not count as a difference; a base kernel that is missing or altered does.

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


# per-file numbering of local labels, in label definitions, operands and loop comments
_LOCAL = re.compile(r"(\.L|\b)(BB|func_end|func_begin|JTI|tmp)\d+")
_PAD = re.compile(r"[ \t]+;")


def _kernels(lines: list[str]) -> dict[str, list[str]]:
    """Function name -> its text: the ``Begin function`` block (up to the next one or the
    file's trailer) and its ``amdhsa.kernels`` metadata entry, local label numbers dropped."""
    out: dict[str, list[str]] = {}
    cur = None
    meta: list[str] | None = None
    in_meta = False

    def close_meta():
        nonlocal meta
        if meta:
            name = next((ln.split(":", 1)[1].strip() for ln in meta if ln.lstrip().startswith(".name:")), None)
            if name:
                out.setdefault(name, []).extend(meta)
        meta = None

    for ln in lines:
        if in_meta:
            if ln.startswith("  - "):
                close_meta()
                meta = [ln]
            elif ln.startswith("    ") and meta is not None:
                meta.append(ln)
            else:
                close_meta()
                if ".end_amdgpu_metadata" in ln:
                    in_meta = False
            continue
        if ".amdgpu_metadata" in ln:
            in_meta, cur = True, None
            continue
        m = re.search(r"; -- Begin function (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif ln.startswith("\t.section\t.AMDGPU.gpr_maximums"):
            cur = None
        # "\t.text" opens the NEXT function (absent after a file's last one), and a label's comment
        # column moves with the width of the label number that was dropped: neither is kernel text
        if cur is not None and not ln.startswith("\t.section\t.text.") and ln != "\t.text":
            cur.append(_PAD.sub(" ;", _LOCAL.sub(lambda k: k.group(1) + k.group(2), ln)))
    return out


def _per_kernel(x: list[str], y: list[str]) -> tuple[int, int]:
    """(base kernels missing or altered in new, kernels only in new)"""
    kx, ky = _kernels(x), _kernels(y)
    return sum(1 for k, v in kx.items() if ky.get(k) != v), sum(1 for k in ky if k not in kx)


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
                changed, added = (1, 0) if a.rename_symbols else _per_kernel(x, y)
                if changed == 0 and added > 0:
                    row += f"{'kernels identical (+%d new)' % added:>28s}"
                    continue
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
