"""Shape table of tests/test_large_extent_gpu.py, checked on any machine by
tests/test_large_extent_cpu.py: every entry places a little work at far offsets of a large, mostly
untouched allocation, so that a dropped 64-bit cast in a kernel's index arithmetic shows up.

Per entry: the tensors it allocates (name -> (elements allocated, bytes per element)), the "rows"
view of its largest tensor (row count and row pitch in elements: batch rows of a cache, logit rows,
GEMM operand rows), the boundaries that tensor crosses, the peak device memory the test may use
(tensors + reference slices + the op's own workspaces; at most ``CAP``) and its GEMM pitches.

Left out, with the reason:
  * ``adamw_step_`` / ``sq_norm_multi`` past 2^31 elements: parameter + master + gradient + two
    moments are ~35 GB of state, far over the cap; their loops already index with ``long``.
  * the attention training kernels, the norms, the embedding, ``linear_w8``, the sampler: no
    benchmarked shape brings any of their tensors near 2^31 elements.
  * ``rope_k``'s unchecked ``int total`` (csrc/elementwise.hip): reached only past ~6.7e6 rows.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import Dict, Tuple

GIB = 1 << 30
CAP = 12 * GIB
E31, E32 = 1 << 31, 1 << 32            # element boundaries
B32 = 1 << 32                          # byte boundary
N_RANDOM = 32

# csrc/binding.cpp kMaxGemmPitch: the largest operand row pitch (elements) for which every 32-bit
# per-lane byte offset of the MFMA GEMMs' staging is exact (derivation at the constant)
GEMM_MAX_PITCH = 8_421_504
# gemm_nt*_supported: 256 * lda * 2 < 2^31 bytes  ->  lda < 2^22 elements
GEMM_NT_PITCH_LIMIT = 1 << 22


@dataclass(frozen=True)
class Entry:
    tensors: Dict[str, Tuple[int, int]]          # name -> (elements allocated, itemsize)
    main: str                                    # the tensor whose rows are selected
    rows: int                                    # its row count ...
    pitch: int                                   # ... and row pitch in elements
    crosses: Tuple[str, ...]                     # of "e31" (2^31 elements), "b32" (2^32 bytes), "e32"
    peak: int                                    # bytes: stated peak device memory of the test
    gemm_pitches: Tuple[int, ...] = ()
    dims: Dict[str, int] = field(default_factory=dict)

    @property
    def itemsize(self) -> int:
        return self.tensors[self.main][1]

    @property
    def tensor_bytes(self) -> int:
        return sum(n * s for n, s in self.tensors.values())

    def boundaries(self):
        """The claimed boundaries as element indices into the main tensor."""
        at = {"e31": E31, "b32": B32 // self.itemsize, "e32": E32}
        return sorted({at[c] for c in self.crosses})


def boundary_rows(rows: int, pitch: int, boundary: int):
    """The row that holds element ``boundary`` and its neighbours (inside [0, rows))."""
    r = boundary // pitch
    return [x for x in (r - 1, r, r + 1) if 0 <= x < rows]


def select_rows(e: Entry, seed: int = 0, first: int = 2, last: int = 2):
    """Rows every test checks: the first, the last, the row containing each boundary the shape
    crosses with the rows either side of it, and N_RANDOM seeded random rows.  Sorted, unique."""
    pick = set(range(min(first, e.rows))) | set(range(max(e.rows - last, 0), e.rows))
    for b in e.boundaries():
        pick |= set(boundary_rows(e.rows, e.pitch, b))
    rng = random.Random(seed)
    pick |= {rng.randrange(e.rows) for _ in range(N_RANDOM)}
    return sorted(pick)


def _cache(B, G, Tmax, hd, itemsize, scales=False):
    n = B * G * Tmax * hd
    t = {"kcache": (n, itemsize), "vcache": (n, itemsize)}
    if scales:
        t["kscale"] = t["vscale"] = (B * G * Tmax, 4)
    return t


_H = 8      # query heads of the decode shapes (= G: no GQA expansion in the reference)

SHAPES: Dict[str, Entry] = {
    # ---- decode / cache fill: rows = batch rows of G * Tmax * hd elements
    # single launch (Tmax <= attn_decode_max_len() = 8,192): the last (b, g) slab starts past 2^31 elements
    "decode": Entry(_cache(260, 8, 8192, 128, 2), "kcache", 260, 8 * 8192 * 128, ("e31", "b32"),
                    peak=int(10.5 * GIB), dims=dict(B=260, G=8, H=_H, Tmax=8192, hd=128)),
    # split-KV: slab 135 starts at 2.26e9 elements = 4.5e9 bytes; + fp32 slices of one full row (2 x 0.5 GiB, twice)
    "decode_split": Entry(_cache(17, 8, 131072, 128, 2), "kcache", 17, 8 * 131072 * 128, ("e31", "b32"),
                          peak=11 * GIB, dims=dict(B=17, G=8, H=_H, Tmax=131072, hd=128)),
    # fp8 bytes cross 2^31 and 2^32 bytes (= elements); + the dequantised fp32 slices of one full row
    "decode_fp8": Entry(_cache(33, 8, 131072, 128, 1, scales=True), "kcache", 33, 8 * 131072 * 128,
                        ("e31", "b32", "e32"), peak=int(11.5 * GIB), dims=dict(B=33, G=8, H=_H, Tmax=131072, hd=128)),
    # ---- cross entropy: [N, ld] logits, V < ld; + one 1-GiB fp32 reference chunk and its logsumexp temporaries
    "ce_bf16": Entry({"logits": (85_504 * 50_304, 2)}, "logits", 85_504, 50_304, ("e31", "b32", "e32"),
                     peak=11 * GIB, dims=dict(N=85_504, V=50_257, ld=50_304)),
    "ce_fp32": Entry({"logits": (42_752 * 50_304, 4)}, "logits", 42_752, 50_304, ("e31", "b32"),
                     peak=10 * GIB, dims=dict(N=42_752, V=50_257, ld=50_304)),
    # ---- elementwise
    # gu + dact + dgu live at once in the backward (10 GiB), + the row chunks of the bitwise comparison:
    # the row-per-workgroup kernels (F / 8 >= 512, Llama's F) and the grid-stride kernels
    "swiglu_rows": Entry({"gu": (74_912 * 28_672, 2), "dact": (74_912 * 14_336, 2), "dgu": (74_912 * 28_672, 2),
                          "chunk": (9_362 * 28_672 + 9_362 * 14_336, 2)},
                         "gu", 74_912, 28_672, ("e31", "b32"), peak=int(11.5 * GIB), dims=dict(N=74_912, F=14_336)),
    "swiglu_grid": Entry({"gu": (1_073_800 * 2_000, 2), "dact": (1_073_800 * 1_000, 2), "dgu": (1_073_800 * 2_000, 2),
                          "chunk": (134_217 * 2_000 + 134_217 * 1_000, 2)},
                         "gu", 1_073_800, 2_000, ("e31", "b32"), peak=int(11.5 * GIB), dims=dict(N=1_073_800, F=1_000)),
    # n just past 2^31, seen as rows of 4,096 elements.  Three such tensors are 12 GiB + a little, so the
    # two-input ops (gelu_bwd, dropout_add) read the same tensor through both (read-only) arguments
    "flat": Entry({"x": (524_304 * 4_096, 2), "out": (524_304 * 4_096, 2), "chunk": (1 << 28, 2)}, "x", 524_304, 4_096,
                  ("e31", "b32"), peak=int(9.5 * GIB), dims=dict(n=524_304 * 4_096)),
    # ---- lora_head_bwd: dl rows 2^21 elements apart, 4.6e9 bytes, so lora_head_bwd_splits must raise S;
    #      + gpart [S, 16 V] fp32, upart, B, gB and one 1-GiB fp32 reference chunk
    "lora_head": Entry({"dl": (1_100 * (1 << 21), 2), "gB": (16 << 21, 4), "g0": (16 << 21, 4), "want_g": (16 << 21, 4),
                        "B": (16 << 21, 2), "B fp32": (16 << 21, 4), "sta": (1_100 * 4_160, 2),
                        "gpart": (5 * (16 << 21), 4), "upart": (2_048 * 1_100 * 16, 4), "ref chunk": (1 << 28, 4)},
                       "dl", 1_100, 1 << 21, ("e31", "b32"), peak=7 * GIB, dims=dict(R=1_100, V=1 << 21)),
    # ---- GEMM operand pitches: A is a [K or M, 256-wide] view of a wide allocation
    "wgrad_pitch": Entry({"a": (16_512 * (1 << 17), 2)}, "a", 16_512, 1 << 17, ("e31", "b32"), peak=5 * GIB,
                         gemm_pitches=(1 << 17,), dims=dict(K=16_512, M=256, N=256)),
    "gemm_nn_pitch": Entry({"a": (16_640 * (1 << 17), 2)}, "a", 16_640, 1 << 17, ("e31", "b32"), peak=5 * GIB,
                           gemm_pitches=(1 << 17,), dims=dict(M=16_640, K=256, N=256)),
    "gemm_nt_pitch": Entry({"a": (768 * (GEMM_NT_PITCH_LIMIT - 8), 2)}, "a", 768, GEMM_NT_PITCH_LIMIT - 8,
                           ("e31", "b32"), peak=7 * GIB, gemm_pitches=(GEMM_NT_PITCH_LIMIT - 8,),
                           dims=dict(M=768, K=256, N=256)),
    # 8 elements below the bound of part 2: TN (K = 256 rows) and NN (M = 256 rows)
    "wgrad_bound": Entry({"a": (256 * (GEMM_MAX_PITCH - 8), 2)}, "a", 256, GEMM_MAX_PITCH - 8, ("e31", "b32"),
                         peak=5 * GIB, gemm_pitches=(GEMM_MAX_PITCH - 8,), dims=dict(K=256, M=256, N=256)),
    "gemm_nn_bound": Entry({"a": (256 * (GEMM_MAX_PITCH - 8), 2)}, "a", 256, GEMM_MAX_PITCH - 8, ("e31", "b32"),
                           peak=5 * GIB, gemm_pitches=(GEMM_MAX_PITCH - 8,), dims=dict(M=256, K=256, N=256)),
}
