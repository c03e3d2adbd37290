"""The shape table of the large-extent GPU tests (tests/large_extent_shapes.py), checked without a
GPU: a later edit that shrinks a shape back under a boundary, lets a test outgrow its memory cap,
breaks the row selection or moves a GEMM pitch above the binding's bound fails here."""
import os
import re

import pytest
from large_extent_shapes import (B32, CAP, E31, E32, GEMM_MAX_PITCH, GEMM_NT_PITCH_LIMIT, N_RANDOM, SHAPES,
                                 boundary_rows, select_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(SHAPES)


@pytest.mark.parametrize("name", NAMES)
def test_crosses_the_boundaries_it_claims(name):
    e = SHAPES[name]
    n, size = e.tensors[e.main]
    assert n == e.rows * e.pitch, "the rows view covers the whole main tensor"
    assert e.crosses and set(e.crosses) <= {"e31", "b32", "e32"}
    assert ("e31" in e.crosses) == (n > E31)
    assert ("b32" in e.crosses) == (n * size > B32)
    assert ("e32" in e.crosses) == (n > E32)
    assert "e31" in e.crosses and "b32" in e.crosses       # every entry is past 2^31 elements and 2^32 bytes
    for b in e.boundaries():                               # and has rows on both sides of each boundary
        assert 0 < b // e.pitch < e.rows, (name, b)


@pytest.mark.parametrize("name", NAMES)
def test_stated_peak(name):
    e = SHAPES[name]
    assert e.tensor_bytes <= e.peak <= CAP, (name, e.tensor_bytes, e.peak)


@pytest.mark.parametrize("name", NAMES)
def test_row_selection_returns_the_straddling_rows(name):
    e = SHAPES[name]
    rows = select_rows(e, seed=3)
    assert rows == sorted(set(rows)) and all(0 <= r < e.rows for r in rows)
    assert {0, e.rows - 1} <= set(rows)
    for b in e.boundaries():
        r = b // e.pitch
        assert r * e.pitch <= b < (r + 1) * e.pitch                   # row r holds element b ...
        assert {r - 1, r, r + 1} & set(range(e.rows)) <= set(rows)    # ... and is there with its neighbours
        assert boundary_rows(e.rows, e.pitch, b) == [x for x in (r - 1, r, r + 1) if 0 <= x < e.rows]
    assert len(rows) >= min(e.rows // 2, N_RANDOM // 2)               # the random rows are in (few collide)
    assert select_rows(e, seed=3) == rows                             # seeded
    if e.rows > 4 * N_RANDOM:
        assert select_rows(e, seed=4) != rows


def test_gemm_pitches_are_within_the_binding_bound():
    src = open(os.path.join(ROOT, "csrc", "binding.cpp")).read()
    m = re.search(r"constexpr int64_t kMaxGemmPitch = (\d+);", src)
    assert m and int(m.group(1)) == GEMM_MAX_PITCH
    from building_llm_from_scratch_amd import ops
    assert ops.GEMM_MAX_PITCH == GEMM_MAX_PITCH                      # the planners' copy of the bound
    # the bound itself: the largest multiple of 8 elements whose worst per-lane byte offset,
    # (255 * ld + 8 * 3) * 2 of gemm_nn's A staging, stays below 2^32
    assert (255 * GEMM_MAX_PITCH + 24) * 2 < 1 << 32 <= (255 * (GEMM_MAX_PITCH + 8) + 24) * 2
    assert GEMM_MAX_PITCH % 8 == 0
    assert 256 * (GEMM_NT_PITCH_LIMIT - 8) * 2 < 1 << 31 <= 256 * GEMM_NT_PITCH_LIMIT * 2
    seen = 0
    for name, e in SHAPES.items():
        for p in e.gemm_pitches:
            assert p % 8 == 0 and p <= GEMM_MAX_PITCH, (name, p)
            seen += 1
    assert seen >= 5
    assert SHAPES["wgrad_bound"].pitch == SHAPES["gemm_nn_bound"].pitch == GEMM_MAX_PITCH - 8
