"""Kernels at offsets past 2^31 elements and 2^32 bytes.

Every test places a little work at far offsets of a large, mostly untouched allocation (the shape
table, its memory budgets and what is left out: tests/large_extent_shapes.py), so it costs memory,
not time.  Inputs are generated in place on the device, the oracles of ops/reference.py run on
slices (the checked rows, or the whole tensor in row chunks of at most 1 GiB of fp32), and the
allowances are those of the existing test of the same op.  Caches, pitch padding and caller-owned
outputs are filled with NaN (e4m3fn caches: bytes 0x7F) before the inputs are written; afterwards
the non-NaN elements are counted per row: a read at a wrapped address puts a NaN into an output, a
write at one leaves a stray non-NaN.  Elementwise kernels, whose outputs the op allocates, are
checked against the oracle on the selected rows and bit for bit, over the whole tensor, against
the same kernel run on row chunks (small offsets)."""
import contextlib
import gc
import math

import pytest
import torch
from large_extent_shapes import B32, E31, GEMM_NT_PITCH_LIMIT, GIB, SHAPES, boundary_rows, select_rows
from numerics import check_close, check_elem

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
K_DECODE = 3.0                              # tests/test_decode_split_gpu.py, tests/test_kv_fp8_gpu.py
K_OF = {1: 2.0, 2: 3.0, 4: 5.0}             # tests/test_kernels_gpu.py _close classes
LSE_TOL = dict(rtol=1e-5, atol=2e-5)        # tests/test_kernels_gpu.py
K_GEMM = 3.0                                # tests/test_kernels_gpu.py test_wgrad_gemm / test_gemm_nn / test_gemm_nt
NAN8 = 0x7F                                 # e4m3fn NaN
NAN = float("nan")
REF_CHUNK = 1 << 28                         # elements of one fp32 reference chunk (1 GiB)
COUNT_CHUNK = 1 << 25                       # elements of one canary-count piece


@pytest.fixture(autouse=True)
def _ext_and_cleanup():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)
    yield
    gc.collect()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _budget(name):
    """Skip only when the device has less free memory than the entry's stated peak + 2 GiB; report
    the test's own measured peak (above what the session already held) and hold it to the stated one."""
    e = SHAPES[name]
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < e.peak + 2 * GIB:
        pytest.skip(f"{name}: {free / GIB:.1f} GiB free, needs {e.peak / GIB:.1f} + 2 GiB")
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()      # what earlier tests of the session keep alive (cached models)
    yield e
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    print(f"PEAK {name}: {peak / GIB:.2f} GiB of {e.peak / GIB:.2f} GiB stated")
    assert peak <= e.peak, (name, peak, e.peak)


def _k():
    return torch.ops.bllm


def _close(a, b, dt, scale=1, name=""):
    check_close(a, b, dt, k=K_OF[scale], name=name)


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _canary(*shape, dt):
    if dt == F8:
        return torch.full(shape, NAN8, dtype=torch.uint8, device=DEV).view(F8)
    return torch.empty(*shape, dtype=dt, device=DEV).fill_(NAN)


def _valid_per_row(t):
    """Non-canary elements per leading-dim row of a contiguous tensor -> int64 [rows] (CPU), counted
    in pieces of at most COUNT_CHUNK elements (the reduction widens its bool input to int64)."""
    t = t.view(torch.uint8) if t.dtype == F8 else t
    rows, per = t.shape[0], t[0].numel()
    sub = per if per <= COUNT_CHUNK else math.gcd(per, COUNT_CHUNK)     # rows longer than a piece: in sub-rows
    flat = t.reshape(-1, sub)
    step = max(1, COUNT_CHUNK // sub)
    out = []
    for r0 in range(0, flat.shape[0], step):
        c = flat[r0:r0 + step]
        out.append(((c != NAN8) if c.dtype == torch.uint8 else (c == c)).sum(1))
    return torch.cat(out).view(rows, per // sub).sum(1).cpu()


def _row_chunks(rows, per_row):
    step = max(1, REF_CHUNK // per_row)
    return [(r0, min(r0 + step, rows)) for r0 in range(0, rows, step)]


# =================================================================== decode and cache fill
def _positions(e, shared=None):
    """Rows 0, the one at the 2^31-element boundary and B - 1 get 5, 1000 and Tmax - 1; every other
    row appends at position 0 (``shared``: that position for all rows)."""
    B, Tmax = e.dims["B"], e.dims["Tmax"]
    if shared is not None:
        return [shared] * B
    pos = [0] * B
    pos[0] = 5
    pos[E31 // e.pitch] = 1000
    pos[B - 1] = Tmax - 1
    return pos


def _special(e):
    """The individually checked batch rows: first, last, around every boundary."""
    s = {0, 1, e.rows - 2, e.rows - 1}
    for b in e.boundaries():
        s |= set(boundary_rows(e.rows, e.pitch, b))
    return sorted(s)


def _check_rows(out, want, dt, special, name):
    check_close(out, want, dt, k=K_DECODE, name=name)                  # every row
    for b in special:                                                  # and the edge rows on their own
        check_close(out[b], want[b], dt, k=K_DECODE, name=f"{name} row {b}")


def _run_append(name, dt, op, shared=None):
    with _budget(name) as e:
        B, G, H, Tmax, hd = (e.dims[k] for k in ("B", "G", "H", "Tmax", "hd"))
        pos = _positions(e, shared)
        kc, vc = _canary(B, G, Tmax, hd, dt=dt), _canary(B, G, Tmax, hd, dt=dt)
        if shared is not None:
            kc[:, :, :shared].normal_()
            vc[:, :, :shared].normal_()
        else:
            for b, p in enumerate(pos):
                if p:
                    kc[b, :, :p].normal_()
                    vc[b, :, :p].normal_()
        qkv = torch.empty(B, (H + 2 * G) * hd, dtype=dt, device=DEV).normal_()
        pos_t = torch.tensor(pos[:1] if shared is not None else pos, dtype=torch.int32, device=DEV)
        pre = {b: (kc[b, :, :p].clone(), vc[b, :, :p].clone()) for b, p in enumerate(pos) if p}
        out = getattr(_k(), op)(qkv, kc, vc, pos_t, H, G)
        torch.cuda.synchronize()
        # the keys that were there are as they were, bit for bit (the oracle below reads them back)
        for b, (k0, v0) in pre.items():
            assert _same_bits(kc[b, :, :pos[b]], k0) and _same_bits(vc[b, :, :pos[b]], v0), b
        del pre, k0, v0                                    # (the loop's names held the last, longest row)
        # the appended k / v, bit for bit, at [b, :, pos[b]]
        rows = qkv.view(B, H + 2 * G, hd)
        at = torch.tensor(pos, device=DEV)
        bi = torch.arange(B, device=DEV)
        assert _same_bits(kc[bi, :, at], rows[:, H:H + G]) and _same_bits(vc[bi, :, at], rows[:, H + G:])
        # nothing else written: prefill + one appended position per row
        expect = torch.tensor([(p + 1) * G * hd for p in pos])
        assert torch.equal(_valid_per_row(kc), expect) and torch.equal(_valid_per_row(vc), expect)
        # every row against the oracle, on fp32 copies of the row's keys (the kernel left 0..p-1
        # as they were; the oracle rewrites row p itself)
        want = torch.empty(B, H * hd, device=DEV)
        for b, p in enumerate(pos):
            ks, vs = kc[b:b + 1, :, :p + 1].float(), vc[b:b + 1, :, :p + 1].float()
            ks[:, :, p] = NAN
            vs[:, :, p] = NAN
            want[b] = ref.attn_decode_append_rows(qkv[b:b + 1].float(), ks, vs, torch.tensor([p]), H, G)[0]
            del ks, vs
        assert torch.isfinite(out.float()).all()
        _check_rows(out, want, dt, _special(e), f"{op} {name}")
        # a row at position 0 attends over its own key alone: its new V, per query head
        zero = [b for b, p in enumerate(pos) if p == 0]
        if zero:
            own = rows[zero][:, H + G:].repeat_interleave(H // G, dim=1).reshape(len(zero), H * hd)
            check_close(out[zero], own.float(), dt, k=K_DECODE, name=f"{op} {name} pos 0 rows")


def _run_plain(name, dt, op, L):
    """The ops with one length for all rows: the first L positions of every row hold keys."""
    with _budget(name) as e:
        B, G, H, Tmax, hd = (e.dims[k] for k in ("B", "G", "H", "Tmax", "hd"))
        kc, vc = _canary(B, G, Tmax, hd, dt=dt), _canary(B, G, Tmax, hd, dt=dt)
        kc[:, :, :L].normal_()
        vc[:, :, :L].normal_()
        q = torch.empty(B, H, hd, dtype=dt, device=DEV).normal_()
        out = getattr(_k(), op)(q, kc, vc, L)
        torch.cuda.synchronize()
        expect = torch.full((B,), L * G * hd)
        assert torch.equal(_valid_per_row(kc), expect) and torch.equal(_valid_per_row(vc), expect)
        want = torch.cat([ref.attn_decode(q[a:b].float(), kc[a:b, :, :L].float(), vc[a:b, :, :L].float(), L)
                          for a, b in _row_chunks(B, 4 * G * L * hd)])      # k, v and their per-head copies
        assert torch.isfinite(out.float()).all()
        _check_rows(out, want, dt, _special(e), f"{op} {name}")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_attn_decode_single_launch(dt):
    assert SHAPES["decode"].dims["Tmax"] <= ops.DECODE_SPLIT_MIN       # the single-launch kernels' limit
    _run_plain("decode", dt, "attn_decode", 1000)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_attn_decode_append_rows(dt):
    _run_append("decode", dt, "attn_decode_append_rows")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_attn_decode_split(dt):
    _run_plain("decode_split", dt, "attn_decode_split", 9000)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("shared", [None, 1000])
def test_attn_decode_append_split(dt, shared):
    _run_append("decode_split", dt, "attn_decode_append_split", shared)


def _quantised(G, n, hd, scale=1.0):
    """Random rows in the fp8 cache format, made in key chunks (the oracle quantises in fp64)."""
    q8 = torch.empty(G, n, hd, dtype=F8, device=DEV)
    s = torch.empty(G, n, device=DEV)
    for a in range(0, n, 16384):
        b = min(a + 16384, n)
        q, sc = ref.kv_quantize_rows(torch.randn(G, b - a, hd, device=DEV) * scale)
        q8.view(torch.uint8)[:, a:b] = q.view(torch.uint8)
        s[:, a:b] = sc
    return q8, s


@pytest.mark.parametrize("dt", [BF16, F16])
def test_attn_decode_append_rows_fp8(dt):
    name = "decode_fp8"
    with _budget(name) as e:
        B, G, H, Tmax, hd = (e.dims[k] for k in ("B", "G", "H", "Tmax", "hd"))
        pos = _positions(e)
        assert pos[B32 // e.pitch] == Tmax - 1             # the row at 2^32 bytes is the last row
        k8, v8 = _canary(B, G, Tmax, hd, dt=F8), _canary(B, G, Tmax, hd, dt=F8)
        ks, vs = _canary(B, G, Tmax, dt=F32), _canary(B, G, Tmax, dt=F32)
        for b, p in enumerate(pos):
            if p:
                for c8, cs, sc in ((k8, ks, 1.0), (v8, vs, 2.0)):
                    q, s = _quantised(G, p, hd, sc)
                    c8.view(torch.uint8)[b, :, :p] = q.view(torch.uint8)
                    cs[b, :, :p] = s
                    del q, s
        qkv = torch.empty(B, (H + 2 * G) * hd, dtype=dt, device=DEV).normal_()
        pos_t = torch.tensor(pos, dtype=torch.int32, device=DEV)
        pre = {b: [t[b, :, :p].clone() for t in (k8, v8, ks, vs)] for b, p in enumerate(pos) if p}
        out = _k().attn_decode_append_rows_fp8(qkv, k8, ks, v8, vs, pos_t, H, G)
        torch.cuda.synchronize()
        # the rows that were there are as they were, bytes and scale bits (the oracle below reads them back)
        for b, saved in pre.items():
            for t, t0 in zip((k8, v8, ks, vs), saved):
                assert _same_bits(t[b, :, :pos[b]], t0), b
        del pre, saved, t0
        eb = torch.tensor([(p + 1) * G * hd for p in pos])
        es = torch.tensor([(p + 1) * G for p in pos])
        assert torch.equal(_valid_per_row(k8), eb) and torch.equal(_valid_per_row(v8), eb)
        assert torch.equal(_valid_per_row(ks), es) and torch.equal(_valid_per_row(vs), es)
        want = torch.empty(B, H * hd, device=DEV)
        for b, p in enumerate(pos):
            c = [t[b:b + 1, :, :p + 1].clone() for t in (k8, v8, ks, vs)]
            c[0].view(torch.uint8)[:, :, p] = NAN8         # the oracle writes position p itself
            c[1].view(torch.uint8)[:, :, p] = NAN8
            c[2][:, :, p] = NAN
            c[3][:, :, p] = NAN
            want[b] = ref.attn_decode_append_rows_fp8(qkv[b:b + 1].float(), c[0], c[1], c[2], c[3],
                                                      torch.tensor([p]), H, G)[0]
            # the appended bytes and scale bits are the oracle's
            assert _same_bits(k8[b, :, p], c[0][0, :, p]) and _same_bits(v8[b, :, p], c[1][0, :, p]), b
            assert _same_bits(ks[b, :, p], c[2][0, :, p]) and _same_bits(vs[b, :, p], c[3][0, :, p]), b
            del c
        assert torch.isfinite(out.float()).all()
        _check_rows(out, want, dt, _special(e), "attn_decode_append_rows_fp8")


def _fill_lengths(e):
    """Lengths {0, 1, 300}: 1 at the first row, 300 at the rows holding each boundary and at the
    last row, 1 after a boundary row, 0 everywhere else (the row before a boundary included)."""
    lens = [0] * e.rows
    lens[0] = 1
    for b in e.boundaries():
        r = b // e.pitch
        lens[r] = 300
        if r + 1 < e.rows:
            lens[r + 1] = 1
    lens[e.rows - 1] = 300
    return lens


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("name", ["decode", "decode_split"])
def test_kv_cache_fill_varlen(name, dt):
    with _budget(name) as e:
        B, G, H, Tmax, hd = (e.dims[k] for k in ("B", "G", "H", "Tmax", "hd"))
        lens = _fill_lengths(e)
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
        qkv = torch.empty(sum(lens), (H + 2 * G) * hd, dtype=dt, device=DEV).normal_()
        kc, vc = _canary(B, G, Tmax, hd, dt=dt), _canary(B, G, Tmax, hd, dt=dt)
        ops.kv_cache_fill_varlen(qkv, cu, kc, vc)
        torch.cuda.synchronize()
        expect = torch.tensor([n * G * hd for n in lens])
        assert torch.equal(_valid_per_row(kc), expect) and torch.equal(_valid_per_row(vc), expect)
        filled = [b for b, n in enumerate(lens) if n]
        wk, wv = _canary(len(filled), G, 300, hd, dt=dt), _canary(len(filled), G, 300, hd, dt=dt)
        ref.kv_cache_fill_varlen(qkv, [0] + torch.tensor([lens[b] for b in filled]).cumsum(0).tolist(), wk, wv)
        assert _same_bits(kc[filled, :, :300], wk) and _same_bits(vc[filled, :, :300], wv)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_kv_cache_fill_varlen_fp8(dt):
    with _budget("decode_fp8") as e:
        B, G, H, Tmax, hd = (e.dims[k] for k in ("B", "G", "H", "Tmax", "hd"))
        lens = _fill_lengths(e)
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
        qkv = torch.empty(sum(lens), (H + 2 * G) * hd, dtype=dt, device=DEV).normal_()
        k8, v8 = _canary(B, G, Tmax, hd, dt=F8), _canary(B, G, Tmax, hd, dt=F8)
        ks, vs = _canary(B, G, Tmax, dt=F32), _canary(B, G, Tmax, dt=F32)
        ops.kv_cache_fill_varlen(qkv, cu, k8, v8, scales=(ks, vs))
        torch.cuda.synchronize()
        eb, es = torch.tensor([n * G * hd for n in lens]), torch.tensor([n * G for n in lens])
        assert torch.equal(_valid_per_row(k8), eb) and torch.equal(_valid_per_row(v8), eb)
        assert torch.equal(_valid_per_row(ks), es) and torch.equal(_valid_per_row(vs), es)
        filled = [b for b, n in enumerate(lens) if n]
        n = len(filled)
        w = (_canary(n, G, 300, hd, dt=F8), _canary(n, G, 300, hd, dt=F8), _canary(n, G, 300, dt=F32),
             _canary(n, G, 300, dt=F32))
        ref.kv_cache_fill_varlen_fp8(qkv.float(), [0] + torch.tensor([lens[b] for b in filled]).cumsum(0).tolist(), *w)
        for got, exp in zip((k8, v8, ks, vs), w):
            assert _same_bits(got[filled, :, :300], exp)


# =================================================================== cross entropy
@pytest.mark.parametrize("name,dt", [("ce_bf16", BF16), ("ce_fp32", F32)])
def test_cross_entropy(name, dt):
    with _budget(name) as e:
        N, V, ld = e.dims["N"], e.dims["V"], e.dims["ld"]
        buf = _canary(N, ld, dt=dt)                        # the pad columns [V, ld) stay NaN
        logits = buf[:, :V]
        chunks = _row_chunks(N, V)
        for a, b in chunks:
            logits[a:b].normal_(0.0, 3.0)
        tgt = torch.randint(0, V, (N,), device=DEV)
        tgt[3] = -100
        tgt[E31 // ld] = -100                              # an ignored target on a straddling row
        loss, lse = ops.ce_fwd(logits, tgt)
        parts = [ref.ce_fwd(logits[a:b], tgt[a:b]) for a, b in chunks]
        loss0, lse0 = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        del parts
        check_elem(loss, loss0, **LSE_TOL, name=f"{name} loss")
        check_elem(lse, lse0, **LSE_TOL, name=f"{name} lse")
        assert float(loss[E31 // ld]) == 0.0 and float(loss[3]) == 0.0
        full = torch.full((N,), V)
        assert torch.equal(_valid_per_row(buf), full)
        # backward in place: the checked rows are saved first
        rows = select_rows(e, seed=1)
        assert E31 // ld in rows
        saved = logits[rows].clone()
        scale = torch.tensor([0.5], device=DEV)
        ops.ce_bwd_(logits, tgt, lse, scale)
        torch.cuda.synchronize()
        g0 = ref.ce_bwd_(saved.float(), tgt[rows], lse0[rows], scale)
        _close(logits[rows], g0, dt, 2, name=f"{name} dlogits")
        assert not logits[E31 // ld].any()                 # the ignored row's gradient is zero
        assert torch.equal(_valid_per_row(buf), full)      # pad columns of every row still canary
        assert torch.isnan(buf[rows][:, V:]).all()


# =================================================================== elementwise
def _chunkwise_same(big, small_of, rows, per_row, name):
    """``big`` [rows, ...] equals, bit for bit, the same kernel run on each row chunk alone."""
    for a, b in _row_chunks(rows, per_row):
        assert torch.equal(_bits(big[a:b]), _bits(small_of(a, b))), f"{name}: rows {a}..{b}"


def _regen(shape, dt, seed):
    """The same random tensor for the same seed: dact is overwritten by swiglu_bwd_act, and a second
    full copy would not fit the cap, so its row chunks are generated again when they are needed."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.empty(*shape, dtype=dt, device=DEV).normal_(generator=g)


def _run_swiglu(name, rows_path):
    """swiglu_fwd, swiglu_bwd and swiglu_bwd_act: the oracle on the selected rows, and every output
    bit for bit, over the whole tensor, against the same kernel run on row chunks."""
    dt = BF16
    with _budget(name) as e:
        N, F = e.dims["N"], e.dims["F"]
        assert (F // 8 >= 512) == rows_path                # row-per-workgroup or grid-stride kernels
        rows = select_rows(e, seed=2)
        chunks = _row_chunks(N, 2 * F)
        gu = torch.empty(N, 2 * F, dtype=dt, device=DEV).normal_()
        act = ops.swiglu_fwd(gu)
        _close(act[rows], ref.swiglu_fwd(gu[rows].float()), dt, name=f"swiglu {name}")
        _chunkwise_same(act, lambda a, b: ops.swiglu_fwd(gu[a:b]), N, 2 * F, f"swiglu {name}")
        del act
        dact = torch.empty(N, F, dtype=dt, device=DEV)
        for a, b in chunks:
            dact[a:b] = _regen((b - a, F), dt, 100 + a)
        dact_rows = dact[rows].float()
        dgu = ops.swiglu_bwd(gu, dact)
        _close(dgu[rows], ref.swiglu_bwd(gu[rows].float(), dact_rows), dt, 2, name=f"swiglu_bwd {name}")
        _chunkwise_same(dgu, lambda a, b: ops.swiglu_bwd(gu[a:b], dact[a:b]), N, 2 * F, f"swiglu_bwd {name}")
        dgu_rows = dgu[rows].clone()
        del dgu
        # fused variant: the same dgu, and act written in place of dact
        dgu2 = ops.swiglu_bwd_act(gu, dact)
        assert torch.equal(dgu2[rows], dgu_rows)
        _close(dgu2[rows], ref.swiglu_bwd(gu[rows].float(), dact_rows), dt, 2, name=f"swiglu_bwd_act {name}")
        _chunkwise_same(dgu2, lambda a, b: ops.swiglu_bwd(gu[a:b], _regen((b - a, F), dt, 100 + a)), N, 2 * F,
                        f"swiglu_bwd_act {name} dgu")
        del dgu2
        _chunkwise_same(dact, lambda a, b: ops.swiglu_fwd(gu[a:b]), N, 2 * F, f"swiglu_bwd_act {name} act")


def test_swiglu_row_kernels():
    _run_swiglu("swiglu_rows", rows_path=True)


def test_swiglu_grid_stride_kernels():
    _run_swiglu("swiglu_grid", rows_path=False)


def test_gelu_and_dropout_add():
    dt = BF16
    with _budget("flat") as e:
        n, W = e.dims["n"], e.pitch
        assert n > E31
        rows = select_rows(e, seed=4)
        x = torch.empty(e.rows, W, dtype=dt, device=DEV).normal_()
        xr = x[rows].float()
        g = ops.gelu_fwd(x)
        _close(g[rows], ref.gelu_fwd(xr), dt, name="gelu")
        _chunkwise_same(g, lambda a, b: ops.gelu_fwd(x[a:b]), e.rows, W, "gelu")
        del g
        d = ops.gelu_bwd(x, x)                             # f and dg: the same (read-only) tensor
        _close(d[rows], ref.gelu_bwd(xr, xr), dt, name="gelu_bwd")
        _chunkwise_same(d, lambda a, b: ops.gelu_bwd(x[a:b], x[a:b]), e.rows, W, "gelu_bwd")
        del d
        p, seed, offset = 0.1, 1234, 777
        o = ops.dropout_add(x, x, p, seed, offset)
        want = torch.stack([ref.dropout_add(x[r].float(), x[r].float(), p, seed, offset + r * W) for r in rows])
        _close(o[rows], want, dt, name="dropout_add")
        for r in rows:                                     # the keep mask itself, on windows: kept <=> out != x
            keep = ref.drop_keep_mask(seed, offset + r * W, W, p, device=DEV)
            nz = x[r] != 0
            assert torch.equal((o[r] != x[r])[nz], keep[nz]), r
        _chunkwise_same(o, lambda a, b: ops.dropout_add(x[a:b], x[a:b], p, seed, offset + a * W), e.rows, W,
                        "dropout_add")


# =================================================================== lora_head_bwd
@pytest.mark.parametrize("accumulate", [False, True])
def test_lora_head_bwd(accumulate):
    """tests/test_kernels_gpu.py::test_lora_head_bwd with dl rows 2^21 elements apart (4.6e9 bytes:
    the row ranges must be split further to fit the kernel's 32-bit buffer offsets), the fp32
    matmul oracle formed in row chunks."""
    dt, r = BF16, 16
    with _budget("lora_head") as e:
        R, V = e.dims["R"], e.dims["V"]
        assert R * V * 2 > B32
        dl = torch.empty(R, V, dtype=dt, device=DEV).normal_(0.0, 0.01)
        sta = torch.randn(R, 4160, device=DEV).to(dt)
        st = sta[:, 4096:4096 + r]
        B = torch.empty(r, V, dtype=dt, device=DEV).normal_(0.0, 0.1)
        g0 = torch.randn(V, r, device=DEV)
        gB = g0.clone().t()
        u = _canary(R, r, dt=dt)
        ops.lora_head_bwd_(dl, st, B, u, gB, accumulate)
        torch.cuda.synchronize()
        Bf = B.float()
        want_u = torch.empty(R, r, device=DEV)
        want_g = g0.t().clone() if accumulate else torch.zeros(r, V, device=DEV)
        for a, b in _row_chunks(R, V):
            dlf = dl[a:b].float()
            want_u[a:b] = dlf @ Bf.t()
            want_g += st[a:b].float().t() @ dlf
            del dlf
        _close(u, want_u, dt, 4, name="lora_head_bwd u")
        check_elem(gB, want_g, rtol=1e-4, atol=1e-4 * want_g.abs().max().item(), name="lora_head_bwd gB")
        rows = select_rows(e, seed=5)
        _close(u[rows], want_u[rows], dt, 4, name="lora_head_bwd u, selected rows")


# =================================================================== GEMM operand pitches
def _pitched(rows, cols, pitch, dt, col0=32):
    """[rows, cols] view, rows ``pitch`` elements apart, of a NaN-filled allocation."""
    buf = _canary(rows, pitch, dt=dt)
    v = buf[:, col0:col0 + cols]
    v.normal_()
    return buf, v


def _gemm_check(buf, c, expect, odt, cols, name):
    torch.cuda.synchronize()
    check_close(c, expect, odt, k=K_GEMM, name=name)
    assert torch.equal(_valid_per_row(buf), torch.full((buf.shape[0],), cols))      # the operand is as it was


@pytest.mark.parametrize("name", ["wgrad_pitch", "wgrad_bound"])
@pytest.mark.parametrize("dt", [BF16, F16])
def test_wgrad_gemm_wide_pitch(name, dt):
    """c (+)= a^T b with a = [K, 256] rows up to 8.4e6 elements apart: whole K on the 4-wave kernel
    (S = 1), split-K on it (S = 3) and on the 8-wave kernel (S = 8), and the split tail."""
    with _budget(name) as e:
        K, M, N = e.dims["K"], e.dims["M"], e.dims["N"]
        buf, a = _pitched(K, M, e.pitch, dt)
        assert a.stride(0) == e.pitch and ops.wgrad_gemm_ok(a, torch.empty(K, N, dtype=dt, device=DEV),
                                                            torch.empty(M, N, device=DEV))
        b = torch.randn(K, N, device=DEV).to(dt)
        ab = a.double().t() @ b.double()
        splits = [1] + ([3, 8] if K // 128 >= 8 else [2])
        for S, odt, accumulate in [(s, o, acc) for s in splits for o, acc in ((F32, True), (dt, False))]:
            c = torch.randn(M, N, device=DEV).to(odt)
            expect = ab + (c.double() if accumulate else 0)
            ops.wgrad_gemm_(a, b, c, accumulate, S)
            _gemm_check(buf, c, expect, odt, M, f"wgrad {name} S {S}")
        for odt, accumulate in ((F32, False), (dt, True)):
            c = torch.randn(M, N, device=DEV).to(odt)
            expect = ab + (c.double() if accumulate else 0)
            _k().wgrad_gemm_tail_(a, b, c, accumulate, 0, 2)
            _gemm_check(buf, c, expect, odt, M, f"wgrad tail {name}")
        # the wide pitch on the b operand
        c = torch.randn(N, M, device=DEV)
        ops.wgrad_gemm_(b, a, c, False, 1)
        _gemm_check(buf, c, ab.t(), F32, M, f"wgrad {name} wide b")


@pytest.mark.parametrize("name", ["gemm_nn_pitch", "gemm_nn_bound"])
@pytest.mark.parametrize("dt", [BF16, F16])
def test_gemm_nn_wide_pitch(name, dt):
    with _budget(name) as e:
        M, K, N = e.dims["M"], e.dims["K"], e.dims["N"]
        buf, a = _pitched(M, K, e.pitch, dt)
        b = torch.randn(K, N, device=DEV).to(dt)
        assert a.stride(0) == e.pitch and ops.gemm_nn_ok(a, b)
        ab = a.double() @ b.double()
        for odt, accumulate in ((F32, True), (dt, False)):
            c = torch.randn(M, N, device=DEV).to(odt)
            expect = ab + (c.double() if accumulate else 0)
            ops.gemm_nn_(a, b, c, accumulate)
            _gemm_check(buf, c, expect, odt, K, f"gemm_nn {name}")
            rows = select_rows(e, seed=6)
            check_close(c[rows], expect[rows], odt, k=K_GEMM, name=f"gemm_nn {name}, selected rows")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_gemm_nt_pitch_under_and_over_the_guard(dt):
    name = "gemm_nt_pitch"
    with _budget(name) as e:
        M, K, N = e.dims["M"], e.dims["K"], e.dims["N"]
        assert 256 * e.pitch * 2 < E31 <= 256 * (e.pitch + 8) * 2
        buf, a = _pitched(M, K, e.pitch, dt, col0=0)
        b = torch.randn(N, K, device=DEV).to(dt)
        ab = a.double() @ b.double().t()
        for odt, accumulate in ((F32, True), (dt, False)):
            c = torch.randn(M, N, device=DEV).to(odt)
            expect = ab + (c.double() if accumulate else 0)
            ops.gemm_nt_(a, b, c, accumulate)
            _gemm_check(buf, c, expect, odt, K, f"gemm_nt {name}")
        del buf, a
        # just over the guard: refused by the binding, nothing launched (the allocation stays uninitialised)
        over = torch.empty(256, GEMM_NT_PITCH_LIMIT, dtype=dt, device=DEV)[:, :K]
        c = torch.zeros(256, N, device=DEV)
        for args in ((over, b, c, False), (b, over, c, False)):
            with pytest.raises(RuntimeError, match="gemm_nt_"):
                _k().gemm_nt_(*args)
        assert not c.any()
