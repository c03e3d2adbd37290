"""HIP kernels vs the reference on the code paths and arguments a training run takes.  GPU only.

tests/test_kernels_gpu.py keeps its shapes small; several launchers switch to another path above
those sizes (a capped grid that loops, several rows per workgroup, the 16-byte vector kernels) or
for other arguments (even / > 2^33 dropout offsets, a device-side decode position, padded logit
rows).  Each test here names the launcher rule that sends its shape down the path in question.
Allowances are the classes of test_kernels_gpu.py (``K_OF`` / ``K_MAX`` / ``LSE_TOL``), the class
of the existing test of the same kernel."""
import math

import pytest
import torch
from numerics import check_close, check_elem
from test_kernels_gpu import K_MAX, K_OF, LSE_TOL

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16, F32]
ES = {BF16: 2, F16: 2, F32: 4}          # element size; 16 // ES = elements per 16-byte vector


def _close(a, b, dt, scale=1.0, name=""):
    k = K_OF[scale]
    assert k <= K_MAX
    check_close(a, b, dt, k=k, name=name)


def _bits(t):
    """The tensor's bit pattern as integers: equality that tells NaNs and signed zeros apart."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b.to(a.device)))


def _f(t):
    """An fp32 CPU copy (never an alias of ``t``), the oracle's input."""
    return None if t is None else t.detach().to("cpu", torch.float32, copy=True)


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


# ------------------------------------------------------------------ 1. norm backward, rows > workgroups
# norm_bwd_num_wg caps the grid at MAX_BWD_WG = 1,024 workgroups and rows are grid-strided over
# them: N = 2,051 -> workgroups 0..2 take 3 rows (LDS parities 0, 1, 0), the rest 2, and every
# workgroup's prefetch looks one row past its last; N = 1,025 -> workgroup 0 takes 2 rows.
# bwd_dispatch picks the variant by 16-byte vectors per row: < 256 -> ceil(v / 64) waves with the
# next-row register prefetch (PF); 256 / 512 / 1,024 -> 4 waves with NV = 1 / 2 / 4.
NORM_ROWS = [2051, 1025]
NORM_VECS = [8, 160, 256, 512, 1024]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("vecs", NORM_VECS)
@pytest.mark.parametrize("N", NORM_ROWS)
def test_rmsnorm_bwd_rows_per_workgroup(dt, vecs, N):
    d = vecs * (16 // ES[dt])
    x = torch.randn(N, d, device=DEV).to(dt)
    w = (1 + 0.1 * torch.randn(d, device=DEV)).to(dt)
    dy = torch.randn(N, d, device=DEV).to(dt)
    acc = torch.randn(N, d, device=DEV).to(dt)
    y, r = ops.rmsnorm_fwd(x, w, 1e-5)
    y0, r0 = ref.rmsnorm_fwd(_f(x), _f(w), 1e-5)
    _close(y, y0, dt, name="y")
    check_elem(r, r0, rtol=2e-5, atol=0, name="rstd")
    dx0, dw0 = ref.rmsnorm_bwd(_f(dy), _f(x), _f(w), r0, None)
    # the reference adds dx_acc to its fp32 dx as its last step: the same sum, formed once here
    want_dx = {False: dx0, True: dx0 + _f(acc)}
    for with_acc in (True, False):
        dx, dw = ops.rmsnorm_bwd(dy, x, w, r, acc if with_acc else None)
        _close(dx, want_dx[with_acc], dt, 2, name=f"dx acc={with_acc}")
        _close(dw, dw0, dt, 2, name=f"dw acc={with_acc}")
    # weight gradient written / accumulated straight into a parameter-dtype buffer
    for accumulate in (False, True):
        out = torch.randn(d, device=DEV).to(dt)
        expect = dw0 + (_f(out) if accumulate else 0)
        dx, _ = ops.rmsnorm_bwd(dy, x, w, r, acc if accumulate else None, out, accumulate)
        _close(out, expect, dt, 4, name=f"dw_out acc={accumulate}")
        _close(dx, want_dx[accumulate], dt, 2, name=f"dx (dw_out) acc={accumulate}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("vecs", NORM_VECS)
@pytest.mark.parametrize("N", NORM_ROWS)
def test_layernorm_bwd_rows_per_workgroup(dt, vecs, N):
    d = vecs * (16 // ES[dt])
    x = (torch.randn(N, d, device=DEV) + 0.5).to(dt)
    w = (1 + 0.1 * torch.randn(d, device=DEV)).to(dt)
    b = (0.1 * torch.randn(d, device=DEV)).to(dt)
    dy = torch.randn(N, d, device=DEV).to(dt)
    acc = torch.randn(N, d, device=DEV).to(dt)
    y, m, r = ops.layernorm_fwd(x, w, b, 1e-5)
    y0, m0, r0 = ref.layernorm_fwd(_f(x), _f(w), _f(b), 1e-5)
    _close(y, y0, dt, name="y")
    dx0, dw0, db0 = ref.layernorm_bwd(_f(dy), _f(x), _f(w), m0, r0, None)
    want_dx = {False: dx0, True: dx0 + _f(acc)}     # as the reference's last step, see above
    for with_acc in (False, True):
        dx, dw, db = ops.layernorm_bwd(dy, x, w, m, r, acc if with_acc else None)
        _close(dx, want_dx[with_acc], dt, 2, name=f"dx acc={with_acc}")
        _close(dw, dw0, dt, 2, name=f"dw acc={with_acc}")
        _close(db, db0, dt, 2, name=f"db acc={with_acc}")
    for accumulate in (False, True):
        ow, ob = torch.randn(d, device=DEV).to(dt), torch.randn(d, device=DEV).to(dt)
        ew = dw0 + (_f(ow) if accumulate else 0)
        eb = db0 + (_f(ob) if accumulate else 0)
        dx, _, _ = ops.layernorm_bwd(dy, x, w, m, r, acc if accumulate else None, ow, ob, accumulate)
        _close(ow, ew, dt, 4, name=f"dw_out acc={accumulate}")
        _close(ob, eb, dt, 4, name=f"db_out acc={accumulate}")
        _close(dx, want_dx[accumulate], dt, 2, name=f"dx (dw_out) acc={accumulate}")


# ------------------------------------------------------------------ 2. AdamW, 16-byte vector path
# adamw_launch: n % 4 == 0 -> adamw_k<P, G, 4, 2> on nv = n / 4 vectors, min(ceil(nv / 512), 2048)
# workgroups of 256 threads x 2 unrolled vectors: nv = 1 a single lane; nv = 259 the second
# unroll half in range for lanes 0..2 only; nv = 513 a second workgroup with one vector;
# nv = 2048 * 512 + 512 + 5 a second grid-stride pass of one full workgroup and a ragged one.
ADAMW_N = [4, 4 * 259, 4 * 513, 4 * (2048 * 512 + 512 + 5)]
# (param, grad, fp32 master): FusedAdamW keeps a master for every 16-bit parameter and gradient
# shards have the parameter dtype in every engine (local, DDP, ZeRO, FSDP), so the first three are
# all that training produces; the master-less bf16 form is the kernel's remaining branch
ADAMW_DT = [(BF16, BF16, True), (F16, F16, True), (F32, F32, False), (BF16, BF16, False)]
ALIGN = 64      # models/flat.py: every slot of a flat buffer starts on a 64-element boundary


def _slot(vals, dtype):
    """``vals`` as a 64-element-aligned slice of a larger buffer with live data on both sides."""
    n = vals.numel()
    buf = torch.randn(ALIGN + (n + ALIGN - 1) // ALIGN * ALIGN + ALIGN, device=DEV).to(dtype)
    buf[ALIGN:ALIGN + n] = vals.to(dtype)
    return buf, buf[ALIGN:ALIGN + n]


@pytest.mark.parametrize("pdt,gdt,has_master", ADAMW_DT)
@pytest.mark.parametrize("n", ADAMW_N)
@pytest.mark.parametrize("use_scale", [True, False])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_vector_path(pdt, gdt, has_master, n, use_scale, step, wd):
    assert n % 4 == 0
    first = slice(0, n // 8)                                    # first step: m = v = 0, g != 0
    zero = torch.zeros(n, dtype=torch.bool, device=DEV)         # g = m = v = 0: decay alone
    zero[n // 3:n // 3 + max(1, n // 16)] = True
    zero[n - 1] = True                                          # the ragged end's last lane
    p32 = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    m = torch.randn(n, device=DEV).abs() * 0.1
    v = torch.randn(n, device=DEV).abs() * 0.1
    m[first] = 0
    v[first] = 0
    for t in (g, m, v):
        t[zero] = 0
    bufs = {"param": _slot(p32, pdt), "grad": _slot(g, gdt), "m": _slot(m, F32), "v": _slot(v, F32)}
    if has_master:
        # the master is the fp32 value whose rounding the parameter is
        bufs["master"] = _slot(bufs["param"][1].float(), F32)
    before = {k: b.clone() for k, (b, _) in bufs.items()}
    param, grad, em, ev = (bufs[k][1] for k in ("param", "grad", "m", "v"))
    master = bufs["master"][1] if has_master else None
    scale = torch.tensor([0.7], device=DEV) if use_scale else None
    args = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, step=step)
    # oracle on the CPU, fp32 state.  Without a master the kernel still computes in fp32 from the
    # parameter's value and rounds once, so the oracle updates an fp32 copy of that value.
    r_param = param.cpu().clone() if has_master else _f(param)
    r_master, r_grad, r_m, r_v = _f(master), grad.cpu().clone(), _f(em), _f(ev)
    ref.adamw_step_(r_param, r_master, r_grad, r_m, r_v, grad_scale=None if scale is None else scale.cpu(), **args)
    ops.adamw_step_(param, master, grad, em, ev, grad_scale=scale, **args)
    check_elem(em, r_m, rtol=1e-6, atol=1e-7, name="m")
    check_elem(ev, r_v, rtol=5e-5, atol=1e-9, name="v")
    if has_master:
        check_elem(master, r_master, rtol=1e-6, atol=1e-7, name="master")
    _close(param, r_param, pdt, name="param")
    # g = m = v = 0: the moments stay exactly 0 and the parameter is finite (its value, the decay
    # alone, is part of the oracle comparison above)
    assert (em[zero] == 0).all() and (ev[zero] == 0).all()
    assert torch.isfinite(param.float()[zero]).all()
    if has_master:
        assert torch.isfinite(master[zero]).all()
    # nothing outside the slot is written, and the gradient not at all
    for k, (b, _) in bufs.items():
        assert _same_bits(b[:ALIGN], before[k][:ALIGN]), k
        assert _same_bits(b[ALIGN + n:], before[k][ALIGN + n:]), k
    assert _same_bits(bufs["grad"][0], before["grad"])


# ------------------------------------------------------------------ 3. sq_norm_multi, exact counts
# sqsum_slots(n) = min(ceil(n / 8,192), 1,024) workgroups; n a multiple of the vector -> the
# vector kernel, whose lane with global id t sums vectors t, t + s, t + 2s, t + 3s per unrolled
# pass (s = 256 * slots) while t + 4 s k + 3 s < nvec, then the rest one vector per pass.
def _sq_places(nvec, slots):
    s = 256 * slots
    vecs = {0, nvec - 1}
    # both sides of every lane-stride boundary (the four streams of a pass, the passes themselves)
    for k in range(1, nvec // s + 1):
        vecs.update((k * s - 1, k * s))
    # per lane: the last vector its unrolled loop takes and the first one its remainder loop takes;
    # lanes at both ends of the grid and on either side of each change of the unrolled pass count
    # (lane t makes ceil((nvec - 3 s - t) / 4 s) unrolled passes: the count drops at
    # t = nvec - 3 s - 4 s k) and of the ragged end of the last remainder pass
    passes = lambda t: max(0, -(-(nvec - 3 * s - t) // (4 * s)))          # noqa: E731
    lanes = {0, s - 1}
    for t in [nvec - 3 * s - 4 * s * k for k in range(nvec // (4 * s) + 2)] + [nvec % s]:
        if 1 <= t < s:
            lanes.update((t - 1, t))
    for t in lanes:
        k = passes(t)
        if k > 0:
            vecs.add(t + 4 * s * (k - 1) + 3 * s)
        vecs.add(t + 4 * s * k)
    return sorted(v for v in vecs if 0 <= v < nvec)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("big", [False, True])
def test_sq_norm_multi_exact_count(dt, big):
    """Indicator inputs: the fp32 sum of squares is an exact count, so a dropped or doubled
    vector shows as an inequality."""
    VEC = 16 // ES[dt]
    if big:      # two unrolled passes (bf16; four in fp32) of the capped grid + 7 ragged vectors
        nvec, slots = 2 * 8192 * 1024 // VEC + 7, 1024
    else:        # one workgroup: lanes 0..4 take one unrolled pass, the others the remainder loop only
        nvec, slots = 3 * 256 + 5, 1
    n = nvec * VEC
    assert min(-(-n // 8192), 1024) == slots
    x = torch.zeros(n, device=DEV, dtype=dt)
    vecs = torch.tensor(_sq_places(nvec, slots), device=DEV)
    x.view(nvec, VEC)[vecs] = 1.0                   # whole vectors, the last one included
    x[0] = 1.0
    x[n - 1] = 1.0
    count = int(vecs.numel()) * VEC
    assert ops.sq_norm_multi([x]).item() == count
    # one element per chosen vector, a different position in each
    x.zero_()
    x.view(nvec, VEC)[vecs, vecs % VEC] = 1.0
    assert ops.sq_norm_multi([x]).item() == vecs.numel()
    # next to an odd-length tensor (scalar kernel) in the same call
    y = torch.ones(37, device=DEV)
    assert ops.sq_norm_multi([y, x, y.to(BF16)]).item() == vecs.numel() + 74


@pytest.mark.parametrize("dt", [BF16, F32])
def test_sq_norm_multi_random_vector_path(dt):
    VEC = 16 // ES[dt]
    ts = [torch.randn((3 * 256 + 5) * VEC, device=DEV).to(dt),
          torch.randn((2 * 4 * 256 * 1024 + 7) * VEC, device=DEV).to(dt)]
    sq = ops.sq_norm_multi(ts)
    sq0 = sum(t.double().pow(2).sum().item() for t in ts)
    assert math.isclose(sq.item(), sq0, rel_tol=1e-4)


# ------------------------------------------------------------------ 4. dropout bits at training offsets
# reserve_offsets (models/base.py) hands out multiples of 256: the elementwise kernels take the
# even branch of drop_bits_run (one hash per element pair); past 2^33 the pair index has a
# non-zero high word (drop_seed_mix, DropSlab's second window).
P_DROP, SEED = 0.1, 4321


def _drop_offsets(numel):
    assert numel > 1024
    straddle = ((1 << 33) - numel // 2) // 256 * 256     # 2^33 falls inside the tensor
    assert straddle < (1 << 33) < straddle + numel
    return {"even": 256 * 1000, "high": (1 << 33) + 256 * 12345, "straddle": straddle}


OFFSET_KINDS = ["even", "high", "straddle"]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", OFFSET_KINDS)
def test_dropout_elementwise_offsets(dt, kind):
    N, d = 53, 768
    off = _drop_offsets(N * d)[kind]
    assert off % 256 == 0
    keep = ref.drop_keep_mask(SEED, off, N * d, P_DROP).view(N, d)
    x = torch.randn(N, d, device=DEV).to(dt)
    a = torch.randn(N, d, device=DEV).to(dt)
    ones, zeros = torch.ones_like(a), torch.zeros_like(a)
    # dropout_add
    _close(ops.dropout_add(x, a, P_DROP, SEED, off), ref.dropout_add(_f(x), _f(a), P_DROP, SEED, off), dt,
           name="dropout_add")
    assert torch.equal((ops.dropout_add(zeros, ones, P_DROP, SEED, off) != 0).cpu(), keep)
    # dropout_bwd
    want = ref.dropout_bwd(_f(a), P_DROP, SEED, off)
    _close(ops.dropout_bwd(a, P_DROP, SEED, off), want, dt, name="dropout_bwd")
    assert torch.equal((ops.dropout_bwd(ones, P_DROP, SEED, off) != 0).cpu(), keep)
    # dropout_bwd_bias: the same output, and db (+)= its column sums
    for accumulate in (False, True):
        db = torch.randn(d, device=DEV).to(dt)
        db0 = want.sum(0) + (_f(db) if accumulate else 0)
        out = ops.dropout_bwd_bias(a, P_DROP, SEED, off, db, accumulate)
        _close(out, want, dt, name="dropout_bwd_bias")
        _close(db, db0, dt, 4, name=f"dropout_bwd_bias db acc={accumulate}")
    db = torch.zeros(d, device=DEV, dtype=dt)
    assert torch.equal((ops.dropout_bwd_bias(ones, P_DROP, SEED, off, db) != 0).cpu(), keep)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", OFFSET_KINDS)
def test_dropout_add_layernorm_offsets(dt, kind):
    N, d = 53, 768
    off = _drop_offsets(N * d)[kind]
    keep = ref.drop_keep_mask(SEED, off, N * d, P_DROP).view(N, d)
    x = (torch.randn(N, d, device=DEV) + 0.5).to(dt)
    a = torch.randn(N, d, device=DEV).to(dt)
    w = (1 + 0.1 * torch.randn(d, device=DEV)).to(dt)
    b = (0.1 * torch.randn(d, device=DEV)).to(dt)
    x2, y, m, r = ops.dropout_add_layernorm(x, a, w, b, 1e-5, P_DROP, SEED, off)
    x20 = ref.dropout_add(_f(x), _f(a), P_DROP, SEED, off)
    y0, m0, r0 = ref.layernorm_fwd(x20, _f(w), _f(b), 1e-5)
    _close(x2, x20, dt, name="x2")
    _close(y, y0, dt, 2, name="y")
    mask = ops.dropout_add_layernorm(torch.zeros_like(a), torch.ones_like(a), w, b, 1e-5, P_DROP, SEED, off)[0]
    assert torch.equal((mask != 0).cpu(), keep)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pos", [False, True])
@pytest.mark.parametrize("kind", OFFSET_KINDS)
def test_embedding_fwd_dropout_offsets(dt, pos, kind):
    V, d, B, T = 300, 96, 3, 20
    off = _drop_offsets(B * T * d)[kind]
    keep = ref.drop_keep_mask(SEED, off, B * T * d, P_DROP).view(B * T, d)
    wte = torch.randn(V, d, device=DEV).to(dt)
    wpe = torch.randn(T, d, device=DEV).to(dt) if pos else None
    idx = torch.randint(0, 40, (B * T,), device=DEV)
    x = ops.embedding_fwd(idx, wte, wpe, T, P_DROP, SEED, off)
    x0 = ref.embedding_fwd(idx.cpu(), _f(wte), _f(wpe), T, P_DROP, SEED, off)
    _close(x, x0, dt, name="emb fwd dropout")
    # tables of ones: the output is non-zero exactly where the element is kept
    mask = ops.embedding_fwd(idx, torch.ones_like(wte), None if wpe is None else torch.ones_like(wpe), T,
                             P_DROP, SEED, off)
    assert torch.equal((mask != 0).cpu(), keep)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,G,hd", [(2, 4, 4, 64), (1, 8, 2, 128)])
@pytest.mark.parametrize("T", [200, 256])
@pytest.mark.parametrize("kind", OFFSET_KINDS)
def test_flash_attention_dropout_offsets(dt, B, H, G, hd, T, kind):
    """Attention dropout at an even offset, above 2^33, and with 2^33 inside the (batch, head)
    slab of a middle head: slabs wholly below, across and wholly above the boundary."""
    p, seed, causal = 0.1, 99, True
    slab, mid = T * T, (B * H) // 2
    off = {"even": 256 * 1000, "high": (1 << 33) + 256 * 12345,
           "straddle": ((1 << 33) - mid * slab - slab // 2) // 256 * 256}[kind]
    if kind == "straddle":
        assert 0 < mid < B * H - 1 and off + mid * slab < (1 << 33) < off + (mid + 1) * slab
    qkv = torch.randn(B * T, (H + 2 * G) * hd, device=DEV).to(dt)
    do = torch.randn(B * T, H * hd, device=DEV).to(dt)
    km = ops.attn_keep_mask(qkv, B, T, H, hd, p)
    assert (km is None) == (dt == F32)
    o, lse = ops.flash_attn_fwd(qkv, B, T, H, G, hd, causal, p, seed, off, keep_mask=km)
    o0, lse0 = ref.flash_attn_fwd(_f(qkv), B, T, H, G, hd, causal, p, seed, off)
    _close(o, o0, dt, 2, name="o")
    check_elem(lse, lse0, **LSE_TOL, name="lse")
    dqkv0 = ref.flash_attn_bwd(_f(qkv), o0, lse0, _f(do), B, T, H, G, hd, causal, p, seed, off)
    dqkv = ops.flash_attn_bwd(qkv, o, lse, do, B, T, H, G, hd, causal, p, seed, off)      # re-hashes
    _close(dqkv, dqkv0, dt, 4, name="dqkv")
    if km is not None:
        KW = (T + 31) // 32
        bits = (km.view(B * H, KW, T).permute(0, 2, 1).unsqueeze(-1).to(torch.int64)
                >> torch.arange(32, device=DEV)) & 1                        # [BH, T(q), KW, 32]
        got = bits.reshape(B * H, T, KW * 32)[:, :, :T].bool().cpu()
        want = ref.drop_keep_mask(seed, off, B * H * T * T, p).view(B * H, T, T)
        cover = torch.ones(T, T, dtype=torch.bool).tril()
        assert torch.equal(got[:, cover], want[:, cover])
        dqkv_m = ops.flash_attn_bwd(qkv, o, lse, do, B, T, H, G, hd, causal, p, seed, off, keep_mask=km)
        _close(dqkv_m, dqkv0, dt, 4, name="dqkv (keep mask)")


# ------------------------------------------------------------------ 5. second pass of capped grids
# ew_grid caps at 2,048 workgroups = 524,288 work items; every case below has more.
@pytest.mark.parametrize("dt", DTYPES)
def test_rope_second_grid_pass(dt):
    """16-bit: rope_k, one item per 8 rotation pairs, 6,600 rows x (8 + 2) heads x 8 = 528,000
    items; fp32: rope_scalar_k, one item per pair, 4,224,000 items."""
    B, T, H, G, hd, po = 6, 1100, 8, 2, 128, 7
    N = B * T
    assert N * (H + G) * (hd // 16) > 2048 * 256
    cos, sin = ops.rope_tables(hd, T + po, 500000.0, None, device=DEV)
    qkv = torch.randn(N, (H + 2 * G) * hd, device=DEV).to(dt)
    q0 = ref.rope_(_f(qkv).clone(), cos.cpu(), sin.cpu(), T, H, G, hd, pos_offset=po)
    q1 = ops.rope_(qkv.clone(), cos, sin, T, H, G, hd, pos_offset=po)
    _close(q1, q0, dt, name="rope")
    v0 = (H + G) * hd
    assert _same_bits(q1[:, v0:], qkv[:, v0:])                      # v heads untouched
    back0 = ref.rope_(_f(q1).clone(), cos.cpu(), sin.cpu(), T, H, G, hd, inverse=True, pos_offset=po)
    back = ops.rope_(q1.clone(), cos, sin, T, H, G, hd, inverse=True, pos_offset=po)
    _close(back, back0, dt, name="rope inverse")
    _close(back, _f(qkv), dt, 2, name="rope round trip")
    assert _same_bits(back[:, v0:], qkv[:, v0:])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_dev_positions(dt, hd):
    """rope_dev_ reads the position from device memory: equal to rope_ at T = 1 and that offset."""
    H, G, ctx = 4, 2, 300
    cos, sin = ops.rope_tables(hd, ctx, 500000.0, None, device=DEV)
    pos_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pos in (0, 1, 255, ctx - 1):
        qkv = torch.randn(3, (H + 2 * G) * hd, device=DEV).to(dt)
        want = ref.rope_(_f(qkv).clone(), cos.cpu(), sin.cpu(), 1, H, G, hd, pos_offset=pos)
        pos_t.fill_(pos)
        got = ops.rope_dev_(qkv.clone(), cos, sin, H, G, hd, pos_t)
        _close(got, want, dt, name=f"rope_dev pos={pos}")
        assert _same_bits(got[:, (H + G) * hd:], qkv[:, (H + G) * hd:])
        if pos == 0:
            assert _same_bits(got, qkv)                            # cos 1, sin 0: the identity


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,F", [(4200, 1000), (52500, 10)])
def test_swiglu_second_grid_pass(dt, N, F):
    """F = 1,000: fewer than 512 vectors per row -> the grid-stride vector kernels, 4,200 x 125
    items (16-bit); F = 10: not a whole vector -> the scalar instantiation, 525,000 items."""
    VEC = 16 // ES[dt] if F % (16 // ES[dt]) == 0 else 1
    assert F // VEC < 512 and N * F // VEC > 2048 * 256
    gu = torch.randn(N, 2 * F, device=DEV).to(dt)
    da = torch.randn(N, F, device=DEV).to(dt)
    act0 = ref.swiglu_fwd(_f(gu))
    dgu0 = ref.swiglu_bwd(_f(gu), _f(da))
    _close(ops.swiglu_fwd(gu), act0, dt, name="swiglu")
    _close(ops.swiglu_bwd(gu, da), dgu0, dt, 2, name="swiglu_bwd")
    da2 = da.clone()
    dgu2 = ops.swiglu_bwd_act(gu, da2)
    _close(dgu2, dgu0, dt, 2, name="swiglu_bwd_act dgu")
    _close(da2, act0, dt, name="swiglu_bwd_act act")


# ------------------------------------------------------------------ 6. decode kernels
def _nan_rows(c, start):
    c[:, :, start:] = float("nan")


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("B,H,G,hd,L,Tmax", [(2, 8, 2, 128, 255, 512), (2, 8, 2, 128, 256, 512),
                                             (2, 8, 2, 128, 257, 512), (2, 8, 2, 128, 512, 512),
                                             (1, 4, 1, 128, 8192, 8192)])
def test_attn_decode_stride_edges(dt, B, H, G, hd, L, Tmax):
    """Lengths around one 256-thread key stride, the full cache, and the largest cache (the whole
    LDS score buffer); rows at and beyond L hold NaN and must not be read."""
    q = torch.randn(B, H, hd, device=DEV).to(dt)
    kc = torch.randn(B, G, Tmax, hd, device=DEV).to(dt)
    vc = torch.randn(B, G, Tmax, hd, device=DEV).to(dt)
    _nan_rows(kc, L)
    _nan_rows(vc, L)
    o = ops.attn_decode(q, kc, vc, L)
    assert torch.isfinite(o.float()).all()
    o0 = ref.attn_decode(_f(q), _f(kc), _f(vc), L)
    _close(o, o0, dt, 2, name="decode")


def _append_step(run, qkv, kc, vc, kbase, vbase, pos_t, pos, H, G, dt):
    """One attn_decode_append at ``pos``: cache rows >= pos hold NaN before the call; afterwards
    row pos is the qkv row's k / v bit for bit, every other row is untouched, and the output is
    the oracle's over the updated cache."""
    B, _, Tmax, hd = kc.shape
    kc.copy_(kbase)
    vc.copy_(vbase)
    _nan_rows(kc, pos)
    _nan_rows(vc, pos)
    kb, vb = kc.clone(), vc.clone()
    pos_t.fill_(pos)
    out = run()
    torch.cuda.synchronize()
    v = qkv.view(B, H + 2 * G, hd)
    assert _same_bits(kc[:, :, pos], v[:, H:H + G]), pos
    assert _same_bits(vc[:, :, pos], v[:, H + G:]), pos
    other = torch.ones(Tmax, dtype=torch.bool, device=kc.device)
    other[pos] = False
    assert _same_bits(kc[:, :, other], kb[:, :, other]), pos
    assert _same_bits(vc[:, :, other], vb[:, :, other]), pos
    o0 = ref.attn_decode(_f(v[:, :H]), _f(kc), _f(vc), pos + 1)
    _close(out, o0, dt, 2, name=f"decode append pos={pos}")


APPEND_SHAPES = [(2, 8, 2, 128, 512), (3, 4, 4, 64, 300), (1, 4, 1, 128, 8192)]


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("B,H,G,hd,Tmax", APPEND_SHAPES)
def test_attn_decode_append(dt, B, H, G, hd, Tmax):
    kbase = torch.randn(B, G, Tmax, hd, device=DEV).to(dt)
    vbase = torch.randn(B, G, Tmax, hd, device=DEV).to(dt)
    kc, vc = kbase.clone(), vbase.clone()
    pos_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pos in (0, 1, 255, 256, 257, Tmax - 1):
        qkv = torch.randn(B, (H + 2 * G) * hd, device=DEV).to(dt)
        _append_step(lambda: ops.attn_decode_append(qkv, kc, vc, pos_t, H, G), qkv, kc, vc, kbase, vbase,
                     pos_t, pos, H, G, dt)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_attn_decode_append_graph_replay(dt):
    """Captured once, replayed at three positions by writing the position tensor (and new qkv
    rows into the captured input), as train/generate.py's DecodeGraph does."""
    B, H, G, hd, Tmax = 2, 8, 2, 128, 512
    kbase = torch.randn(B, G, Tmax, hd, device=DEV).to(dt)
    vbase = torch.randn(B, G, Tmax, hd, device=DEV).to(dt)
    kc, vc = kbase.clone(), vbase.clone()
    qkv = torch.randn(B, (H + 2 * G) * hd, device=DEV).to(dt)
    pos_t = torch.full((1,), Tmax - 1, dtype=torch.int32, device=DEV)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):                       # warm-up outside the capture
        ops.attn_decode_append(qkv, kc, vc, pos_t, H, G)
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_decode_append(qkv, kc, vc, pos_t, H, G)

    def replay():
        graph.replay()
        return out

    for pos in (1, 256, Tmax - 1):
        qkv.copy_(torch.randn(B, (H + 2 * G) * hd, device=DEV).to(dt))
        _append_step(replay, qkv, kc, vc, kbase, vbase, pos_t, pos, H, G, dt)


# ------------------------------------------------------------------ 7. cross-entropy, padded rows
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("V,ld", [(50257, 50304), (97, 104), (128256, 128320)])
def test_cross_entropy_padded_rows(dt, V, ld):
    """logits = buf[:, :V] of an [N, ld] buffer (the vocabulary padded to whole GEMM tiles): the
    row stride is ld, and the pad columns -- a large finite sentinel that would wreck the
    log-sum-exp if read -- come back bit-identical."""
    N, sentinel = 24, 3.0e4
    scale = torch.tensor([0.5], device=DEV)
    for mode in ("default", "all ignored", "ignore_index 5"):
        buf = torch.full((N, ld), sentinel, device=DEV, dtype=dt)
        buf[:, :V] = (3 * torch.randn(N, V, device=DEV)).to(dt)
        logits = buf[:, :V]
        assert logits.stride(0) == ld and not logits.is_contiguous()
        before = buf.clone()
        tgt = torch.randint(0, V, (N,), device=DEV)
        tgt[0] = 0              # first column
        tgt[1] = V - 1          # last column: the scalar tail after the last whole vector
        ignore = -100
        if mode == "default":
            tgt[3] = -100
        elif mode == "all ignored":
            tgt[:] = -100
        else:
            ignore = 5
            tgt[tgt == 5] = 6
            tgt[3] = 5
            tgt[7] = 5
        dense = _f(logits).contiguous()
        l, lse = ops.ce_fwd(logits, tgt, ignore)
        assert _same_bits(buf, before)                  # the forward writes nothing
        l0, lse0 = ref.ce_fwd(dense, tgt.cpu(), ignore)
        check_elem(l, l0, **LSE_TOL, name=f"loss ({mode})")
        check_elem(lse, lse0, **LSE_TOL, name=f"lse ({mode})")
        if mode == "all ignored":
            assert (l == 0).all()
        ops.ce_bwd_(logits, tgt, lse, scale, ignore)
        g0 = ref.ce_bwd_(dense.clone(), tgt.cpu(), lse0, scale.cpu(), ignore)
        _close(logits, g0, dt, 2, name=f"dlogits ({mode})")
        assert _same_bits(buf[:, V:], before[:, V:]), mode
