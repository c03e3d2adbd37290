"""csrc/binding.cpp holds every ``torch.ops.bllm`` op to one contract: before a launch, each pointer
the launcher receives covers what the kernel reads and writes through it, in the dtype the kernel
assumes.  For every op with tensor arguments: one accepted call with the smallest valid arguments
(the fixture is valid; compared with the ``ops.reference`` oracle where there is one, with the
tolerance class of the neighbouring kernel tests), then one refused call per check, each with
exactly one argument changed, expecting a ``RuntimeError`` that names the op.

Every changed argument errs in the safe direction -- a buffer longer than required, a dtype with a
larger element, a strided or misaligned view into a larger allocation, an extra dimension -- so
the call would stay inside its allocations even if the check were missing and the kernel ran.
Closed by reading csrc/binding.cpp instead, because the mutated call could read or write out of
bounds without its check: buffers shorter or dtypes narrower than expected, negative window
offsets (c0 / ocol / toff / pa / qb / pos_offset), T <= 0, one RoPE table without the other, and a
tensor on a second GPU (needs two devices).  The ops are called directly: ops/__init__.py pre-filters."""
import re

import pytest
import torch
from numerics import check_close, check_elem

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = torch.bfloat16
K_OF = {1: 2.0, 2: 3.0, 4: 5.0}            # allowance per kernel class (tests/test_kernels_gpu.py)
LSE_TOL = dict(rtol=1e-5, atol=2e-5)
N, D, V, T, H, G, HD, R = 8, 64, 64, 8, 1, 1, 64, 16
QKV = (H + 2 * G) * HD


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


def rnd(*shape, dt=DT):
    return torch.randn(*shape, device=DEV).to(dt)


def f32(t):
    return t.detach().cpu().float()


def _close(a, b, scale=1, name=""):
    check_close(a, b, a.dtype, k=K_OF[scale], name=name)


def call(name, args):
    return getattr(torch.ops.bllm, name)(*args)


def refused(name, args, i, bad):
    """Why the call with argument i replaced was NOT refused on the host by a message that names the op."""
    a = list(args)
    a[i] = bad
    try:
        call(name, a)
    except RuntimeError as e:
        return None if name in str(e) else f"{name} argument {i}: the message lacks the op name: {e}"
    return f"{name} argument {i}: accepted"


def refusals(name, args, cases):
    """Every (argument index, replacement) of ``cases`` is refused; one report for all that are not."""
    missed = [m for m in (refused(name, args, i, bad) for i, bad in cases) if m]
    assert not missed, "\n".join(missed)


# ---- mutations, all in the safe direction
WIDER = {torch.bfloat16: torch.float32, torch.float32: torch.float64, torch.int32: torch.int64}


def wider(t):
    """The same values in a dtype with a larger element."""
    return t.to(WIDER[t.dtype])


def longer(t):
    """One extra element (1-D) or one extra row."""
    return torch.cat([t, t[:1]])


def strided(t):
    """The same values with element stride 2 in the last dim, inside a twice larger allocation."""
    buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    v = buf[..., ::2]
    v.copy_(t)
    return v


def misaligned(t):
    """The same values, contiguous, one element past a 16-B boundary inside a larger allocation."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def extra_dim(t):
    return t.unsqueeze(0)


# ------------------------------------------------------------------ norms
def test_rmsnorm():
    x, w, dy = rnd(N, D), rnd(D), rnd(N, D)
    y, rstd = call("rmsnorm_fwd", (x, w, 1e-5))
    y0, r0 = ref.rmsnorm_fwd(f32(x), f32(w), 1e-5)
    _close(y, y0, name="y")
    check_elem(rstd, r0, rtol=2e-5, atol=0, name="rstd")
    refusals("rmsnorm_fwd", (x, w, 1e-5), ((0, strided(x)), (0, extra_dim(x)), (1, wider(w)), (1, longer(w))))

    buf = torch.zeros(N, D + 16, dtype=DT, device=DEV)
    args = (x, w, 1e-5, buf[:, :D])
    assert torch.equal(call("rmsnorm_fwd_into_", args), rstd) and torch.equal(buf[:, :D], y)
    refusals("rmsnorm_fwd_into_", args, ((1, wider(w)), (3, misaligned(y)), (3, wider(y)), (3, longer(y)),
             (3, strided(y))))

    acc, out = rnd(N, D), torch.zeros(D, device=DEV)
    args = (dy, x, w, rstd, acc, out, False)
    dx, dw = call("rmsnorm_bwd", args)
    dx0, dw0 = ref.rmsnorm_bwd(f32(dy), f32(x), f32(w), r0, f32(acc))
    _close(dx, dx0, 2, name="dx")
    check_close(dw, dw0, DT, k=K_OF[2], name="dw")
    refusals("rmsnorm_bwd", args, ((0, strided(dy)), (0, wider(dy)), (2, wider(w)), (3, longer(rstd)), (3, wider(rstd)),
                   (4, wider(acc)), (4, longer(acc)), (5, longer(out))))


def test_layernorm():
    x, w, b, dy = rnd(N, D), rnd(D), rnd(D), rnd(N, D)
    y, mean, rstd = call("layernorm_fwd", (x, w, b, 1e-5))
    y0, m0, r0 = ref.layernorm_fwd(f32(x), f32(w), f32(b), 1e-5)
    _close(y, y0, name="y")
    refusals("layernorm_fwd", (x, w, b, 1e-5), ((0, strided(x)), (1, wider(w)), (2, wider(b)), (2, longer(b))))

    args = (dy, x, w, mean, rstd, None, None, None, False)
    dx, dw, db = call("layernorm_bwd", args)
    dx0, dw0, db0 = ref.layernorm_bwd(f32(dy), f32(x), f32(w), m0, r0, None)
    _close(dx, dx0, 2, name="dx")
    check_close(dw, dw0, DT, k=K_OF[2], name="dw")
    check_close(db, db0, DT, k=K_OF[2], name="db")
    refusals("layernorm_bwd", args, ((0, wider(dy)), (2, wider(w)), (3, longer(mean)), (3, strided(mean)),
             (3, wider(mean)),
                   (4, longer(rstd)), (4, wider(rstd)), (5, wider(x)), (6, torch.zeros(D, device=DEV))))

    a = rnd(N, D)
    args = (x, a, w, b, 1e-5, 0.0, 1, 2)
    x2, y2, m2, r2 = call("dropout_add_layernorm", args)
    _close(x2, f32(x) + f32(a), name="x2")
    _close(y2, ref.layernorm_fwd(f32(x2), f32(w), f32(b), 1e-5)[0], 2, name="y")
    refusals("dropout_add_layernorm", args, ((1, strided(a)), (1, wider(a)), (2, wider(w)), (3, longer(b))))


# ------------------------------------------------------------------ elementwise
def test_dropout_gelu_transpose():
    x, a = rnd(N, D), rnd(N, D)
    _close(call("dropout_add", (x, a, 0.0, 1, 2)), f32(x) + f32(a), name="dropout_add")
    refusals("dropout_add", (x, a, 0.0, 1, 2), ((0, strided(x)), (1, wider(a)), (1, longer(a))))
    _close(call("dropout_bwd", (x, 0.0, 1, 2)), f32(x), name="dropout_bwd p = 0")
    refusals("dropout_bwd", (x, 0.0, 1, 2), [(0, strided(x))])

    _close(call("gelu_fwd", (x,)), ref.gelu_fwd(f32(x)), name="gelu")
    refusals("gelu_fwd", (x,), [(0, strided(x))])
    _close(call("gelu_bwd", (x, a)), ref.gelu_bwd(f32(x), f32(a)), name="gelu_bwd")
    refusals("gelu_bwd", (x, a), ((1, wider(a)), (1, longer(a)), (1, strided(a))))

    assert torch.equal(call("transpose2d", (x,)), x.t().contiguous())
    refusals("transpose2d", (x,), [(0, bad) for bad in (strided(x), wider(x), extra_dim(x))])


def test_bias_grads_and_partials():
    dy, f = rnd(N, D), rnd(N, D)
    db = torch.zeros(D, device=DEV)
    call("bias_grad_", (dy, db, False))
    check_close(db, f32(dy).sum(0), DT, k=K_OF[4], name="bias_grad")
    refusals("bias_grad_", (dy, db, False), ((0, strided(dy)), (0, extra_dim(dy)), (1, longer(db)),
             (1, extra_dim(db)), (1, strided(db))))

    args = (dy.clone(), f, db, False, 1, 0.0, 0, 0, False)
    out = call("bwd_bias_grad_", args)
    assert torch.equal(out, call("gelu_bwd", (f, dy)))
    refusals("bwd_bias_grad_", args, ((0, strided(dy)), (1, wider(f)), (1, longer(f)), (2, longer(db)),
             (2, extra_dim(db)), (4, 2)))
    refusals("bwd_bias_grad_", (dy.clone(), None, db, False, 0, 0.1, 0, 0, False), [(8, True)])   # act only with GELU

    part, out = rnd(2, D, dt=torch.float32), torch.zeros(D, dtype=DT, device=DEV)
    call("sum_partials_", (part, out, False))
    _close(out, f32(part).sum(0), name="sum_partials")
    refusals("sum_partials_", (part, out, False), ((0, rnd(2, D + 8, dt=torch.float32)), (0, strided(part)),
             (1, strided(out))))


def test_swiglu():
    F = D
    gu, da = rnd(N, 2 * F), rnd(N, F)
    act = call("swiglu_fwd", (gu,))
    _close(act, ref.swiglu_fwd(f32(gu)), name="swiglu")
    refusals("swiglu_fwd", (gu,), [(0, bad) for bad in (strided(gu), extra_dim(gu))])

    buf = torch.zeros(N, F + 16, dtype=DT, device=DEV)
    call("swiglu_fwd_into_", (gu, buf[:, :F]))
    assert torch.equal(buf[:, :F], act)
    refusals("swiglu_fwd_into_", (gu, buf[:, :F]), [(1, bad) for bad in (misaligned(act), wider(act), longer(act),
             strided(act))])

    dgu = call("swiglu_bwd", (gu, da))
    _close(dgu, ref.swiglu_bwd(f32(gu), f32(da)), 2, name="swiglu_bwd")
    da2 = da.clone()
    assert torch.equal(call("swiglu_bwd_act", (gu, da2)), dgu) and torch.equal(da2, act)
    for name in ("swiglu_bwd", "swiglu_bwd_act"):
        refusals(name, (gu, da.clone()), ((0, rnd(N, 2 * F + 1)), (0, extra_dim(gu)), (1, extra_dim(da)),
                 (1, wider(da)), (1, longer(da)),
                       (1, strided(da))))


def test_swiglu_lowrank():
    F = D
    gu, base, u, P = rnd(N, 2 * F), rnd(N, F), rnd(N, R), rnd(R, F)
    args = (gu, base, u, P, 0.5)
    dgu = call("swiglu_bwd_lowrank", args)
    _close(dgu, ref.swiglu_bwd(f32(gu), f32(base) + 0.5 * f32(u) @ f32(P)), 2, name="swiglu_bwd_lowrank")
    refusals("swiglu_bwd_lowrank", args, ((0, strided(gu)), (1, misaligned(base)), (1, wider(base)), (2, wider(u)),
             (2, strided(u)),
                   (3, wider(P)), (3, rnd(2 * R, F)), (3, extra_dim(P))))

    st = rnd(N, 2 * R)
    gs = [torch.zeros(R, F, device=DEV) for _ in range(3)]
    args = (gu, base, u, P, 0.5, st, *gs, False)
    assert call("swiglu_bwd_lowrank_wgrad", args).shape == gu.shape and gs[0].dtype == torch.float32
    check_close(gs[0], f32(st)[:, :R].t() @ f32(dgu)[:, :F], DT, k=K_OF[4], name="gB_gate")
    refusals("swiglu_bwd_lowrank_wgrad", args, ((1, misaligned(base)), (2, strided(u)), (3, wider(P)),
             (5, misaligned(st)), (5, wider(st)),
                   (7, torch.zeros(R, F, dtype=torch.float64, device=DEV)), (8, extra_dim(gs[2])), (8, longer(gs[2]))))


# ------------------------------------------------------------------ RoPE
def test_rope():
    cos, sin = ops.rope_tables(HD, T, 10000.0, device=DEV)
    qkv = rnd(N, QKV)
    args = (qkv.clone(), cos, sin, T, H, G, HD, False, 0)
    call("rope_", args)
    _close(args[0], ref.rope_(f32(qkv), cos.cpu(), sin.cpu(), T, H, G, HD), name="rope")
    refusals("rope_", args, ((0, strided(qkv)), (0, extra_dim(qkv)), (1, wider(cos)), (1, extra_dim(cos)),
             (2, longer(sin)),
                   (2, wider(sin))))

    pos = torch.tensor([3], dtype=torch.int32, device=DEV)
    q1 = qkv[:1].clone()
    args = (q1, cos, sin, H, G, HD, pos)
    call("rope_dev_", args)
    _close(q1, ref.rope_(f32(qkv[:1]), cos.cpu(), sin.cpu(), 1, H, G, HD, False, 3), name="rope_dev")
    refusals("rope_dev_", args, ((1, wider(cos)), (2, longer(sin)), (6, longer(pos)), (6, wider(pos))))

    ids = torch.arange(N, dtype=torch.int32, device=DEV)
    args = (qkv.clone(), cos, sin, ids, H, G, HD, False)
    call("rope_pos_", args)
    _close(args[0], ref.rope_pos_(f32(qkv), cos.cpu(), sin.cpu(), ids.cpu(), H, G, HD), name="rope_pos")
    refusals("rope_pos_", args, ((1, extra_dim(cos)), (2, longer(sin)), (3, longer(ids)), (3, wider(ids)),
             (3, strided(ids))))


# ------------------------------------------------------------------ GEMM: the smallest supported tile
def _gemm_refusals(name, args, extra=()):
    a, b, c = args[:3]
    refusals(name, args, ((0, misaligned(a)), (0, strided(a)), (1, wider(b)), (1, longer(b)), (1, misaligned(b)),
                   (2, strided(c)), (2, extra_dim(c)), (2, longer(c))) + tuple(extra))


def test_gemms():
    M, Nn, K = 256, 256, 128
    a, b, c = rnd(K, M), rnd(K, Nn), torch.zeros(M, Nn, device=DEV)
    call("wgrad_gemm_", (a, b, c, False, 1))
    check_close(c, f32(a).t() @ f32(b), torch.float32, k=3.0, name="wgrad")
    _gemm_refusals("wgrad_gemm_", (a, b, c, False, 1), ((4, 0),))          # splits 0: no such plan

    a2, b2 = rnd(2 * K, M), rnd(2 * K, Nn)
    call("wgrad_gemm_tail_", (a2, b2, c, False, 0, 2))
    check_close(c, f32(a2).t() @ f32(b2), torch.float32, k=3.0, name="wgrad tail")
    _gemm_refusals("wgrad_gemm_tail_", (a2, b2, c, False, 0, 2), ((2, misaligned(c)), (5, 1)))

    an = rnd(M, K)
    call("gemm_nn_", (an, b, c, False))
    check_close(c, f32(an) @ f32(b), torch.float32, k=3.0, name="gemm_nn")
    _gemm_refusals("gemm_nn_", (an, b, c, False), ((2, c.double()),))

    bt = rnd(Nn, K)
    call("gemm_nt_", (an, bt, c, False))
    check_close(c, f32(an) @ f32(bt).t(), torch.float32, k=3.0, name="gemm_nt")
    _gemm_refusals("gemm_nt_", (an, bt, c, False), ((2, c.double()),))

    F = Nn // 2
    gu, act = torch.zeros(M, Nn, dtype=DT, device=DEV), torch.zeros(M, F, dtype=DT, device=DEV)
    call("gemm_nt_swiglu_", (an, bt, gu, act))
    check_close(gu, f32(an) @ f32(bt).t(), DT, k=3.0, name="gemm_nt_swiglu gu")
    assert torch.equal(act, call("swiglu_fwd", (gu,)))
    _gemm_refusals("gemm_nt_swiglu_", (an, bt, gu, act),
                   ((2, misaligned(gu)), (2, wider(gu)), (3, wider(act)), (3, strided(act)), (3, longer(act))))

    cos, sin = ops.rope_tables(128, T, 10000.0, device=DEV)
    qkv = torch.zeros(M, Nn, dtype=DT, device=DEV)
    args = (an, bt, qkv, cos, sin, T, 128, 128)
    call("gemm_nt_rope_", args)
    sep = (f32(an) @ f32(bt).t()).to(DT)
    want = ref.rope_(sep.float()[:, :128].contiguous(), cos.cpu(), sin.cpu(), T, 1, 0, 128)
    check_close(qkv[:, :128], want, DT, k=4.0, name="gemm_nt_rope")
    _gemm_refusals("gemm_nt_rope_", args, ((2, wider(qkv)), (3, wider(cos)), (3, extra_dim(cos)), (4, longer(sin)),
                                           (7, 64)))                    # head dim 64: no such kernel

    bias, f, g = rnd(Nn), torch.zeros(M, Nn, dtype=DT, device=DEV), torch.zeros(M, Nn, dtype=DT, device=DEV)
    call("gemm_nt_bias_gelu_", (an, bt, bias, f, g))
    check_close(f, f32(an) @ f32(bt).t() + f32(bias), DT, k=3.0, name="gemm_nt_bias_gelu f")
    assert torch.equal(g, call("gelu_fwd", (f,)))
    refusals("gemm_nt_bias_gelu_", (an, bt, bias, f, g), ((0, misaligned(an)), (1, wider(bt)), (2, wider(bias)),
             (2, longer(bias)), (2, strided(bias)),
                   (3, wider(f)), (3, strided(f)), (4, wider(g)), (4, longer(g))))

    x, W, C = rnd(N, D), rnd(D, D) / 8, rnd(N, D)
    _close(call("linear_residual", (x, W, C)), f32(C) + f32(x) @ f32(W).t(), 2, name="linear_residual")
    refusals("linear_residual", (x, W, C), ((0, strided(x)), (1, wider(W)), (1, longer(W).t()), (2, longer(C)),
             (2, wider(C))))


def test_gemm_operand_pitch_bound():
    """Row pitches 8 elements above ``kMaxGemmPitch`` (csrc/binding.cpp: the largest pitch whose
    32-bit per-lane staging offsets are exact) are refused for either operand of every layout; a
    refused call launches nothing, so the wide allocations stay uninitialised.  The accepted side,
    8 elements below the bound, is tests/test_large_extent_gpu.py."""
    from large_extent_shapes import GEMM_MAX_PITCH, GEMM_NT_PITCH_LIMIT, GIB
    if torch.cuda.mem_get_info()[0] < 10 * GIB:
        pytest.skip("needs 8 GiB of free device memory (+ 2 GiB)")
    M, Nn, K = 256, 256, 128
    over = GEMM_MAX_PITCH + 8
    wide_k = torch.empty(K, over, dtype=DT, device=DEV)[:, :256]      # [128, 256] rows ``over`` apart: TN a / b, NN b
    a, b, c = rnd(K, M), rnd(K, Nn), torch.zeros(M, Nn, device=DEV)
    refusals("wgrad_gemm_", (a, b, c, False, 1), ((0, wide_k), (1, wide_k)))
    a2, b2 = rnd(2 * K, M), rnd(2 * K, Nn)
    wide_2k = torch.empty(2 * K, over, dtype=DT, device=DEV)[:, :256]
    refusals("wgrad_gemm_tail_", (a2, b2, c, False, 0, 2), ((0, wide_2k), (1, wide_2k)))
    del wide_2k
    torch.cuda.empty_cache()
    an, bt = rnd(M, K), rnd(Nn, K)
    wide_m = torch.empty(M, over, dtype=DT, device=DEV)[:, :K]        # [256, 128] rows ``over`` apart: NN / NT a, NT b
    refusals("gemm_nn_", (an, b, c, False), ((0, wide_m), (1, wide_k)))
    refusals("gemm_nt_", (an, bt, c, False), ((0, wide_m), (1, wide_m)))
    assert wide_k.stride(0) == wide_m.stride(0) == over
    assert "too large" in _message("gemm_nn_", (wide_m, b, c, False))      # refused by the pitch check itself
    assert "too large" in _message("wgrad_gemm_", (a, wide_k, c, False, 1))
    # the planners of ops/__init__.py agree with the binding
    assert ops.wgrad_gemm_ok(a, b, c) and not ops.wgrad_gemm_ok(wide_k, b, c) and not ops.wgrad_gemm_ok(a, wide_k, c)
    assert ops.gemm_nn_ok(an, b, c) and not ops.gemm_nn_ok(wide_m, b, c) and not ops.gemm_nn_ok(an, wide_k, c)
    assert ops.GEMM_MAX_PITCH == GEMM_MAX_PITCH
    del wide_k, wide_m
    torch.cuda.empty_cache()
    # gemm_nt_swiglu_: a wave stages w rows up to F + 127 past its base, so the pitch that
    # gemm_nt_'s own guard (256 rows) accepts is refused once (F + 128) * pitch * 2 reaches 2^32
    F, pitch = 512, GEMM_NT_PITCH_LIMIT - 8
    assert 256 * pitch * 2 < 1 << 31 and (F + 128) * pitch * 2 >= 1 << 32
    w = torch.empty(2 * F, pitch, dtype=DT, device=DEV)[:, :K]
    gu, act = torch.zeros(M, 2 * F, dtype=DT, device=DEV), torch.zeros(M, F, dtype=DT, device=DEV)
    call("gemm_nt_swiglu_", (an, rnd(2 * F, K), gu, act))                  # the same shapes, dense w: accepted
    refusals("gemm_nt_swiglu_", (an, rnd(2 * F, K), gu, act), ((1, w),))
    assert ops.gemm_nt_swiglu_ok(an, rnd(2 * F, K)) and ops.gemm_nt_ok(an, w) and not ops.gemm_nt_swiglu_ok(an, w)


def _message(name, args):
    with pytest.raises(RuntimeError) as e:
        call(name, args)
    return str(e.value)


# ------------------------------------------------------------------ attention
def test_attn_decode():
    q, kc, vc = rnd(1, H, HD), rnd(1, G, T, HD), rnd(1, G, T, HD)
    _close(call("attn_decode", (q, kc, vc, T)), ref.attn_decode(f32(q), f32(kc), f32(vc), T), 2, name="decode")
    more = rnd(1, G, T + 1, HD)
    refusals("attn_decode", (q, kc, vc, T), ((0, strided(q)), (1, extra_dim(kc)), (1, strided(kc)), (2, wider(vc)),
             (2, more), (3, 0)))

    qkv = rnd(1, QKV)
    pos = torch.tensor([3], dtype=torch.int32, device=DEV)
    args = (qkv, kc.clone(), vc.clone(), pos, H, G)
    out = call("attn_decode_append", args)
    k2, v2 = f32(kc), f32(vc)
    k2[0, 0, 3], v2[0, 0, 3] = f32(qkv)[0, HD:2 * HD], f32(qkv)[0, 2 * HD:]
    _close(out, ref.attn_decode(f32(qkv)[:, :HD].view(1, H, HD), k2, v2, 4), 2, name="decode append")
    refusals("attn_decode_append", args, ((0, strided(qkv)), (1, extra_dim(kc)), (2, wider(vc)), (2, more),
             (3, longer(pos)), (3, wider(pos))))


def test_flash_attn():
    qkv, do = rnd(T, QKV), rnd(T, H * HD)
    args = (qkv, 1, T, H, G, HD, True, 0.0, 0, 0, None)
    o, lse = call("flash_attn_fwd", args)
    o0, lse0 = ref.flash_attn_fwd(f32(qkv), 1, T, H, G, HD, True)
    _close(o, o0, 2, name="o")
    check_elem(lse, lse0, **LSE_TOL, name="lse")
    refusals("flash_attn_fwd", args, ((0, strided(qkv)), (0, extra_dim(qkv)), (0, longer(qkv))))
    mask = torch.zeros(H, 1, T, dtype=torch.int32, device=DEV)
    pargs = (qkv, 1, T, H, G, HD, True, 0.1, 0, 0, mask)
    assert call("flash_attn_fwd", pargs)[0].shape == o.shape
    refusals("flash_attn_fwd", pargs, [(10, bad) for bad in (wider(mask), longer(mask), strided(mask))])

    args = (qkv, o, lse, do, 1, T, H, G, HD, True, 0.0, 0, 0, None, None, None)
    dqkv = call("flash_attn_bwd", args)
    _close(dqkv, ref.flash_attn_bwd(f32(qkv), f32(o), lse0, f32(do), 1, T, H, G, HD, True), 4, name="dqkv")
    cos, sin = ops.rope_tables(HD, T, 10000.0, device=DEV)
    refusals("flash_attn_bwd", args, ((0, strided(qkv)), (1, strided(o)), (1, wider(o)), (2, longer(lse.flatten())),
             (2, wider(lse)),
                   (2, strided(lse)), (3, wider(do)), (3, longer(do))))
    rargs = args[:14] + (cos, sin)
    assert call("flash_attn_bwd", rargs).shape == qkv.shape
    refusals("flash_attn_bwd", rargs, ((14, wider(cos)), (14, extra_dim(cos)), (15, wider(sin)), (15, strided(sin))))


def test_flash_attn_varlen():
    qkv, do = rnd(N, QKV), rnd(N, H * HD)
    cu = torch.tensor([0, 3, N], dtype=torch.int32, device=DEV)
    ids = torch.tensor([0, 1, 2, 0, 1, 2, 3, 4], dtype=torch.int32, device=DEV)
    args = (qkv, cu, 5, H, G, HD)
    o, lse = call("flash_attn_varlen_fwd", args)
    o0, lse0 = ref.flash_attn_varlen_fwd(f32(qkv), cu.cpu(), 5, H, G, HD)
    _close(o, o0, 2, name="o")
    check_elem(lse, lse0, **LSE_TOL, name="lse")
    refusals("flash_attn_varlen_fwd", args, ((0, strided(qkv)), (1, wider(cu)), (1, extra_dim(cu)), (1, strided(cu))))

    args = (qkv, o, lse, do, cu, ids, 5, H, G, HD, None, None)
    dqkv = call("flash_attn_varlen_bwd", args)
    want = ref.flash_attn_varlen_bwd(f32(qkv), f32(o), lse0, f32(do), cu.cpu(), ids.cpu(), 5, H, G, HD)
    _close(dqkv, want, 4, name="dqkv")
    refusals("flash_attn_varlen_bwd", args, ((1, wider(o)), (2, longer(lse)), (2, wider(lse)), (3, strided(do)),
             (4, wider(cu)), (5, longer(ids)),
                   (5, wider(ids))))


# ------------------------------------------------------------------ loss, embedding
def test_cross_entropy():
    logits = rnd(N, V)
    tg = torch.randint(0, V, (N,), device=DEV)
    loss, lse = call("ce_fwd", (logits, tg, -100))
    l0, lse0 = ref.ce_fwd(f32(logits), tg.cpu(), -100)
    check_elem(loss, l0, **LSE_TOL, name="loss")
    check_elem(lse, lse0, **LSE_TOL, name="lse")
    refusals("ce_fwd", (logits, tg, -100), ((0, strided(logits)), (0, extra_dim(logits)), (1, longer(tg)),
             (1, strided(tg))))

    scale = torch.full((1,), 0.125, device=DEV)
    args = (logits.clone(), tg, lse, scale, -100)
    call("ce_bwd_", args)
    _close(args[0], ref.ce_bwd_(f32(logits), tg.cpu(), lse0, scale.cpu(), -100), 2, name="dlogits")
    refusals("ce_bwd_", args, ((0, strided(logits)), (1, longer(tg)), (1, strided(tg)), (2, longer(lse)),
             (2, wider(lse)),
                   (2, strided(lse)), (3, wider(scale))))


def test_embedding():
    idx = torch.randint(0, V, (N,), device=DEV)
    wte, wpe, dx = rnd(V, D), rnd(T, D), rnd(N, D)
    args = (idx, wte, wpe, T, 0.0, 0, 0)
    _close(call("embedding_fwd", args), ref.embedding_fwd(idx.cpu(), f32(wte), f32(wpe), T), name="emb fwd")
    refusals("embedding_fwd", args, ((0, strided(idx)), (1, extra_dim(wte)), (1, strided(wte)), (2, wider(wpe)),
             (2, extra_dim(wpe)),
                   (2, strided(wpe)), (2, rnd(T, D + 8))))

    gw, gp = torch.zeros(V, D, dtype=DT, device=DEV), torch.zeros(T, D, dtype=DT, device=DEV)
    args = (idx, dx, gw, gp, T, False)
    call("embedding_bwd", args)
    gw0, gp0 = torch.zeros(V, D), torch.zeros(T, D)
    ref.embedding_bwd(idx.cpu(), f32(dx), gw0, gp0, T, False)
    _close(gw, gw0, 4, name="emb dW")
    _close(gp, gp0, 4, name="pos dW")
    refusals("embedding_bwd", args, ((0, longer(idx)), (1, extra_dim(dx)), (1, strided(dx)), (2, wider(gw)),
             (2, rnd(V, D + 8)),
                   (3, wider(gp)), (3, extra_dim(gp))))


# ------------------------------------------------------------------ LoRA, rank 16
def test_lora_down_up():
    x, w = rnd(N, D), rnd(R, D)
    args = (x, [w], [0], [D], [0], R, 0.5)
    t = call("lora_down", args)
    _close(t, ref.lora_down(f32(x), [f32(w)], [0], [D], [0], R, 0.5), 2, name="down")
    refusals("lora_down", args, ((0, misaligned(x)), (0, strided(x)), (0, extra_dim(x)), (1, [wider(w)]),
             (1, [misaligned(w)]),
                   (1, [w, w]), (5, 24)))
    out = torch.zeros(N, R + 8, dtype=DT, device=DEV)
    call("lora_down_into_", args + (out,))
    assert torch.equal(out[:, :R], t) and (out[:, R:] == 0).all()
    refusals("lora_down_into_", args + (out,), ((1, [wider(w)]), (7, wider(out)), (7, extra_dim(out)),
             (7, longer(out)), (7, strided(out))))

    u, y, base, bias = rnd(R, D), torch.zeros(N, D, dtype=DT, device=DEV), rnd(N, D), rnd(D)
    args = (y, t, [u], [0], [0], 2.0, base, bias)
    call("lora_up_", args)
    _close(y, f32(base) + f32(bias) + 2.0 * f32(t) @ f32(u), 2, name="up")
    refusals("lora_up_", args, ((0, misaligned(y)), (1, misaligned(t)), (1, wider(t)), (1, longer(t)), (2, [wider(u)]),
                   (2, [extra_dim(u)]), (6, wider(base)), (6, misaligned(base)), (6, longer(base)), (7, longer(bias)),
                   (7, wider(bias)), (7, misaligned(bias))))

    dst, B = torch.ones(D, R, dtype=DT, device=DEV), rnd(R, D)
    call("lora_block_", (dst, [B], [0], [0]))
    assert torch.equal(dst, B.t())
    refusals("lora_block_", (dst, [B], [0], [0]), ((0, extra_dim(dst)), (0, strided(dst.t()).t()), (1, [wider(B)]),
             (1, [strided(B)]),
                   (1, [longer(B)]), (1, [B, B])))

    As = [rnd(D, R), rnd(D, R)]
    assert torch.equal(call("lora_pack_t", (As,)), torch.cat([a.t() for a in As], 0))
    refusals("lora_pack_t", (As,), [(0, bad) for bad in ([As[0], wider(As[1])], [As[0], longer(As[1])], [As[0],
             strided(As[1])], [As[0], extra_dim(As[1])])])


def test_lora_grads():
    p, q = rnd(N, R), rnd(N, D)
    g = torch.zeros(R, D, device=DEV)
    args = (p, q, [g], [0], [0], 0.5, False)
    call("lora_wgrad", args)
    check_close(g, 0.5 * f32(p).t() @ f32(q), DT, k=K_OF[4], name="lora_wgrad")
    refusals("lora_wgrad", args, ((0, misaligned(p)), (1, misaligned(q)), (1, wider(q)), (1, longer(q)),
             (2, [extra_dim(g)]),
                   (2, [strided(g)]), (2, [g, g.double()]), (2, [longer(g)])))

    dl, st, B = rnd(N, V), rnd(N, R), rnd(R, V)
    u, gB = torch.zeros(N, R, dtype=DT, device=DEV), torch.zeros(R, V, device=DEV)
    args = (dl, st, B, u, gB, False)
    call("lora_head_bwd_", args)
    _close(u, f32(dl) @ f32(B).t(), 4, name="u")
    want = f32(st).t() @ f32(dl)
    check_elem(gB, want, rtol=1e-4, atol=1e-4 * want.abs().max().item(), name="gB")
    refusals("lora_head_bwd_", args, ((0, strided(dl)), (1, misaligned(st)), (1, wider(st)), (1, longer(st)),
             (2, longer(B)),
                   (2, wider(B)), (3, wider(u)), (3, strided(u)), (4, extra_dim(gB)), (4, longer(gB))))


# ------------------------------------------------------------------ optimizer
def test_optimizer():
    a, b = rnd(N, D), rnd(D, dt=torch.float32)
    s = call("sq_norm_multi", ([a, b],))
    check_elem(s, ref.sq_norm(f32(a)) + ref.sq_norm(f32(b)), rtol=1e-5, atol=0, name="sq_norm")
    refusals("sq_norm_multi", ([a, b],), [(0, bad) for bad in ([a, strided(b)], [strided(a), b], [a, b.double()])])

    n = N * D
    master, grad = rnd(n, dt=torch.float32), rnd(n)
    param, m, v = master.to(DT), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gs = torch.ones(1, device=DEV)
    args = (param, master, grad, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, gs)
    refs = [t.cpu().clone() for t in (param, master, grad, m, v)]
    call("adamw_step_", args)
    ref.adamw_step_(refs[0], refs[1], refs[2], refs[3], refs[4], 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, gs.cpu())
    check_elem(m, refs[3], rtol=1e-6, atol=1e-7, name="m")
    check_elem(master, refs[1], rtol=1e-6, atol=1e-7, name="master")
    _close(param, refs[0].float(), name="param")
    refusals("adamw_step_", args, ((0, strided(param)), (1, longer(master)), (1, wider(master)), (2, longer(grad)),
             (2, strided(grad)),
                   (3, wider(m)), (3, longer(m)), (4, wider(v)), (4, strided(v)), (11, wider(gs))))
