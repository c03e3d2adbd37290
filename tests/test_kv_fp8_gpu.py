"""FP8 KV cache on the GPU (csrc/attn_decode_fp8.hip): the quantised fill and the append + decode
step against the oracles of ops/reference.py -- bytes and scale bits bitwise, outputs in the decode
kernels' class -- at the chunk edges and past 8,192 positions; stale partials, graph replay, row
isolation, the binding's refusals, and the model / generation paths that reach the kernels."""
import pytest
import torch
from numerics import _report, check_close

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.models.base import pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
K_DECODE = 3.0        # the decode kernels' class (tests/test_decode_split_gpu.py)
NAN8 = 0x7F           # e4m3fn NaN: a byte that must never reach a sum
EDGES = [0, 1, 254, 255, 256, 257, 511, 512, 767]


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


def _u8(t):
    return t.contiguous().view(torch.uint8)


def _i32(t):
    return t.contiguous().view(torch.int32)


def _same_cache(a, b):
    """Two (K8, V8, Ks, Vs): equal bytes and equal scale bits (NaN sentinels included)."""
    return all(torch.equal(_u8(x), _u8(y.to(x.device))) for x, y in zip(a[:2], b[:2])) and \
        all(torch.equal(_i32(x), _i32(y.to(x.device))) for x, y in zip(a[2:], b[2:]))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.to(a.device).contiguous().view(torch.int16))


def _f(t):
    return t.detach().to("cpu", torch.float32, copy=True)


def _cpu(cache):
    return tuple(t.detach().to("cpu", copy=True) for t in cache)


def _rnd(*shape, dt):
    return torch.randn(*shape, device=DEV).to(dt)


def _case(dt, hd, H, Gk, pos, Tmax, vscale=2.0):
    """qkv rows; an fp8 cache of quantised random rows whose slots at and above pos[b] hold NaN
    bytes and NaN scales (they must not be read); pos."""
    B = len(pos)
    qkv = _rnd(B, (H + 2 * Gk) * hd, dt=dt)
    k8, ks = ref.kv_quantize_rows(torch.randn(B, Gk, Tmax, hd, device=DEV))
    v8, vs = ref.kv_quantize_rows(torch.randn(B, Gk, Tmax, hd, device=DEV) * vscale)
    for b, p in enumerate(pos):
        _u8(k8)[b, :, p:] = NAN8
        _u8(v8)[b, :, p:] = NAN8
        ks[b, :, p:] = float("nan")
        vs[b, :, p:] = float("nan")
    return qkv, (k8, v8, ks, vs), torch.tensor(pos, dtype=torch.int32, device=DEV)


def _step(qkv, cache, pos_t, H, Gk):
    k8, v8, ks, vs = cache
    return torch.ops.bllm.attn_decode_append_rows_fp8(qkv, k8, ks, v8, vs, pos_t, H, Gk)


def _oracle(qkv, cache0, pos, H, Gk):
    """The oracle on fp32 copies of the inputs: (output, the cache after the append)."""
    c = _cpu(cache0)
    out = ref.attn_decode_append_rows_fp8(_f(qkv), c[0], c[1], c[2], c[3], torch.tensor(pos), H, Gk)
    return out, c


def _check_step(out, qkv, cache, cache0, pos, H, Gk, dt, name):
    want, after = _oracle(qkv, cache0, pos, H, Gk)
    assert _same_cache(cache, after), name           # the appended bytes and scales, nothing else changed
    assert torch.isfinite(out.float()).all(), name
    check_close(out, want, dt, k=K_DECODE, name=name)


# ------------------------------------------------------------------ fill
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd", [64, 128])
def test_fill_bitwise(dt, hd):
    H, Gk, Tmax = 4, 2, 512
    lens = [1, 255, 256, 257, 300]
    B, N = len(lens), sum(lens)
    qkv = _rnd(N, (H + 2 * Gk) * hd, dt=dt)
    rows = qkv.view(N, H + 2 * Gk, hd)
    rows[3, H] = 0                                     # an all-zero k row
    rows[5, H + Gk + 1] = 0                            # an all-zero v row
    rows[7, H + 1, 11] = rows[7, H + 1].abs().max() * 100      # one 100x outlier
    rows[400, H + Gk, 0] = -rows[400, H + Gk].abs().max() * 100
    rows[9, H, :] = 1e-3 * rows[9, H, :]               # a small row
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    k8 = torch.full((B, Gk, Tmax, hd), 0x55, dtype=torch.uint8, device=DEV).view(F8)
    v8 = torch.full((B, Gk, Tmax, hd), 0x2A, dtype=torch.uint8, device=DEV).view(F8)
    ks = torch.full((B, Gk, Tmax), 7.0, device=DEV)
    vs = torch.full((B, Gk, Tmax), -7.0, device=DEV)
    want = _cpu((k8, v8, ks, vs))
    ops.kv_cache_fill_varlen(qkv, cu, k8, v8, scales=(ks, vs))
    torch.cuda.synchronize()
    ref.kv_cache_fill_varlen_fp8(_f(qkv), cu.cpu(), *want)
    assert _same_cache((k8, v8, ks, vs), want)
    for b, n in enumerate(lens):                       # the sentinels, stated on their own
        assert (_u8(k8[b, :, n:]) == 0x55).all() and (_u8(v8[b, :, n:]) == 0x2A).all()
        assert (ks[b, :, n:] == 7.0).all() and (vs[b, :, n:] == -7.0).all()
    assert float(ks[0, 0, 0]) != 7.0 and float(want[2][1, 0, 2]) == 1.0      # row 3 = (b 1, t 2): the zero row


# ------------------------------------------------------------------ append + decode
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,Gk", [(4, 4), (8, 2), (4, 1), (8, 1)])
def test_append_rows_at_the_chunk_edges(dt, hd, H, Gk):
    qkv, cache, pos_t = _case(dt, hd, H, Gk, EDGES, 768)
    cache0 = _cpu(cache)
    out = _step(qkv, cache, pos_t, H, Gk)
    torch.cuda.synchronize()
    _check_step(out, qkv, cache, cache0, EDGES, H, Gk, dt, "fp8 rows")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_append_rows_zero_and_outlier_rows(dt):
    """The appended k is all zero (scale 1, bytes 0) in one row and has a 100x outlier in another."""
    H, Gk, hd, pos = 4, 2, 64, [5, 256, 300]
    qkv, cache, pos_t = _case(dt, hd, H, Gk, pos, 768)
    rows = qkv.view(3, H + 2 * Gk, hd)
    rows[0, H] = 0
    rows[1, H + Gk, 3] = 300.0
    rows[2, H + 1, 60] = -250.0
    cache0 = _cpu(cache)
    out = _step(qkv, cache, pos_t, H, Gk)
    torch.cuda.synchronize()
    assert float(cache[2][0, 0, 5]) == 1.0 and (_u8(cache[0][0, 0, 5]) == 0).all()
    _check_step(out, qkv, cache, cache0, pos, H, Gk, dt, "fp8 rows zero / outlier")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_append_rows_beyond_the_single_launch_limit(dt):
    H, Gk, hd, pos = 2, 1, 64, [8200, 5]
    qkv, cache, pos_t = _case(dt, hd, H, Gk, pos, 8192 + 256)
    cache0 = _cpu(cache)
    out = _step(qkv, cache, pos_t, H, Gk)
    torch.cuda.synchronize()
    _check_step(out, qkv, cache, cache0, pos, H, Gk, dt, "fp8 rows beyond 8192")


def test_ops_route_to_the_kernels(monkeypatch):
    """``ops.attn_decode_append_rows`` with scales reaches the fp8 kernel at every cache length (no
    single-launch sibling); fp32 activations on the GPU go to the oracle."""
    names = set()

    class Rec:
        def __getattr__(self, n):
            names.add(n)
            return getattr(torch.ops.bllm, n)

    monkeypatch.setattr(ops, "_k", lambda: Rec())
    H, Gk, hd, pos = 4, 2, 64, [3, 17]
    qkv, cache, pos_t = _case(BF16, hd, H, Gk, pos, 32)
    cache0 = _cpu(cache)
    out = ops.attn_decode_append_rows(qkv, cache[0], cache[1], pos_t, H, Gk, scales=cache[2:])
    assert names == {"attn_decode_append_rows_fp8"}
    _check_step(out, qkv, cache, cache0, pos, H, Gk, BF16, "fp8 rows through ops")
    names.clear()
    q32, c32, _ = _case(F32, hd, H, Gk, pos, 32)
    c0 = _cpu(c32)
    out = ops.attn_decode_append_rows(q32, c32[0], c32[1], pos_t, H, Gk, scales=c32[2:])
    assert not names
    want, after = _oracle(q32, c0, pos, H, Gk)
    assert _same_cache(c32, after)
    check_close(out, want, F32, k=K_DECODE, name="fp8 rows fp32 oracle on the GPU")


def _capture(fn):
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):                       # warm-up outside the capture
        fn()
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def _load(dst_qkv, dst_cache, dst_pos, qkv, cache, pos_t):
    dst_qkv.copy_(qkv)
    for d, s in zip(dst_cache, cache):
        if d.dtype == F8:
            d, s = _u8(d), _u8(s)
        d.copy_(s)
    dst_pos.copy_(pos_t)


def test_stale_partials():
    """One captured step, so one workspace: a step at position 700 with scores far above anything
    that follows (q scaled up) fills the slots of chunks 0..2; the step at position 3 must merge
    chunk 0 alone."""
    dt, hd, H, Gk, Tmax = BF16, 64, 8, 2, 768
    qkv, cache, pos_t = _case(dt, hd, H, Gk, [700, 700], Tmax)
    qkv.mul_(8.0)
    graph, out = _capture(lambda: _step(qkv, cache, pos_t, H, Gk))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    q2, c2, p2 = _case(dt, hd, H, Gk, [3, 3], Tmax)
    cache0 = _cpu(c2)
    _load(qkv, cache, pos_t, q2, c2, p2)
    graph.replay()
    torch.cuda.synchronize()
    _check_step(out, q2, cache, cache0, [3, 3], H, Gk, dt, "fp8 after stale partials")


def test_graph_replay_and_determinism():
    """Captured once; replayed at positions 254..258 (across a chunk boundary) with new qkv rows
    and caches written into the captured tensors: the eager call bit for bit, and two eager calls
    agree bit for bit."""
    dt, hd, H, Gk, Tmax = F16, 128, 8, 2, 768
    qkv, cache, pos_t = _case(dt, hd, H, Gk, [767, 767], Tmax)
    graph, out = _capture(lambda: _step(qkv, cache, pos_t, H, Gk))
    for p in range(254, 259):
        q2, c2, p2 = _case(dt, hd, H, Gk, [p, 767 - p], Tmax)
        ce, ca = tuple(t.clone() for t in c2), tuple(t.clone() for t in c2)
        eager = _step(q2, ce, p2, H, Gk)
        again = _step(q2, ca, p2, H, Gk)
        assert _same_bits(eager, again) and _same_cache(ce, ca), p
        _load(qkv, cache, pos_t, q2, c2, p2)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, eager) and _same_cache(cache, ce), p


def test_rows_are_isolated():
    """Other values in row 1's qkv and cache: no bit of row 0's output or cache changes."""
    dt, hd, H, Gk, Tmax, pos = BF16, 64, 8, 2, 768, [300, 520]
    qkv, cache, pos_t = _case(dt, hd, H, Gk, pos, Tmax)
    q2, c2, _ = _case(dt, hd, H, Gk, pos, Tmax, vscale=5.0)
    q2[0] = qkv[0]
    for a, b in zip(c2, cache):
        (_u8(a) if a.dtype == F8 else a)[0] = (_u8(b) if b.dtype == F8 else b)[0]
    o1 = _step(qkv, cache, pos_t, H, Gk)
    o2 = _step(q2, c2, pos_t, H, Gk)
    torch.cuda.synchronize()
    assert _same_bits(o1[0], o2[0]) and not _same_bits(o1[1], o2[1])
    assert _same_cache(tuple(t[0] for t in cache), tuple(t[0] for t in c2))


# ------------------------------------------------------------------ binding refusals
def _refused(name, args, i, bad):
    a = list(args)
    a[i] = bad
    try:
        getattr(torch.ops.bllm, name)(*a)
    except RuntimeError as e:
        return None if name in str(e) else f"{name} argument {i}: the message lacks the op name: {e}"
    return f"{name} argument {i}: accepted"


def _refusals(name, args, cases):
    missed = [m for m in (_refused(name, args, i, bad) for i, bad in cases) if m]
    assert not missed, "\n".join(missed)


def _strided(t):
    """The same shape with a stride of two elements in the last dimension."""
    if t.dtype == F8:
        return torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=torch.uint8, device=t.device).view(F8)[..., ::2]
    buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    v = buf[..., ::2]
    v.copy_(t)
    return v


def _misaligned(t):
    """The same shape, contiguous, one element off the allocation's 16-byte alignment."""
    raw = torch.zeros(t.numel() + 16, dtype=torch.uint8 if t.dtype == F8 else t.dtype, device=t.device)
    if t.dtype == F8:
        raw = raw.view(F8)
    return raw[1:1 + t.numel()].view(t.shape)


def test_binding_refusals():
    """One accepted call, then one refused call per check with exactly one argument changed in the
    safe direction (longer, wider, strided or shifted inside a larger allocation, an extra
    dimension); every refusal comes from the argument checks, before any launch."""
    H, Gk, hd, T, B = 2, 1, 64, 8, 2
    pos = [3, 5]
    qkv, (k8, v8, ks, vs), pos_t = _case(BF16, hd, H, Gk, pos, T)
    cache0 = _cpu((k8, v8, ks, vs))
    args = (qkv, k8, ks, v8, vs, pos_t, H, Gk)
    out = torch.ops.bllm.attn_decode_append_rows_fp8(*args)
    _check_step(out, qkv, (k8, v8, ks, vs), cache0, pos, H, Gk, BF16, "fp8 rows accepted")
    wide8 = torch.zeros(B, Gk, T + 1, hd, dtype=torch.uint8, device=DEV).view(F8)
    _refusals("attn_decode_append_rows_fp8", args, (
        (0, _strided(qkv)), (0, qkv.to(F32)), (0, qkv.unsqueeze(0)), (0, _misaligned(qkv)),
        (0, torch.cat([qkv, qkv[:1]])),
        (1, k8.unsqueeze(0)), (1, _strided(k8)), (1, _misaligned(k8)), (1, _u8(k8)), (1, k8.to(BF16)),
        (2, ks.double()), (2, ks[:, :, :-1].contiguous()), (2, ks.unsqueeze(-1)), (2, _strided(ks)),
        (2, torch.zeros(B, Gk, T + 1, device=DEV)),
        (3, v8.to(BF16)), (3, wide8), (3, _misaligned(v8)),
        (4, vs.to(BF16)), (4, torch.zeros(B, Gk + 1, T, device=DEV)), (4, _strided(vs)),
        (5, torch.cat([pos_t, pos_t[:1]])), (5, pos_t.to(torch.int64)), (5, _strided(pos_t)), (5, pos_t[:1]),
        (6, 3),                                   # qkv no longer [B, (H + 2G) hd]
        (7, 2),                                   # not the cache's G
    ))
    # H that is no multiple of G, every shape consistent with it
    H3, G2 = 3, 2
    q3, c3, _ = _case(BF16, hd, H3, G2, pos, T)
    with pytest.raises(RuntimeError, match="attn_decode_append_rows_fp8"):
        torch.ops.bllm.attn_decode_append_rows_fp8(q3, c3[0], c3[2], c3[1], c3[3], pos_t, H3, G2)
    # a head dim without a kernel
    q4, c4, _ = _case(BF16, 32, H, Gk, pos, T)
    with pytest.raises(RuntimeError, match="attn_decode_append_rows_fp8"):
        torch.ops.bllm.attn_decode_append_rows_fp8(q4, c4[0], c4[2], c4[1], c4[3], pos_t, H, Gk)
    # a grid beyond attn_decode_split_grid_ok: G (H / G = 1) past the y dimension; the tensors are empty
    # in B so that nothing large is allocated -- refused on B first, so ask with B = 1 and a tiny Tmax
    Gbig = 65536
    qb = torch.zeros(1, 3 * Gbig * hd, dtype=BF16, device=DEV)
    kb = torch.zeros(1, Gbig, 1, hd, dtype=torch.uint8, device=DEV).view(F8)
    sb = torch.zeros(1, Gbig, 1, device=DEV)
    with pytest.raises(RuntimeError, match="attn_decode_append_rows_fp8.*exceeds the launch grid"):
        torch.ops.bllm.attn_decode_append_rows_fp8(qb, kb, sb, kb.clone(), sb.clone(), pos_t[:1] * 0, Gbig, Gbig)

    cu = torch.tensor([0, 3, 8], dtype=torch.int32, device=DEV)
    pq = _rnd(8, (H + 2 * Gk) * hd, dt=BF16)
    fargs = (pq, cu, k8, ks, v8, vs)
    torch.ops.bllm.kv_cache_fill_varlen_fp8(*fargs)
    want = _cpu((k8, v8, ks, vs))
    ref.kv_cache_fill_varlen_fp8(_f(pq), cu.cpu(), *want)
    torch.cuda.synchronize()
    assert _same_cache((k8, v8, ks, vs), want)
    _refusals("kv_cache_fill_varlen_fp8", fargs, (
        (0, _strided(pq)), (0, pq.to(F32)), (0, pq.unsqueeze(0)), (0, _misaligned(pq)),
        (0, _rnd(8, 2 * Gk * hd, dt=BF16)),       # no query head left
        (1, cu.to(torch.int64)), (1, torch.cat([cu, cu[-1:]])), (1, _strided(cu)),
        (2, k8.unsqueeze(0)), (2, _strided(k8)), (2, _misaligned(k8)), (2, k8.to(BF16)),
        (3, ks.double()), (3, torch.zeros(B, Gk, T + 1, device=DEV)), (3, _strided(ks)),
        (4, wide8), (4, _misaligned(v8)), (4, _u8(v8)),
        (5, vs.to(BF16)), (5, vs.unsqueeze(-1)), (5, _strided(vs)),
    ))


# ------------------------------------------------------------------ model level
def _cfgs():
    """The tiny head-dim-64 configurations of tests/test_generate_ragged_gpu.py::_cfgs."""
    llama = get_config("llama3_2", "1B").replace(context_length=64, emb_dim=256, n_heads=4, n_kv_groups=2,
                                                 hidden_dim=384, n_layers=2, vocab_size=512)
    gpt = get_config("GPT2", "124M").replace(context_length=64, emb_dim=256, n_heads=4, n_kv_groups=4, hidden_dim=1024,
                                             n_layers=2, vocab_size=512, drop_rate=0.0)
    return {"llama": llama, "gpt2": gpt}


_MODELS = {}


def _model(key, cfg, dt, device):
    if key not in _MODELS:
        torch.manual_seed(0)
        m = build_model(cfg.replace(dtype=dt), device=device)
        m.flatten()
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


def _teacher_forced(m, full, lens, steps, device, kv_dtype, graph=False):
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, lens)], device)
    cache = m.new_kv_cache(len(lens), 64, kv_dtype=kv_dtype)
    with torch.no_grad():
        got = [m.forward_prefill_ragged(idx, seq, cache).clone()]
        pos = torch.tensor(lens, dtype=torch.int32, device=device)
        dec = G.RowsDecodeGraph(m, cache, pos, device) if graph else None
        for s in range(steps):
            tok = torch.stack([f[n + s] for f, n in zip(full, lens)])[:, None].to(device)
            if graph:
                got.append(dec.step(tok).clone())
            else:
                got.append(m.forward_cached_rows(tok, cache, pos).clone())
                pos += 1
    return torch.stack(got), cache


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_model_row_steps_on_the_fp8_cache(name):
    """Ragged prefill + 12 teacher-forced row steps, bf16 on the GPU with the fp8 cache, against
    the CPU fp32 model with the fp8 cache through the oracle.  The two sides quantise slightly
    different K / V, so single roundings can flip and no bound follows from the format; E_q, the
    CPU fp32 model's own relative logits difference between the fp8 and the exact cache, is the
    size of what quantising does, and the GPU may differ from the CPU fp8 run by at most
    2 * max(2e-2, E_q): the project's whole-model bound, or flips on both sides."""
    gpu = _model((name, "gpu"), _cfgs()[name], BF16, DEV)
    cpu = _model((name, "cpu"), _cfgs()[name], F32, "cpu")
    cpu.load_state_dict(gpu.state_dict())
    lens, steps = [1, 7, 40, 13], 12
    g = torch.Generator().manual_seed(5)
    full = [torch.randint(0, gpu.cfg.vocab_size, (n + steps,), generator=g) for n in lens]
    cache = gpu.new_kv_cache(len(lens), 64, kv_dtype="fp8")
    assert gpu.decode_graph_ok(cache) and len(cache[0]) == 4 and cache[0][0].dtype == F8
    exact, _ = _teacher_forced(cpu, full, lens, steps, "cpu", None)
    want, _ = _teacher_forced(cpu, full, lens, steps, "cpu", "fp8")
    got, _ = _teacher_forced(gpu, full, lens, steps, DEV, "fp8")
    replay, _ = _teacher_forced(gpu, full, lens, steps, DEV, "fp8", graph=True)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, replay)                     # graph replay == eager
    e_q = _rel(want[1:], exact[1:])
    err = _rel(got[1:], want[1:])
    bound = 2 * max(2e-2, e_q)
    print(f"{name}: E_q {e_q:.3e}  gpu-vs-cpu {err:.3e}  bound {bound:.3e}")
    _report(f"kv fp8 {name} E_q (absolute, not a ratio)", e_q)
    _report(f"kv fp8 {name} gpu-vs-cpu logits error / bound", err / bound)
    assert e_q > 0.0 and err <= bound, (e_q, err, bound)


def test_generate_and_capacity(monkeypatch):
    """``generate_ragged`` on the fp8 cache: the graph-replayed run returns the lengths of the eager
    run; and the cache allocation is (hd + 4) / (2 hd) of the bf16 one, within 2 %."""
    gpu = _model(("llama", "gpu"), _cfgs()["llama"], BF16, DEV)
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, gpu.cfg.vocab_size, (n,), generator=g) for n in (3, 30, 11)]
    new, runs = 12, {}
    for flag in ("1", "0"):
        monkeypatch.setenv("BLLM_DECODE_GRAPH", flag)
        runs[flag] = G.generate_ragged(gpu, prompts, new, 64, kv_dtype="fp8")
    for p, a, b in zip(prompts, runs["1"], runs["0"]):
        assert a.numel() == b.numel() == p.numel() + new and torch.equal(a[:p.numel()].cpu(), p)

    def peak(kv_dtype):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        cache = gpu.new_kv_cache(8, 64, kv_dtype=kv_dtype)
        used = torch.cuda.max_memory_allocated() - base
        del cache
        return used

    hd = gpu.cfg.head_dim
    ratio = peak("fp8") / peak(None)
    assert abs(ratio / ((hd + 4) / (2 * hd)) - 1) <= 0.02, ratio
