"""Split-KV decode attention (csrc/attn_decode_split.hip) on the GPU: the two ops against their
oracles at the chunk edges and beyond the single-launch kernel's 8,192 positions, what they may
and may not write, graph replay, their binding checks, and the model / generation paths that
reach them (forced through ``ops.DECODE_SPLIT_MIN`` on tiny caches, and at a context past 8,192)."""
import pytest
import torch
from numerics import NOMINAL, check_close

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.models.base import pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
K_DECODE = 3.0        # the decode kernels' class (tests/test_generate_ragged_gpu.py)
# tests/test_generate_ragged_gpu.py K_MODEL: 2e-2 of the reference logits' norm in check_close's unit
K_MODEL = 2e-2 / NOMINAL[BF16]


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


def _chunk():
    return int(torch.ops.bllm.attn_decode_split_chunk())


def _edges(C):
    """One key, around every chunk boundary of a 4-chunk cache, mid-chunk, the last slot."""
    return [0, 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 3 * C + 17, 4 * C - 1]


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b.to(a.device)))


def _f(t):
    return t.detach().to("cpu", torch.float32, copy=True)


def _rnd(*shape, dt):
    return torch.randn(*shape, device=DEV).to(dt)


def _case(dt, hd, H, Gk, pos, Tmax):
    """qkv rows, caches with every row at and above pos[b] NaN (they must not be read), pos."""
    B = len(pos)
    qkv = _rnd(B, (H + 2 * Gk) * hd, dt=dt)
    kc, vc = _rnd(B, Gk, Tmax, hd, dt=dt), _rnd(B, Gk, Tmax, hd, dt=dt)
    for b, p in enumerate(pos):
        kc[b, :, p:] = float("nan")
        vc[b, :, p:] = float("nan")
    return qkv, kc, vc, torch.tensor(pos, dtype=torch.int32, device=DEV)


def _check_append(out, qkv, kc, vc, k0, v0, pos, H, Gk, dt, name):
    """Cache row pos[b] is the qkv row's k / v, every other cache element is what it was, the
    output is finite and in the decode class of the oracle on fp32 copies."""
    B, Tmax, hd = len(pos), kc.shape[2], kc.shape[3]
    rows = qkv.view(B, H + 2 * Gk, hd)
    for b, p in enumerate(pos):
        assert _same_bits(kc[b, :, p], rows[b, H:H + Gk]), b
        assert _same_bits(vc[b, :, p], rows[b, H + Gk:]), b
        other = torch.ones(Tmax, dtype=torch.bool, device=DEV)
        other[p] = False
        assert _same_bits(kc[b][:, other], k0[b][:, other]), b
        assert _same_bits(vc[b][:, other], v0[b][:, other]), b
    assert torch.isfinite(out.float()).all()
    want = ref.attn_decode_append_rows(_f(qkv), _f(k0), _f(v0), torch.tensor(pos), H, Gk)
    check_close(out, want, dt, k=K_DECODE, name=name)


# ------------------------------------------------------------------ op level
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,Gk", [(4, 4), (8, 2), (4, 1), (8, 1)])
def test_append_split_per_row(dt, hd, H, Gk):
    C = _chunk()
    pos = _edges(C)
    qkv, kc, vc, pos_t = _case(dt, hd, H, Gk, pos, 4 * C)
    k0, v0 = kc.clone(), vc.clone()
    out = torch.ops.bllm.attn_decode_append_split(qkv, kc, vc, pos_t, H, Gk)
    torch.cuda.synchronize()
    _check_append(out, qkv, kc, vc, k0, v0, pos, H, Gk, dt, "split rows")


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd,H,Gk", [(64, 4, 1), (128, 8, 2), (64, 8, 1)])
def test_append_split_shared_position(dt, hd, H, Gk):
    """One position for all rows (pos of one element), and the per-row form at equal positions is
    the same launch: bitwise equal outputs and caches."""
    C = _chunk()
    for p in _edges(C):
        qkv, kc, vc, pos_t = _case(dt, hd, H, Gk, [p, p], 4 * C)
        k0, v0 = kc.clone(), vc.clone()
        kc1, vc1 = kc.clone(), vc.clone()
        out = torch.ops.bllm.attn_decode_append_split(qkv, kc, vc, pos_t[:1].clone(), H, Gk)
        rows = torch.ops.bllm.attn_decode_append_split(qkv, kc1, vc1, pos_t, H, Gk)
        torch.cuda.synchronize()
        _check_append(out, qkv, kc, vc, k0, v0, [p, p], H, Gk, dt, f"split shared pos {p}")
        assert _same_bits(out, rows) and _same_bits(kc, kc1) and _same_bits(vc, vc1), p


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd,H,Gk", [(64, 4, 4), (128, 8, 2), (64, 8, 1)])
def test_split_plain_length(dt, hd, H, Gk):
    C = _chunk()
    B, Tmax = 2, 4 * C
    for L in (1, C, C + 1, 4 * C):
        q = _rnd(B, H, hd, dt=dt)
        kc, vc = _rnd(B, Gk, Tmax, hd, dt=dt), _rnd(B, Gk, Tmax, hd, dt=dt)
        kc[:, :, L:] = float("nan")
        vc[:, :, L:] = float("nan")
        k0, v0 = kc.clone(), vc.clone()
        out = torch.ops.bllm.attn_decode_split(q, kc, vc, L)
        torch.cuda.synchronize()
        assert _same_bits(kc, k0) and _same_bits(vc, v0)
        assert torch.isfinite(out.float()).all()
        check_close(out, ref.attn_decode(_f(q), _f(kc), _f(vc), L), dt, k=K_DECODE, name=f"split plain L {L}")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_append_split_beyond_the_single_launch_limit(dt):
    C = _chunk()
    Tmax, H, Gk, hd = 8192 + C, 2, 1, 64
    pos = [8192, Tmax - 1]
    qkv, kc, vc, pos_t = _case(dt, hd, H, Gk, pos, Tmax)
    k0, v0 = kc.clone(), vc.clone()
    out = torch.ops.bllm.attn_decode_append_split(qkv, kc, vc, pos_t, H, Gk)
    torch.cuda.synchronize()
    _check_append(out, qkv, kc, vc, k0, v0, pos, H, Gk, dt, "split beyond 8192")


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


def test_append_split_stale_partials():
    """The captured call's partial buffer is filled for every chunk at positions near Tmax - 1,
    with scores far above anything that follows (q scaled up), then replayed at small positions:
    a merge that read the slots of chunks beyond L would be dominated by the stale ones."""
    C = _chunk()
    dt, hd, H, Gk, Tmax = BF16, 64, 8, 2, 4 * C
    qkv, kc, vc, pos = _case(dt, hd, H, Gk, [Tmax - 1, Tmax - 2, Tmax - 1], Tmax)
    kc.normal_()
    vc.normal_()
    qkv.mul_(8.0)
    graph, out = _capture(lambda: torch.ops.bllm.attn_decode_append_split(qkv, kc, vc, pos, H, Gk))
    graph.replay()                                      # every chunk's slot written, large maxima
    for new_pos in ([0, 5, C - 1], [C, 1, C + 3], [2 * C, 17, 0]):
        q2, k2, v2, p2 = _case(dt, hd, H, Gk, new_pos, Tmax)
        ke, ve = k2.clone(), v2.clone()
        eager = torch.ops.bllm.attn_decode_append_split(q2, ke, ve, p2, H, Gk)
        qkv.copy_(q2)
        kc.copy_(k2)
        vc.copy_(v2)
        pos.copy_(p2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        assert _same_bits(out, eager) and _same_bits(kc, ke) and _same_bits(vc, ve), new_pos
        want = ref.attn_decode_append_rows(_f(q2), _f(k2), _f(v2), torch.tensor(new_pos), H, Gk)
        check_close(out, want, dt, k=K_DECODE, name="split after stale partials")


@pytest.mark.parametrize("shared", [False, True])
def test_append_split_graph_replay_and_determinism(shared):
    """Captured once; replayed with other qkv rows, caches and positions written into the captured
    tensors: the eager call's result, bit for bit; and two eager calls agree bit for bit."""
    C = _chunk()
    dt, hd, H, Gk, Tmax = F16, 128, 8, 2, 4 * C
    qkv, kc, vc, pos = _case(dt, hd, H, Gk, [Tmax - 1] * 3, Tmax)
    kc.normal_()
    vc.normal_()
    if shared:
        pos = pos[:1].clone()
    graph, out = _capture(lambda: torch.ops.bllm.attn_decode_append_split(qkv, kc, vc, pos, H, Gk))
    for new_pos in ([3, C, 3 * C + 5], [2 * C - 1, 0, 4 * C - 1]):
        if shared:
            new_pos = [new_pos[0]] * 3
        q2, k2, v2, p2 = _case(dt, hd, H, Gk, new_pos, Tmax)
        if shared:
            p2 = p2[:1].clone()
        ke, ve = k2.clone(), v2.clone()
        eager = torch.ops.bllm.attn_decode_append_split(q2, ke, ve, p2, H, Gk)
        again = torch.ops.bllm.attn_decode_append_split(q2, k2.clone(), v2.clone(), p2, H, Gk)
        assert _same_bits(eager, again)
        qkv.copy_(q2)
        kc.copy_(k2)
        vc.copy_(v2)
        pos.copy_(p2)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, eager) and _same_bits(kc, ke) and _same_bits(vc, ve), new_pos


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd,H,Gk", [(64, 4, 4), (128, 8, 2), (64, 4, 1)])
def test_split_and_single_launch_kernels_agree_with_the_oracle(dt, hd, H, Gk):
    """Same inputs through both kernels: each within the decode class of the oracle (no bitwise
    claim between them: they sum in different orders)."""
    C = _chunk()
    pos = [p for p in _edges(C) if p < 2 * C]
    qkv, kc, vc, pos_t = _case(dt, hd, H, Gk, pos, 2 * C)
    k1, v1 = kc.clone(), vc.clone()
    want = ref.attn_decode_append_rows(_f(qkv), _f(kc), _f(vc), torch.tensor(pos), H, Gk)
    split = torch.ops.bllm.attn_decode_append_split(qkv, kc, vc, pos_t, H, Gk)
    single = torch.ops.bllm.attn_decode_append_rows(qkv, k1, v1, pos_t, H, Gk)
    torch.cuda.synchronize()
    check_close(split, want, dt, k=K_DECODE, name="split vs oracle")
    check_close(single, want, dt, k=K_DECODE, name="single launch vs oracle")
    assert _same_bits(kc, k1) and _same_bits(vc, v1)


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
    buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    v = buf[..., ::2]
    v.copy_(t)
    return v


def _misaligned(t):
    """The same values, contiguous, one element off the allocation's 16-byte alignment."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def test_binding_refusals():
    """In the style of tests/test_generate_ragged_gpu.py::test_binding_refusals: one accepted
    call, then one refused call per check with exactly one argument changed in the safe direction
    (longer, wider, strided or shifted inside a larger allocation, an extra dimension).  No
    out-of-range position or length reaches a kernel."""
    H, Gk, hd, T, B = 2, 1, 64, 8, 2
    qkv = _rnd(B, (H + 2 * Gk) * hd, dt=BF16)
    kc, vc = _rnd(B, Gk, T, hd, dt=BF16), _rnd(B, Gk, T, hd, dt=BF16)
    pos = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
    args = (qkv, kc.clone(), vc.clone(), pos, H, Gk)
    out = torch.ops.bllm.attn_decode_append_split(*args)
    want = ref.attn_decode_append_rows(_f(qkv), _f(kc), _f(vc), pos.cpu(), H, Gk)
    check_close(out, want, BF16, k=K_DECODE, name="split rows")
    _refusals("attn_decode_append_split", args, (
        (0, _strided(qkv)), (0, qkv.to(F32)), (0, qkv.unsqueeze(0)), (0, _misaligned(qkv)),
        (0, torch.cat([qkv, qkv[:1]])),
        (1, kc.unsqueeze(0)), (1, _strided(kc)), (1, _misaligned(kc)),
        (2, vc.to(F32)), (2, _rnd(B, Gk, T + 1, hd, dt=BF16)), (2, _misaligned(vc)),
        (3, torch.cat([pos, pos[:1]])), (3, pos.to(torch.int64)), (3, _strided(pos)),
        (4, 3),                                   # qkv no longer [B, (H + 2G) hd]
        (5, 2),                                   # not the cache's G
    ))
    # H that is no multiple of G, every shape consistent with it
    H3, G2 = 3, 2
    a = (_rnd(B, (H3 + 2 * G2) * hd, dt=BF16), _rnd(B, G2, T, hd, dt=BF16), _rnd(B, G2, T, hd, dt=BF16), pos, H3, G2)
    with pytest.raises(RuntimeError, match="attn_decode_append_split"):
        torch.ops.bllm.attn_decode_append_split(*a)
    # a head dim without a kernel
    a = (_rnd(B, (H + 2 * Gk) * 32, dt=BF16), _rnd(B, Gk, T, 32, dt=BF16), _rnd(B, Gk, T, 32, dt=BF16), pos, H, Gk)
    with pytest.raises(RuntimeError, match="attn_decode_append_split"):
        torch.ops.bllm.attn_decode_append_split(*a)

    q = _rnd(B, H, hd, dt=BF16)
    pargs = (q, kc.clone(), vc.clone(), 5)
    out = torch.ops.bllm.attn_decode_split(*pargs)
    check_close(out, ref.attn_decode(_f(q), _f(kc), _f(vc), 5), BF16, k=K_DECODE, name="split plain")
    _refusals("attn_decode_split", pargs, (
        (0, _strided(q)), (0, q.to(F32)), (0, q.unsqueeze(0)), (0, _misaligned(q)), (0, torch.cat([q, q[:1]])),
        (0, _rnd(B, H, 2 * hd, dt=BF16)),
        (1, kc.unsqueeze(0)), (1, _strided(kc)), (1, _misaligned(kc)),
        (2, vc.to(F32)), (2, _rnd(B, Gk, T + 1, hd, dt=BF16)), (2, _misaligned(vc)),
        (3, 0), (3, T + 1), (3, -1),
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


class _Recorder:
    """``torch.ops.bllm`` that notes the name of every op asked for."""

    def __init__(self):
        self.names = set()

    def __getattr__(self, name):
        self.names.add(name)
        return getattr(torch.ops.bllm, name)


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_model_row_steps_forced_onto_the_split_kernel(name, monkeypatch):
    """tests/test_generate_ragged_gpu.py::test_model_ragged_prefill_and_row_steps with every decode
    step sent to the split kernel (``DECODE_SPLIT_MIN = 0``): ragged prefill + 6 teacher-forced
    steps against the CPU fp32 full forward, eager and replayed from the graph."""
    gpu = _model((name, "gpu"), _cfgs()[name], BF16, DEV)
    cpu = _model((name, "cpu"), _cfgs()[name], F32, "cpu")
    cpu.load_state_dict(gpu.state_dict())
    assert gpu.cfg.head_dim == 64
    monkeypatch.setattr(ops, "DECODE_SPLIT_MIN", 0)
    rec = _Recorder()
    monkeypatch.setattr(ops, "_k", lambda: rec)
    lens, steps = [1, 7, 40, 13], 6
    g = torch.Generator().manual_seed(5)
    full = [torch.randint(0, gpu.cfg.vocab_size, (n + steps,), generator=g) for n in lens]
    with torch.no_grad():
        want = [cpu(f[None])[0] for f in full]
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, lens)], DEV)
    runs = []
    for graph in (False, True):
        cache = gpu.new_kv_cache(len(lens), 64)
        assert gpu.decode_graph_ok(cache)
        got = [gpu.forward_prefill_ragged(idx, seq, cache).clone()]
        pos = torch.tensor(lens, dtype=torch.int32, device=DEV)
        dec = G.RowsDecodeGraph(gpu, cache, pos, DEV) if graph else None
        for s in range(steps):
            tok = torch.stack([f[n + s] for f, n in zip(full, lens)])[:, None].to(DEV)
            if graph:
                got.append(dec.step(tok).clone())
            else:
                got.append(gpu.forward_cached_rows(tok, cache, pos).clone())
                pos += 1
        runs.append(got)
    assert "attn_decode_append_split" in rec.names and "attn_decode_append_rows" not in rec.names
    for s, (a, b) in enumerate(zip(*runs)):
        assert _same_bits(a, b), s                          # graph replay == eager
    for s, lg in enumerate(runs[0]):
        ref_rows = torch.stack([w[n - 1 + s] for w, n in zip(want, lens)])
        check_close(lg, ref_rows, BF16, k=K_MODEL, name=f"{name} split step {s}")


LONG_CTX = 8192 + 256
LONG_LENS = [8200, 5]


def _long_llama():
    return _model(("llama", "long"), _cfgs()["llama"].replace(context_length=LONG_CTX), BF16, DEV)


def test_model_long_context_row_steps():
    """A cache past 8,192 positions: one row decodes at positions 8,200.. (split kernel, more keys
    than the single-launch kernel holds), the other at 5..; six teacher-forced steps against the
    same model's full forward over each final sequence (flash attention)."""
    gpu = _long_llama()
    steps = 6
    g = torch.Generator().manual_seed(11)
    full = [torch.randint(0, gpu.cfg.vocab_size, (n + steps,), generator=g) for n in LONG_LENS]
    with torch.no_grad():
        want = [gpu(f[None].to(DEV))[0] for f in full]
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, LONG_LENS)], DEV)
    cache = gpu.new_kv_cache(len(LONG_LENS), LONG_CTX)
    assert cache[0][0].shape[2] == LONG_CTX and gpu.decode_graph_ok(cache)
    got = [gpu.forward_prefill_ragged(idx, seq, cache).clone()]
    pos = torch.tensor(LONG_LENS, dtype=torch.int32, device=DEV)
    for s in range(steps):
        tok = torch.stack([f[n + s] for f, n in zip(full, LONG_LENS)])[:, None].to(DEV)
        got.append(gpu.forward_cached_rows(tok, cache, pos).clone())
        pos += 1
    for s, lg in enumerate(got):
        ref_rows = torch.stack([w[n - 1 + s] for w, n in zip(want, LONG_LENS)])
        assert torch.isfinite(lg.float()).all()
        check_close(lg, ref_rows, BF16, k=K_MODEL, name=f"long context step {s}")


def test_generate_at_a_long_context(monkeypatch):
    """``generate_ragged`` and ``generate_cached`` with a cache of 8,448 positions and a prompt of
    8,200 tokens, greedy: the graph-replayed loop gives the eager loop's tokens, and a second run
    the same.  (With the single-launch kernels alone both calls raise from the binding.)"""
    gpu = _long_llama()
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, gpu.cfg.vocab_size, (n,), generator=g) for n in LONG_LENS]
    new = 12
    ragged, cached = {}, {}
    for tag, flag in (("graph", "1"), ("graph again", "1"), ("eager", "0")):
        monkeypatch.setenv("BLLM_DECODE_GRAPH", flag)
        ragged[tag] = G.generate_ragged(gpu, prompts, new, LONG_CTX)
        cached[tag] = G.generate_cached(gpu, prompts[0][None], new, LONG_CTX)
    for p, a, b, c in zip(prompts, ragged["graph"], ragged["graph again"], ragged["eager"]):
        assert a.numel() == p.numel() + new and torch.equal(a[:p.numel()].cpu(), p)
        assert torch.equal(a, b) and torch.equal(a, c)
    a, b, c = cached["graph"], cached["graph again"], cached["eager"]
    assert a.shape == (1, LONG_LENS[0] + new) and torch.equal(a[0, :LONG_LENS[0]].cpu(), prompts[0])
    assert torch.equal(a, b) and torch.equal(a, c)
