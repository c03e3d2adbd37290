"""Batched generation from ragged prompts on the GPU: the per-row decode kernel and the packed
cache fill against their oracles (bitwise where they copy), their binding checks, the model's
ragged prefill + per-row decode against the CPU fp32 full forward, and ``generate_ragged``."""
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
K_DECODE = 3.0        # tests/test_kernel_paths_gpu.py: the decode kernels' class (K_OF[2])


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


def _bits(t):
    """The bit pattern as integers: equality that tells NaNs and signed zeros apart."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b.to(a.device)))


def _f(t):
    return t.detach().to("cpu", torch.float32, copy=True)


def _rnd(*shape, dt):
    return torch.randn(*shape, device=DEV).to(dt)


# ------------------------------------------------------------------ attn_decode_append_rows
# B = 6 rows in a cache of 320 positions (the 256-thread key loop wraps once): one key, the wave
# edge (63 / 64 -> 64 / 65 keys), the block edge (255 -> 256 keys), the last slot
POS = [0, 1, 63, 64, 255, 319]
TMAX = 320


def _decode_case(dt, hd, H, Gk, pos):
    B = len(pos)
    qkv = _rnd(B, (H + 2 * Gk) * hd, dt=dt)
    kc, vc = _rnd(B, Gk, TMAX, hd, dt=dt), _rnd(B, Gk, TMAX, hd, dt=dt)
    for b, p in enumerate(pos):          # rows >= pos[b] must not be read: NaN
        kc[b, :, p:] = float("nan")
        vc[b, :, p:] = float("nan")
    return qkv, kc, vc, torch.tensor(pos, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,Gk", [(4, 4), (8, 2), (4, 1)])
def test_attn_decode_append_rows(dt, hd, H, Gk):
    qkv, kc, vc, pos = _decode_case(dt, hd, H, Gk, POS)
    k0, v0 = kc.clone(), vc.clone()
    out = ops.attn_decode_append_rows(qkv, kc, vc, pos, H, Gk)
    torch.cuda.synchronize()
    rows = qkv.view(len(POS), H + 2 * Gk, hd)
    for b, p in enumerate(POS):
        assert _same_bits(kc[b, :, p], rows[b, H:H + Gk]), b
        assert _same_bits(vc[b, :, p], rows[b, H + Gk:]), b
        other = torch.ones(TMAX, dtype=torch.bool, device=DEV)
        other[p] = False
        assert _same_bits(kc[b][:, other], k0[b][:, other]), b
        assert _same_bits(vc[b][:, other], v0[b][:, other]), b
    assert torch.isfinite(out.float()).all()
    want = ref.attn_decode_append_rows(_f(qkv), _f(k0), _f(v0), pos.cpu(), H, Gk)
    check_close(out, want, dt, k=K_DECODE, name="decode rows")


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd,H,Gk", [(64, 4, 4), (128, 8, 2)])
def test_attn_decode_append_rows_equal_positions_is_attn_decode_append(dt, hd, H, Gk):
    for p in (64, 255):
        qkv, kc, vc, pos = _decode_case(dt, hd, H, Gk, [p] * 3)
        kc1, vc1 = kc.clone(), vc.clone()
        a = ops.attn_decode_append_rows(qkv, kc, vc, pos, H, Gk)
        b = ops.attn_decode_append(qkv, kc1, vc1, pos[:1].clone(), H, Gk)
        assert _same_bits(a, b) and _same_bits(kc, kc1) and _same_bits(vc, vc1)


def test_attn_decode_append_rows_graph_replay():
    """Captured once; replayed with another position vector and other qkv rows written into the
    captured tensors: the result is the eager call's, bit for bit."""
    dt, hd, H, Gk = BF16, 128, 8, 2
    qkv, kc, vc, pos = _decode_case(dt, hd, H, Gk, [TMAX - 1] * 4)
    kc.normal_()
    vc.normal_()
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):                       # warm-up outside the capture
        ops.attn_decode_append_rows(qkv, kc, vc, pos, H, Gk)
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_decode_append_rows(qkv, kc, vc, pos, H, Gk)
    for new_pos in ([3, 64, 200, 0], [256, 1, 63, 318]):
        q2, k2, v2, p2 = _decode_case(dt, hd, H, Gk, new_pos)
        ke, ve = k2.clone(), v2.clone()
        eager = ops.attn_decode_append_rows(q2, ke, ve, p2, H, Gk)
        qkv.copy_(q2)
        kc.copy_(k2)
        vc.copy_(v2)
        pos.copy_(p2)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, eager) and _same_bits(kc, ke) and _same_bits(vc, ve)


# ------------------------------------------------------------------ kv_cache_fill_varlen
FILL_LENS = [1, 31, 64, 129, 0, 200]


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("Gk", [1, 2, 4])
def test_kv_cache_fill_varlen(dt, hd, Gk):
    H, Tmax, B = 4, 256, len(FILL_LENS)
    bounds = [0]
    for n in FILL_LENS:
        bounds.append(bounds[-1] + n)
    qkv = _rnd(bounds[-1], (H + 2 * Gk) * hd, dt=dt)
    cu = torch.tensor(bounds, dtype=torch.int32, device=DEV)
    kc = torch.full((B, Gk, Tmax, hd), float("nan"), device=DEV, dtype=dt)
    vc = torch.full((B, Gk, Tmax, hd), float("nan"), device=DEV, dtype=dt)
    kc[:, :, ::3] = 1.5                   # what must stay: NaNs and numbers
    vc[:, :, 1::3] = -2.5
    k0, v0 = kc.clone(), vc.clone()
    ops.kv_cache_fill_varlen(qkv, cu, kc, vc)
    torch.cuda.synchronize()
    rows = qkv.view(-1, H + 2 * Gk, hd)
    for b, n in enumerate(FILL_LENS):
        r0 = bounds[b]
        assert _same_bits(kc[b, :, :n], rows[r0:r0 + n, H:H + Gk].transpose(0, 1)), b
        assert _same_bits(vc[b, :, :n], rows[r0:r0 + n, H + Gk:].transpose(0, 1)), b
        assert _same_bits(kc[b, :, n:], k0[b, :, n:]) and _same_bits(vc[b, :, n:], v0[b, :, n:]), b
    # the oracle says the same
    k1, v1 = k0.cpu(), v0.cpu()
    ref.kv_cache_fill_varlen(qkv.cpu(), bounds, k1, v1)
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


def test_binding_refusals():
    """In the style of tests/test_binding_checks_gpu.py: one accepted call, then one refused call per
    check with exactly one argument changed in the safe direction (longer, wider, strided inside a
    larger allocation, an extra dimension).  No out-of-range position reaches a kernel."""
    H, Gk, hd, T, B = 1, 1, 64, 8, 2
    qkv = _rnd(B, (H + 2 * Gk) * hd, dt=BF16)
    kc, vc = _rnd(B, Gk, T, hd, dt=BF16), _rnd(B, Gk, T, hd, dt=BF16)
    pos = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
    args = (qkv, kc.clone(), vc.clone(), pos, H, Gk)
    out = torch.ops.bllm.attn_decode_append_rows(*args)
    want = ref.attn_decode_append_rows(_f(qkv), _f(kc), _f(vc), pos.cpu(), H, Gk)
    check_close(out, want, BF16, k=K_DECODE, name="decode rows")
    too_long = torch.zeros(B, Gk, 8192 + 1, hd, dtype=BF16, device=DEV)   # csrc/attn_decode.hip DEC_MAXL + 1
    _refusals("attn_decode_append_rows", args, (
        (0, _strided(qkv)), (0, qkv.to(F32)), (0, qkv.unsqueeze(0)),
        (1, kc.unsqueeze(0)), (1, _strided(kc)), (2, vc.to(F32)), (2, _rnd(B, Gk, T + 1, hd, dt=BF16)),
        (3, torch.cat([pos, pos[:1]])), (3, pos.to(torch.int64)), (3, _strided(pos)),
    ))
    # a cache longer than the LDS score buffer (both caches, so only that check can object)
    a = list(args)
    a[1], a[2] = too_long, too_long.clone()
    with pytest.raises(RuntimeError, match="attn_decode_append_rows"):
        torch.ops.bllm.attn_decode_append_rows(*a)

    packed = _rnd(6, (H + 2 * Gk) * hd, dt=BF16)
    cu = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    fargs = (packed, cu, kc.clone(), vc.clone())
    torch.ops.bllm.kv_cache_fill_varlen(*fargs)
    k1, v1 = kc.cpu().clone(), vc.cpu().clone()
    ref.kv_cache_fill_varlen(packed.cpu(), [0, 2, 6], k1, v1)
    assert _same_bits(fargs[2], k1) and _same_bits(fargs[3], v1)
    _refusals("kv_cache_fill_varlen", fargs, (
        (0, _strided(packed)), (0, packed.to(F32)), (0, packed.unsqueeze(0)),
        (1, torch.cat([cu, cu[-1:]])), (1, cu.to(torch.int64)), (1, _strided(cu)),
        (2, kc.unsqueeze(0)), (2, _strided(kc)), (3, vc.to(F32)), (3, _rnd(B, Gk, T + 1, hd, dt=BF16)),
    ))


# ------------------------------------------------------------------ model
def _cfgs():
    llama = get_config("llama3_2", "1B").replace(context_length=64, emb_dim=256, n_heads=4, n_kv_groups=2,
                                                 hidden_dim=384, n_layers=2, vocab_size=512)
    gpt = get_config("GPT2", "124M").replace(context_length=64, emb_dim=256, n_heads=4, n_kv_groups=4, hidden_dim=1024,
                                             n_layers=2, vocab_size=512, drop_rate=0.0)
    return {"llama": llama, "gpt2": gpt}


_PAIRS = {}


def _pair(name):
    """(bf16 GPU model, the CPU fp32 model with the same weights), built once per family."""
    if name not in _PAIRS:
        cfg = _cfgs()[name]
        torch.manual_seed(0)
        gpu = build_model(cfg.replace(dtype=BF16), device=DEV)
        cpu = build_model(cfg.replace(dtype=F32))
        cpu.load_state_dict(gpu.state_dict())
        for m in (gpu, cpu):
            m.flatten()
            m.eval()
        _PAIRS[name] = (gpu, cpu)
    return _PAIRS[name]


# tests/test_model_gpu.py bounds forward_cached's bf16 logits by 2e-2 of the full forward's norm;
# in check_close's unit (the bf16 rounding error, numerics.NOMINAL) that is k = 2e-2 / 1.67e-3
K_MODEL = 2e-2 / NOMINAL[BF16]


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_model_ragged_prefill_and_row_steps(name):
    gpu, cpu = _pair(name)
    assert gpu.cfg.head_dim == 64
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
    for s, (a, b) in enumerate(zip(*runs)):
        assert _same_bits(a, b), s                          # graph replay == eager
    for s, lg in enumerate(runs[0]):
        ref_rows = torch.stack([w[n - 1 + s] for w, n in zip(want, lens)])
        check_close(lg, ref_rows, BF16, k=K_MODEL, name=f"{name} ragged step {s}")


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_ragged_deterministic_and_graph_equals_eager(name, monkeypatch):
    gpu, _ = _pair(name)
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, gpu.cfg.vocab_size, (n,), generator=g) for n in [1, 7, 40, 13]]
    runs = {}
    for tag, flag in (("graph", "1"), ("graph again", "1"), ("eager", "0")):
        monkeypatch.setenv("BLLM_DECODE_GRAPH", flag)
        runs[tag] = G.generate_ragged(gpu, prompts, 24, 64)
    for p, a, b, c in zip(prompts, runs["graph"], runs["graph again"], runs["eager"]):
        assert a.numel() == p.numel() + 24 and torch.equal(a[:p.numel()].cpu(), p)
        assert torch.equal(a, b) and torch.equal(a, c)


def test_generate_ragged_fp32_takes_the_oracle_decode_path():
    """fp32 has no HIP decode kernel: ``ops.attn_decode_append_rows`` hands GPU fp32 tensors to the
    oracle (as ``ops.attn_decode`` does) while RoPE, the variable-length prefill and the cache fill
    stay on their fp32 kernels, and no graph is captured.  Greedy rows equal the one-row
    ``generate_cached`` runs of the same model.  Premise, checked first: no one-row step has a
    runner-up within 1e-4 of its argmax.  A 1-row and a 4-row batch may take GEMM kernels that sum in
    another order: logits of magnitude ~2 over K = 256 then differ by about sqrt(K) * 2^-24 * 2 = 2e-6,
    so 1e-4 leaves a factor 50."""
    cfg = _cfgs()["llama"].replace(dtype=F32)
    torch.manual_seed(0)
    m = build_model(cfg, device=DEV)
    m.flatten()
    m.eval()
    assert not m.decode_graph_ok(m.new_kv_cache(1, 64))
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in [1, 7, 40, 13]]
    ones = [G.generate_cached(m, p[None], 12, 64)[0] for p in prompts]
    with torch.no_grad():
        for p, o in zip(prompts, ones):
            top = m(o[None])[0, p.numel() - 1:-1].float().topk(2, dim=-1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 1e-4
    for o, r in zip(ones, G.generate_ragged(m, prompts, 12, 64)):
        assert torch.equal(o, r)
