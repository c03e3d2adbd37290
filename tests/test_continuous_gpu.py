"""Continuous batching on the GPU: the slot-mapped cache fills against their oracles bit for bit,
the binding's checks of the new argument, admission into a live cache against the CPU fp32 forward
(eager, under a captured ``RowsDecodeGraph``, and on the fp8 cache), ``generate_continuous`` end to
end, and a slot's independence of its index."""
import os
import subprocess
import sys

import pytest
import torch
from numerics import check_close

import continuous_cases as C
from test_generate_ragged_gpu import K_MODEL, _cfgs, _pair, _refusals, _same_bits, _strided

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.models.base import pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


def _u8(t):
    return t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------ fill kernels, bitwise
FILL_LENS, FILL_ROWS, LEAD, CACHE_ROWS, TMAX, H = [1, 31, 64, 129, 0], [5, 0, 3, 2, 4], 3, 6, 256, 4


def _packed(dt, hd, Gk):
    """qkv with ``LEAD`` leading rows outside every sequence, and its cu (cu[0] = LEAD)."""
    bounds = [LEAD]
    for n in FILL_LENS:
        bounds.append(bounds[-1] + n)
    qkv = torch.randn(bounds[-1], (H + 2 * Gk) * hd, device=DEV).to(dt)
    return qkv, bounds, torch.tensor(bounds, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dt", [BF16, F16, F32])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("Gk", [1, 2])
def test_fill_into_chosen_rows_bitwise(dt, hd, Gk):
    qkv, bounds, cu = _packed(dt, hd, Gk)
    kc = torch.full((CACHE_ROWS, Gk, TMAX, hd), float("nan"), device=DEV, dtype=dt)
    vc = torch.full((CACHE_ROWS, Gk, TMAX, hd), float("nan"), device=DEV, dtype=dt)
    kc[:, :, ::3] = 1.5                   # sentinels: NaNs and numbers
    vc[:, :, 1::3] = -2.5
    k0, v0 = kc.clone(), vc.clone()
    ops.kv_cache_fill_varlen(qkv, cu, kc, vc, rows=FILL_ROWS)
    torch.cuda.synchronize()
    k1, v1 = k0.cpu(), v0.cpu()
    ref.kv_cache_fill_varlen(qkv.cpu(), bounds, k1, v1, rows=FILL_ROWS)
    assert _same_bits(kc, k1) and _same_bits(vc, v1)
    # stated on their own: the rows written, the untouched row 1, every position at or beyond a length
    packed = qkv.view(-1, H + 2 * Gk, hd)
    for i, (n, r) in enumerate(zip(FILL_LENS, FILL_ROWS)):
        r0 = bounds[i]
        assert _same_bits(kc[r, :, :n], packed[r0:r0 + n, H:H + Gk].transpose(0, 1)), i
        assert _same_bits(vc[r, :, :n], packed[r0:r0 + n, H + Gk:].transpose(0, 1)), i
        assert _same_bits(kc[r, :, n:], k0[r, :, n:]) and _same_bits(vc[r, :, n:], v0[r, :, n:]), i
    assert _same_bits(kc[1], k0[1]) and _same_bits(vc[1], v0[1])
    # rows = 0..n-1 is rows=None, bit for bit (a cache of exactly n rows)
    a, b = k0[:5].clone(), v0[:5].clone()
    a2, b2 = a.clone(), b.clone()
    ops.kv_cache_fill_varlen(qkv, cu, a, b)
    ops.kv_cache_fill_varlen(qkv, cu, a2, b2, rows=torch.arange(5))
    assert _same_bits(a, a2) and _same_bits(b, b2)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("Gk", [1, 2])
def test_fp8_fill_into_chosen_rows_bitwise(dt, hd, Gk):
    qkv, bounds, cu = _packed(dt, hd, Gk)
    packed = qkv.view(-1, H + 2 * Gk, hd)
    packed[LEAD + 3, H] = 0                                              # an all-zero k row
    packed[LEAD + 5, H + Gk] = 0                                         # an all-zero v row
    packed[LEAD + 40, H, 11] = packed[LEAD + 40, H].abs().max() * 100    # one 100x outlier
    packed[LEAD + 100, H + Gk, 0] = -packed[LEAD + 100, H + Gk].abs().max() * 100

    def fresh(rows):
        return (torch.full((rows, Gk, TMAX, hd), 0x55, dtype=torch.uint8, device=DEV).view(F8),
                torch.full((rows, Gk, TMAX, hd), 0x2A, dtype=torch.uint8, device=DEV).view(F8),
                torch.full((rows, Gk, TMAX), 7.0, device=DEV), torch.full((rows, Gk, TMAX), -7.0, device=DEV))

    def same(a, b):
        return all(torch.equal(_u8(x), _u8(y.to(x.device))) for x, y in zip(a, b))     # bytes, and scale bits

    k8, v8, ks, vs = fresh(CACHE_ROWS)
    want = tuple(t.cpu() for t in (k8, v8, ks, vs))
    ops.kv_cache_fill_varlen(qkv, cu, k8, v8, scales=(ks, vs), rows=FILL_ROWS)
    torch.cuda.synchronize()
    ref.kv_cache_fill_varlen_fp8(qkv.cpu().float(), bounds, *want, rows=FILL_ROWS)
    assert same((k8, v8, ks, vs), want)
    for n, r in zip(FILL_LENS, FILL_ROWS):
        assert (_u8(k8[r, :, n:]) == 0x55).all() and (_u8(v8[r, :, n:]) == 0x2A).all()
        assert (ks[r, :, n:] == 7.0).all() and (vs[r, :, n:] == -7.0).all()
    assert (_u8(k8[1]) == 0x55).all() and (_u8(v8[1]) == 0x2A).all() and (ks[1] == 7.0).all() and (vs[1] == -7.0).all()
    assert float(ks[0, 0, 2]) == 1.0 and float(ks[5, 0, 0]) != 7.0      # packed row LEAD + 3 = (sequence 1 -> row 0, t 2)
    one, two = fresh(5), fresh(5)
    ops.kv_cache_fill_varlen(qkv, cu, one[0], one[1], scales=one[2:])
    ops.kv_cache_fill_varlen(qkv, cu, two[0], two[1], scales=two[2:], rows=[0, 1, 2, 3, 4])
    assert same(one, two)


@pytest.mark.parametrize("fp8", [False, True])
def test_a_row_outside_the_cache_stores_nothing(fp8):
    """The host wrapper never lets such a row through; handed straight to the binding, its threads
    return without storing (release build) while the in-range sequences are filled.  The cache is
    the middle of a larger allocation, whose margins must keep their sentinels too."""
    hd, Gk = 64, 1
    qkv, bounds, cu = _packed(BF16, hd, Gk)
    for bad in (CACHE_ROWS, -1):
        rows = torch.tensor([bad, 0, 3, 2, 4], dtype=torch.int32, device=DEV)
        if fp8:
            big = (torch.full((8, Gk, TMAX, hd), 0x55, dtype=torch.uint8, device=DEV).view(F8),
                   torch.full((8, Gk, TMAX, hd), 0x2A, dtype=torch.uint8, device=DEV).view(F8),
                   torch.full((8, Gk, TMAX), 7.0, device=DEV), torch.full((8, Gk, TMAX), -7.0, device=DEV))
            k8, v8, ks, vs = (t[1:7] for t in big)
            want = tuple(t.cpu().clone() for t in big)
            torch.ops.bllm.kv_cache_fill_varlen_fp8(qkv, cu, k8, ks, v8, vs, rows)
            ref.kv_cache_fill_varlen_fp8(qkv.cpu().float(), bounds[1:], *(t[1:7] for t in want), rows=[0, 3, 2, 4])
        else:
            big = (torch.full((8, Gk, TMAX, hd), 1.5, device=DEV, dtype=BF16),
                   torch.full((8, Gk, TMAX, hd), -2.5, device=DEV, dtype=BF16))
            want = tuple(t.cpu().clone() for t in big)
            torch.ops.bllm.kv_cache_fill_varlen(qkv, cu, big[0][1:7], big[1][1:7], rows)
            ref.kv_cache_fill_varlen(qkv.cpu(), bounds[1:], want[0][1:7], want[1][1:7], rows=[0, 3, 2, 4])
        torch.cuda.synchronize()
        assert all(torch.equal(_u8(a), _u8(b.to(DEV))) for a, b in zip(big, want)), bad
        # the debug build also records the check (and taking the word resets it)
        assert torch.ops.bllm.debug_error() == (3 if torch.ops.bllm.kernel_debug_build() else 0)


DEBUG_CHILD = r"""
import torch
from building_llm_from_scratch_amd import ops
ops.load_ext(required=True)
assert torch.ops.bllm.kernel_debug_build()
dev = "cuda"
qkv = torch.randn(5, 3 * 64, device=dev).bfloat16()
cu = torch.tensor([0, 2, 5], dtype=torch.int32, device=dev)
big = [torch.full((5, 1, 8, 64), v, device=dev, dtype=torch.bfloat16) for v in (1.5, -2.5)]
ops.kv_cache_fill_varlen(qkv, cu, big[0][1:4], big[1][1:4], rows=[2, 0])
assert torch.ops.bllm.debug_error() == 0
rows = torch.tensor([3, 1], dtype=torch.int32, device=dev)       # row 3 of a 3-row cache: past the host check
try:
    ops._k().kv_cache_fill_varlen(qkv, cu, big[0][1:4], big[1][1:4], rows)
    raise SystemExit("fill: no error")
except RuntimeError as e:
    assert "decode cache position" in str(e), e
assert bool((big[0][0] == 1.5).all()) and bool((big[0][4] == 1.5).all()) and bool((big[1][4] == -2.5).all())
assert bool((big[0][2, 0, :3] == qkv.view(5, 3, 64)[2:, 1]).all())     # the in-range sequence was filled
q8 = [torch.zeros(5, 1, 8, 64, device=dev).to(torch.float8_e4m3fn) for _ in range(2)]
sc = [torch.full((5, 1, 8), 7.0, device=dev) for _ in range(2)]
try:
    ops._k().kv_cache_fill_varlen_fp8(qkv, cu, q8[0][1:4], sc[0][1:4], q8[1][1:4], sc[1][1:4], rows)
    raise SystemExit("fp8 fill: no error")
except RuntimeError as e:
    assert "decode cache position" in str(e), e
assert bool((sc[0][0] == 7.0).all()) and bool((sc[0][4] == 7.0).all()) and bool((sc[0][2, 0, :3] != 7.0).all())
ops.kv_cache_fill_varlen(qkv, cu, big[0][1:4], big[1][1:4], rows=[1, 2])        # the word was reset
print("DEBUG-MODE-OK")
"""


def test_kernel_debug_build_reports_a_row_outside_the_cache():
    """As tests/test_sampler_gpu.py: the debug build in a child process.  The kernels record the
    check and return before the store, so the debug run writes nothing out of bounds either."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.isfile(os.path.join(root, "building_llm_from_scratch_amd", "_C_debug.so"))
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=dict(os.environ, BLLM_KERNEL_DEBUG="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEBUG-MODE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ binding refusals
def test_binding_refusals_of_rows():
    Hq, Gk, hd, T = 1, 1, 64, 8
    packed = torch.randn(6, (Hq + 2 * Gk) * hd, device=DEV).to(BF16)
    cu = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    rows = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    kc, vc = (torch.zeros(3, Gk, T, hd, device=DEV, dtype=BF16) for _ in range(2))
    bad_rows = (rows.to(torch.int64), rows.cpu(), torch.cat([rows, rows[:1] + 1]), rows[:1].clone(), _strided(rows),
                rows.view(1, 2), torch.arange(4, dtype=torch.int32, device=DEV))
    fargs = (packed, cu, kc, vc, rows)
    torch.ops.bllm.kv_cache_fill_varlen(*fargs)
    k1, v1 = torch.zeros(3, Gk, T, hd, dtype=BF16), torch.zeros(3, Gk, T, hd, dtype=BF16)
    ref.kv_cache_fill_varlen(packed.cpu(), [0, 2, 6], k1, v1, rows=[2, 0])
    assert _same_bits(kc, k1) and _same_bits(vc, v1)
    _refusals("kv_cache_fill_varlen", fargs, [(4, b) for b in bad_rows] + [(1, torch.cat([cu, cu[-1:]]))])
    k8, v8 = (torch.zeros(3, Gk, T, hd, device=DEV).to(F8) for _ in range(2))
    ks, vs = (torch.zeros(3, Gk, T, device=DEV) for _ in range(2))
    qargs = (packed, cu, k8, ks, v8, vs, rows)
    torch.ops.bllm.kv_cache_fill_varlen_fp8(*qargs)
    want = (torch.zeros(3, Gk, T, hd).to(F8), torch.zeros(3, Gk, T, hd).to(F8), torch.zeros(3, Gk, T), torch.zeros(3, Gk, T))
    ref.kv_cache_fill_varlen_fp8(packed.cpu().float(), [0, 2, 6], *want, rows=[2, 0])
    assert all(torch.equal(_u8(a), _u8(b.to(DEV))) for a, b in zip((k8, v8, ks, vs), want))
    _refusals("kv_cache_fill_varlen_fp8", qargs, [(6, b) for b in bad_rows] + [(1, torch.cat([cu, cu[-1:]]))])


# ------------------------------------------------------------------ admission into a live cache, model level
LEN_A, LEN_B, LEN_C, STEPS = 7, 40, 13, 6


def _tokens(vocab):
    g = torch.Generator().manual_seed(5)
    return (torch.randint(0, vocab, (LEN_A + 2 * STEPS,), generator=g), torch.randint(0, vocab, (LEN_B + STEPS,), generator=g),
            torch.randint(0, vocab, (LEN_C + STEPS,), generator=g))


def _slot_reuse(m, device, kv_dtype=None, graph=False):
    """3 slots, context 64: A (7 tokens) into slot 2 and B (40) into slot 0 in one prefill, 6
    teacher-forced steps, C (13) into slot 0 over the 46 positions B left, 6 more steps; slot 1 stays
    parked.  Returns the logits rows of the live slots in a fixed order, [2 + 12 + 1 + 12, V]."""
    a, b, c = _tokens(m.cfg.vocab_size)
    cache = m.new_kv_cache(3, 64, kv_dtype=kv_dtype)
    got = []
    with torch.no_grad():
        idx, seq = pack_prompts([a[:LEN_A], b[:LEN_B]], device)
        got.append(m.forward_prefill_ragged(idx, seq, cache, rows=[2, 0]).clone())
        pos = torch.tensor([LEN_B, 0, LEN_A], dtype=torch.int32, device=device)
        dec = G.RowsDecodeGraph(m, cache, pos, device) if graph else None
        pos = dec.pos if graph else pos

        def step(tok):
            tok = tok[:, None].to(device)
            if graph:
                return dec.step(tok)
            lg = m.forward_cached_rows(tok, cache, pos)
            pos.add_(1)
            return lg

        for s in range(STEPS):
            got.append(step(torch.stack([b[LEN_B + s], torch.tensor(0), a[LEN_A + s]]))[[0, 2]].clone())
        idx, seq = pack_prompts([c[:LEN_C]], device)
        got.append(m.forward_prefill_ragged(idx, seq, cache, rows=[0]).clone())
        pos[0] = LEN_C
        pos[1] = 0                                  # the parked slot restarts, as the loop's step 5 does
        for s in range(STEPS):
            got.append(step(torch.stack([c[LEN_C + s], torch.tensor(0), a[LEN_A + STEPS + s]]))[[0, 2]].clone())
    return torch.cat(got)


def _slot_reuse_reference(cpu):
    a, b, c = _tokens(cpu.cfg.vocab_size)
    with torch.no_grad():
        fa, fb, fc = (cpu(t[None])[0] for t in (a, b, c))
    rows = [fa[LEN_A - 1], fb[LEN_B - 1]]
    for s in range(STEPS):
        rows += [fb[LEN_B + s], fa[LEN_A + s]]
    rows.append(fc[LEN_C - 1])
    for s in range(STEPS):
        rows += [fc[LEN_C + s], fa[LEN_A + STEPS + s]]
    return torch.stack(rows)


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_model_slot_reuse_against_the_cpu_forward(name):
    gpu, cpu = _pair(name)
    want = _slot_reuse_reference(cpu)
    eager = _slot_reuse(gpu, DEV)
    check_close(eager, want, BF16, k=K_MODEL, name=f"{name} slot reuse")
    replay = _slot_reuse(gpu, DEV, graph=True)
    assert _same_bits(eager, replay)                   # one graph, captured before the second admission


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_model_slot_reuse_on_the_fp8_cache(name):
    """As ``test_kv_fp8_gpu.py::test_model_row_steps_on_the_fp8_cache`` compares, within its bound:
    E_q = the CPU fp32 model's relative logits difference between the fp8 and the exact cache; the
    GPU on the fp8 cache may differ from the CPU on the fp8 cache (through the oracles) by at most
    2 * max(2e-2, E_q).  The prefill rows are left out of both, as there: they never read the cache."""
    gpu, cpu = _pair(name)
    decode = torch.ones(2 + 4 * STEPS + 1, dtype=torch.bool)
    decode[[0, 1, 2 + 2 * STEPS]] = False
    exact = _slot_reuse_reference(cpu)[decode]
    want = _slot_reuse(cpu, "cpu", kv_dtype="fp8")[decode]
    got = _slot_reuse(gpu, DEV, kv_dtype="fp8")
    replay = _slot_reuse(gpu, DEV, kv_dtype="fp8", graph=True)
    assert torch.isfinite(got.float()).all() and torch.equal(got, replay)
    e_q, err = _rel(want, exact), _rel(got[decode], want)
    bound = 2 * max(2e-2, e_q)
    print(f"{name}: E_q {e_q:.3e}  gpu-vs-cpu {err:.3e}  bound {bound:.3e}")
    assert e_q > 0.0 and err <= bound, (e_q, err, bound)


# ------------------------------------------------------------------ generate_continuous end to end
def _prompts(vocab, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g) for n in C.LENS]


@pytest.mark.parametrize("opt", [{}, dict(kv_dtype="fp8"), dict(weight_dtype="fp8")], ids=["bf16", "kv_fp8", "w_fp8"])
@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_continuous_graph_equals_eager(name, opt, monkeypatch):
    gpu, _ = _pair(name)
    prompts = _prompts(gpu.cfg.vocab_size)
    sim = C.simulate([None] * 9, C.BUDGETS, 3, G.EOS_CHECK_EVERY, False)
    runs = {}
    for tag, flag in (("graph", "1"), ("graph again", "1"), ("eager", "0")):
        monkeypatch.setenv("BLLM_DECODE_GRAPH", flag)
        stats = {}
        runs[tag] = G.generate_continuous(gpu, prompts, C.BUDGETS, 64, 3, stats=stats, **opt)
        assert C.stats_match(stats, sim), (tag, stats, sim)
        assert stats["prefills"] >= 2 and max(stats["slot"].count(s) for s in range(3)) >= 2
    for p, n, a, b, c in zip(prompts, C.BUDGETS, runs["graph"], runs["graph again"], runs["eager"]):
        assert a.numel() == p.numel() + n and torch.equal(a[:p.numel()].cpu(), p)
        assert torch.equal(a, b) and torch.equal(a, c)


def test_generate_continuous_fp32_equals_one_row_runs():
    """The fp32 GPU path (oracle decode, no graph), as
    ``test_generate_ragged_fp32_takes_the_oracle_decode_path``: the answers equal the one-row
    ``generate_cached`` runs cut to the budgets, under its premise, asserted first: no one-row step
    has a runner-up within 1e-4 of its argmax (GEMM rounding between batch shapes is about 2e-6)."""
    cfg = _cfgs()["llama"].replace(dtype=F32)
    torch.manual_seed(0)
    m = build_model(cfg, device=DEV)
    m.flatten()
    m.eval()
    assert not m.decode_graph_ok(m.new_kv_cache(1, 64))
    prompts = _prompts(cfg.vocab_size)
    ones = [G.generate_cached(m, p[None], C.NEW, 64)[0] for p in prompts]
    with torch.no_grad():
        for p, o in zip(prompts, ones):
            top = m(o[None])[0, p.numel() - 1:-1].float().topk(2, dim=-1).values
            gap = float((top[:, 0] - top[:, 1]).min())
            print(f"prompt of {p.numel()}: smallest gap {gap:.3e}")
            assert gap > 1e-4
    stats = {}
    res = G.generate_continuous(m, prompts, C.BUDGETS, 64, 3, stats=stats)
    for o, r, p, n in zip(ones, res, prompts, C.BUDGETS):
        assert torch.equal(r, o[:p.numel() + n])
    assert C.stats_match(stats, C.simulate([None] * 9, C.BUDGETS, 3, G.EOS_CHECK_EVERY, False))


def test_a_slot_index_does_not_change_the_answer():
    """With ``weight_dtype="fp8"`` the decode projections are bitwise independent of the other rows
    (and so is per-row attention), so only the admission prefill could tell arrangements apart.
    P is admitted alone in its round each time -- after a budget-1 prompt freed slot 2, after one
    freed slot 0, and into slot 0 of an otherwise empty cache -- and draws the same tokens."""
    gpu, _ = _pair("llama")
    ps = _prompts(gpu.cfg.vocab_size)
    p, x, y, z = ps[3], ps[1], ps[6], ps[8]
    runs = []
    for prompts, budgets, slot in (([x, y, z, p], [9, 9, 1, 12], 2), ([x, y, z, p], [1, 9, 9, 12], 0), ([p], [12], 0)):
        stats = {}
        res = G.generate_continuous(gpu, prompts, budgets, 64, 3, weight_dtype="fp8", stats=stats)
        assert stats["slot"][-1] == slot and stats["prefills"] == (2 if len(prompts) > 1 else 1)
        runs.append(res[-1])
    assert runs[0].numel() == p.numel() + 12
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
