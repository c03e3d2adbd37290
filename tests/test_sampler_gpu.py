"""The token sampler kernel (csrc/sample.hip) on the GPU against its fp64 oracle
(``ops.reference.sample_rows_detail``): tokens and thresholds over dtypes, vocabulary sizes, batch
sizes, filters and temperatures; special rows; row isolation, determinism and guard rows; the
distribution of its draws; graph replay; the binding's checks; and ``generate_ragged`` /
``generate_cached`` with ``seed=...`` on the tiny models of tests/test_generate_ragged_gpu.py.

Adjudication.  A draw is a NEAR TIE when the oracle's winning gap (top Gumbel key minus the
runner-up) is below ``tol = 2^-20 * max(1, max|key|)``, about 8 fp32 ulp: one rounding of l / T, two
1-ulp logs and the subtraction.  On a near tie the kernel's token must have an oracle key within
``tol`` of the maximum; otherwise it must be the oracle's token.  At most 1 % of a test's draws may
be near ties (the gap is of order 1, so the expected share is ~1e-5).  TOP-P: the kernel sums the
masses in 2^-40 fixed point (absolute error < 2^-23 of the total) over a 1-ulp expf, the oracle in
fp64; the inputs are chosen, and asserted from the oracle's detail, so that no cumulative-mass
ratio at a group boundary lies within 1e-5 relative of ``top_p``, ten times that error.  With it
``thr`` must equal the oracle's threshold exactly."""
import os
import subprocess
import sys

import pytest
import torch

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

from test_generate_ragged_gpu import _cfgs, _pair, _refusals, _strided
from test_sampler_cpu import check_calls, chi2_case, recorded, _chi2_bound  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NINF = float("-inf")
SEED = 20240607
VS = [1, 5, 63, 64, 65, 257, 1000, 32000, 50257, 128256]
BS = [1, 3, 8]
FILTERS = [(0, 1.0), (1, 1.0), (5, 1.0), (50, 0.9), (0, 0.5), ("V+1", 1.0)]


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


def case_logits(dt, V):
    """[8, V] logits with the spread of a language model's (std 4: the mass sits on a few dozen
    tokens, so cumulative-mass ratios are far apart where top-p cuts) and, in 16 bits, many ties."""
    # + 30: a seed family under which every case meets the top-p precondition (case_oracle)
    g = torch.Generator().manual_seed(1000 * V + {BF16: 1, F16: 2, F32: 3}[dt] + 30)
    return (4.0 * torch.randn(8, V, generator=g)).to(dt)


def case_streams(B=8):
    return torch.tensor([3, 2 ** 40 + 1, 0, 17, 2 ** 62, 5, 99, 12345][:B], dtype=torch.long)


def case_oracle(l, T, top_k, top_p, ctr0):
    """Oracle tokens, thresholds and details of the 8 rows, with the top-p precondition asserted."""
    B = l.shape[0]
    tok, thr, det = ref.sample_rows_detail(l, case_streams(B), torch.full((B,), ctr0, dtype=torch.int32), SEED, T,
                                           top_k, top_p)
    if T > 0 and top_p < 1.0:
        for b, d in enumerate(det):
            r = d["ratios"]
            assert float(((r - top_p).abs() / top_p).min()) > 1e-5, (b, "a mass ratio sits on top_p: pick other inputs")
    return tok, thr, det


def adjudicate(got, want, det):
    """-> number of near ties; asserts the near-tie rule row by row."""
    near = 0
    for b, d in enumerate(det):
        keys = d["keys"]
        live = keys[keys > NINF]
        tol = 2.0 ** -20 * max(1.0, float(live.abs().max()) if live.numel() else 1.0)
        g = int(got[b])
        assert 0 <= g < keys.numel(), (b, g)
        if d["gap"] < tol:
            near += 1
            assert float(keys.max() - keys[g]) <= tol, (b, g, int(want[b]))
        else:
            assert g == int(want[b]), (b, g, int(want[b]), d["gap"])
    return near


def run_kernel(l, B, T, top_k, top_p, ctr0, **kw):
    ctr = torch.full((B,), ctr0, dtype=torch.int32, device=DEV)
    thr = torch.full((B,), 123.0, device=DEV)
    tok = ops.sample_rows(l[:B].to(DEV).contiguous(), case_streams(B).to(DEV), ctr, SEED, T, top_k, top_p, thr=thr, **kw)
    return tok.cpu(), thr.cpu(), ctr.cpu()


# ------------------------------------------------------------------ kernel vs oracle
@pytest.mark.parametrize("T", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=["bf16", "fp16", "fp32"])
def test_kernel_matches_oracle(dt, V, T):
    l = case_logits(dt, V)
    draws = near = 0
    for fi, (k, p) in enumerate(FILTERS):
        k = V + 1 if k == "V+1" else k
        ctr0 = 7 * fi
        want, wthr, det = case_oracle(l, T, k, p, ctr0)
        for B in BS:
            got, thr, ctr = run_kernel(l, B, T, k, p, ctr0)
            assert ctr.tolist() == [ctr0 + 1] * B
            if T == 0.0:
                assert torch.equal(got, want[:B]), (k, p, B)
                assert bool((thr == 123.0).all())                       # not computed, not written
            else:
                near += adjudicate(got, want[:B], det[:B])
                draws += B
                assert torch.equal(thr.double(), wthr[:B]), (k, p, B, thr, wthr[:B])
    assert near <= 0.01 * draws, (near, draws)


def special_logits(dt, V):
    g = torch.Generator().manual_seed(77)
    l = torch.randn(8, V, generator=g)
    l[0, V - 1] = 9.0                       # the maximum at the last index
    l[1, 0] = 9.0                           # ... and at the first
    l[2] = 1.25                             # all equal
    l[3] = NINF
    l[3, 617] = -3.0                        # one finite entry
    l[4, ::3] = float("nan")                # NaNs among numbers
    l[5] = float("nan")
    l[6] = NINF
    l[7, 5], l[7, 6], l[7, 7] = float("inf"), -0.0, 0.0
    return l.to(dt)


def test_special_rows():
    V = 1000
    for dt in (BF16, F16, F32):
        l = special_logits(dt, V)
        got, _, _ = run_kernel(l, 8, 0.0, 0, 1.0, 0)
        assert got[:4].tolist() == [V - 1, 0, 0, 617] and int(got[6]) == 0 and int(got[7]) == 5
        assert bool(((got >= 0) & (got < V)).all())
        want = ref.sample_rows_detail(l, case_streams(), torch.zeros(8, dtype=torch.int32), SEED, 0.0)[0]
        assert torch.equal(got, want)
        for k, p in [(0, 1.0), (5, 1.0), (V, 0.9), (3, 0.5)]:
            for c in range(4):
                want, wthr, det = case_oracle(l[:4], 1.0, k, p, c)
                got, thr, _ = run_kernel(l, 8, 1.0, k, p, c)
                assert bool(((got >= 0) & (got < V)).all())             # NaN rows included
                adjudicate(got[:4], want, det)
                assert torch.equal(thr[:4].double(), wthr)
                assert int(got[3]) == 617 and int(got[6]) == 0
                assert not bool(torch.isnan(l[4, int(got[4])])) and int(got[7]) in range(V)
                if (k, p) == (5, 1.0):
                    assert float(thr[2]) == 1.25                        # ties at the threshold: all of the row is kept
        # an all-equal row is a uniform draw: the tokens move with the counter
        toks = {int(run_kernel(l, 3, 1.0, 7, 1.0, c)[0][2]) for c in range(16)}
        assert len(toks) > 8


@pytest.mark.parametrize("V", [50257, 1000])
def test_rows_are_isolated_deterministic_and_stay_in_their_buffers(V):
    l = case_logits(BF16, V).to(DEV)
    streams, B, cols, eos = case_streams().to(DEV), 8, 6, None
    first = None
    for run in range(2):
        # guard rows: each buffer is the middle of a larger one
        big = {"ctr": torch.full((B + 2,), 3, dtype=torch.int32, device=DEV),
               "next": torch.full((B + 2,), -7, dtype=torch.long, device=DEV),
               "out": torch.full((B + 2, cols), -7, dtype=torch.long, device=DEV),
               "fin": torch.zeros(B + 2, dtype=torch.bool, device=DEV),
               "thr": torch.full((B + 2,), 55.0, device=DEV)}
        ctr, nxt, out, fin, thr = (big[k][1:B + 1] for k in ("ctr", "next", "out", "fin", "thr"))
        tok = ops.sample_rows(l, streams, ctr, SEED, 0.9, 40, 0.95, eos_id=-1, next_idx=nxt, out=out, finished=fin,
                              thr=thr)
        eos = int(tok[2])
        tok2 = ops.sample_rows(l, streams, ctr, SEED, 0.9, 40, 0.95, eos_id=eos, next_idx=nxt, out=out, finished=fin,
                               thr=thr)
        state = [t.cpu().clone() for t in (tok, tok2, big["ctr"], big["next"], big["out"], big["fin"], big["thr"])]
        if first is None:
            first = state
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, state))                # run to run
    tok, tok2, ctr, nxt, out, fin, thr = first
    assert ctr.tolist() == [3] + [5] * B + [3]                                           # advanced by one per call
    assert nxt.tolist() == [-7] + tok2.tolist() + [-7]
    want_out = torch.full((B + 2, cols), -7, dtype=torch.long)
    want_out[1:B + 1, 3], want_out[1:B + 1, 4] = tok, tok2
    assert torch.equal(out, want_out)
    assert fin.tolist() == [False] + (tok2 == eos).tolist() + [False]
    assert float(thr[0]) == 55.0 and float(thr[-1]) == 55.0 and bool((thr[1:-1] < 55.0).all())
    # row b alone: the same logits, stream and counter give the same token and threshold
    for b in range(B):
        c1 = torch.full((1,), 4, dtype=torch.int32, device=DEV)
        t1 = torch.zeros(1, device=DEV)
        one = ops.sample_rows(l[b:b + 1], streams[b:b + 1], c1, SEED, 0.9, 40, 0.95, thr=t1)
        assert int(one[0]) == int(tok2[b]) and float(t1[0]) == float(thr[1 + b]) and int(c1[0]) == 5, b
    # a counter past the last column writes the last column, nothing outside
    small = torch.full((B + 2, 2), -7, dtype=torch.long, device=DEV)
    late = torch.full((B,), 9, dtype=torch.int32, device=DEV)
    tok3 = ops.sample_rows(l, streams, late, SEED, 0.9, 40, 0.95, out=small[1:B + 1])
    assert bool((small[1:B + 1, 1].cpu() == tok3.cpu()).all()) and int((small == -7).sum()) == 2 * (B + 2) - B


def test_out_may_be_a_column_range_of_a_wider_buffer():
    l = case_logits(F16, 257).to(DEV)
    wide = torch.full((8, 10), -7, dtype=torch.long, device=DEV)
    ctr = torch.zeros(8, dtype=torch.int32, device=DEV)
    toks = [ops.sample_rows(l, case_streams().to(DEV), ctr, SEED, 1.0, out=wide[:, 4:7]) for _ in range(3)]
    assert torch.equal(wide[:, 4:7], torch.stack(toks, dim=1)) and int((wide == -7).sum()) == 8 * 7


# ------------------------------------------------------------------ distribution
@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 1.0), (1.0, 10, 1.0), (1.0, 0, 0.8), (0.5, 0, 1.0), (2.0, 0, 1.0)])
def test_device_draws_follow_the_softmax_of_the_kept_set(T, top_k, top_p):
    stat, bound, _ = chi2_case(lambda *a: ops.sample_rows(*a), T=T, top_k=top_k, top_p=top_p, device=DEV)
    print(f"T={T} top_k={top_k} top_p={top_p}: chi2 {stat:.1f} bound {bound:.1f}")
    assert stat < bound


def test_device_draws_over_a_200_token_kept_set_of_a_real_vocabulary():
    """V = 50,257, 200 tokens spread over the row at linspace(-2, 2) (as rounded to bf16), the rest
    30 below: top_k = 200 keeps exactly those.  8 streams x 4,096 counters = 32,768 draws, recorded
    on the device through ``out``."""
    V, K, B, N = 50257, 200, 8, 4096
    where = torch.arange(K) * 251 + 3
    row = torch.full((V,), -30.0)
    row[where] = torch.linspace(-2, 2, K)
    l = row.to(BF16)[None].repeat(B, 1).to(DEV)
    out = torch.zeros(B, N, dtype=torch.long, device=DEV)
    ctr = torch.zeros(B, dtype=torch.int32, device=DEV)
    streams = case_streams().to(DEV)
    for _ in range(N):
        ops.sample_rows(l, streams, ctr, SEED, 1.0, K, 1.0, out=out)
    counts = torch.bincount(out.cpu().flatten(), minlength=V).double()
    assert int(counts[where].sum()) == B * N
    e = torch.softmax(row.to(BF16).double()[where], dim=0) * B * N
    stat, bound = float(((counts[where] - e) ** 2 / e).sum()), _chi2_bound(K - 1)
    print(f"chi2 {stat:.1f} bound {bound:.1f} smallest expected count {float(e.min()):.1f}")
    assert stat < bound


# ------------------------------------------------------------------ graph replay
def test_graph_replay_equals_eager_calls():
    V, B, N = 32000, 3, 20
    l = case_logits(BF16, V)[:B].to(DEV)
    streams = case_streams(B).to(DEV)

    def state():
        return dict(ctr=torch.zeros(B, dtype=torch.int32, device=DEV), next_idx=torch.zeros(B, 1, dtype=torch.long, device=DEV),
                    out=torch.zeros(B, N, dtype=torch.long, device=DEV), finished=torch.zeros(B, dtype=torch.bool, device=DEV))

    def call(s):
        return ops.sample_rows(l, streams, s["ctr"], SEED, 1.0, 50, 0.9, eos_id=eos, next_idx=s["next_idx"], out=s["out"],
                               finished=s["finished"])
    eos = -1
    e = state()
    eos = int(call(e)[1])                    # a token that does occur: row 1's first
    e = state()
    eager = torch.stack([call(e) for _ in range(N)], dim=1)
    g = state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tok = call(g)
    replayed = []
    for _ in range(N):
        graph.replay()
        replayed.append(tok.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(replayed, dim=1), eager)
    for k in e:
        assert torch.equal(e[k], g[k]), k
    assert e["ctr"].tolist() == [N] * B and torch.equal(e["out"], eager) and bool(e["finished"][1])


# ------------------------------------------------------------------ binding
def _binding_args(B, V):
    return (torch.zeros(B, V, dtype=BF16, device=DEV), torch.zeros(B, dtype=torch.long, device=DEV),
            torch.zeros(B, dtype=torch.int32, device=DEV), 0, 1.0, 0, 1.0, -1,
            torch.zeros(B, dtype=torch.long, device=DEV), torch.zeros(B, 1, dtype=torch.long, device=DEV),
            torch.zeros(B, dtype=torch.bool, device=DEV), torch.zeros(B, device=DEV))


def test_binding_checks():
    """In the style of tests/test_binding_checks_gpu.py: the smallest accepted call, then one refused
    call per check with one argument changed in the safe direction (longer, another dtype, strided
    inside a larger allocation, on the host, an extra or a missing dimension)."""
    args = _binding_args(1, 1)
    assert torch.ops.bllm.sample_rows(*args).tolist() == [0] and args[2].tolist() == [1]
    assert torch.ops.bllm.sample_rows(*args[:8], None, None, None, None).tolist() == [0]
    args = _binding_args(2, 4)
    assert torch.ops.bllm.sample_rows(*args).shape == (2,)
    l, st, ctr, nxt, out, fin, thr = args[0], args[1], args[2], args[8], args[9], args[10], args[11]
    lng = lambda t: torch.cat([t, t[:1]])
    _refusals("sample_rows", args, (
        (0, _strided(l)), (0, l.to(torch.int32)), (0, l.unsqueeze(0)), (0, l.cpu()), (0, l[:, :0]),
        (1, lng(st)), (1, st.to(torch.int32)), (1, _strided(st)), (1, st.cpu()),
        (2, lng(ctr)), (2, ctr.to(torch.long)), (2, _strided(ctr)), (2, ctr.cpu()),
        (4, -1.0), (4, float("nan")), (5, -1), (6, 0.0), (6, 1.5), (6, float("nan")),
        (8, lng(nxt)), (8, nxt.to(torch.int32)), (8, _strided(nxt)), (8, nxt.cpu()),
        (9, lng(out)), (9, out.to(torch.int32)), (9, out[:, 0]), (9, out[:, :0]), (9, out.cpu()), (9, out.unsqueeze(0)),
        (9, torch.zeros(2, 2, 2, dtype=torch.long, device=DEV)[:, :, 0]),                     # column stride 2
        (9, torch.zeros(8, dtype=torch.long, device=DEV).as_strided((2, 4), (2, 1))),         # overlapping rows
        (10, lng(fin)), (10, fin.to(torch.uint8)), (10, _strided(fin)), (10, fin.cpu()),
        (11, lng(thr)), (11, thr.to(F16)), (11, _strided(thr)), (11, thr.cpu()),
    ))


DEBUG_CHILD = r"""
import torch
from building_llm_from_scratch_amd import ops
ops.load_ext(required=True)
assert torch.ops.bllm.kernel_debug_build()
dev = "cuda"
l = torch.randn(3, 300, device=dev).bfloat16()
st = torch.arange(3, device=dev)
guard = torch.full((5, 2), -7, dtype=torch.long, device=dev)
ctr = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
ops.sample_rows(l, st, ctr, 1, 1.0, out=guard[1:4])
try:
    ops.sample_rows(l, st, ctr, 1, 1.0, out=guard[1:4])          # rows 1 and 2 are at column 2 of 2
    raise SystemExit("sampler: no error")
except RuntimeError as e:
    assert "sampler row counter" in str(e), e
assert bool((guard[0] == -7).all()) and bool((guard[4] == -7).all())   # the column was clamped
ops.sample_rows(l, st, torch.zeros(3, dtype=torch.int32, device=dev), 1, 1.0, out=guard[1:4])   # the word was reset
print("DEBUG-MODE-OK")
"""


def test_kernel_debug_build_reports_a_counter_outside_out():
    """As tests/test_kernel_debug_gpu.py: the debug build in a child process (the two builds register
    the same op library).  The kernel clamps the column after recording the check, so the debug run
    writes nothing out of bounds."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.isfile(os.path.join(root, "building_llm_from_scratch_amd", "_C_debug.so"))
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=dict(os.environ, BLLM_KERNEL_DEBUG="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEBUG-MODE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ model level
def _prompts(vocab):
    g = torch.Generator().manual_seed(7)
    return [torch.randint(0, vocab, (n,), generator=g) for n in [1, 7, 40, 13]]


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_ragged_seeded_graph_equals_eager(name, monkeypatch):
    """Same process, same shapes, same kernels: the captured forward + sampler step gives the eager
    calls' tokens, run to run (as the greedy test of tests/test_generate_ragged_gpu.py argues)."""
    gpu, _ = _pair(name)
    prompts = _prompts(gpu.cfg.vocab_size)
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, seed=11, streams=[4, 9, 2, 7])
    runs = {}
    for tag, flag in (("graph", "1"), ("graph again", "1"), ("eager", "0")):
        monkeypatch.setenv("BLLM_DECODE_GRAPH", flag)
        runs[tag] = G.generate_ragged(gpu, prompts, 24, 64, **kw)
    for p, a, b, c in zip(prompts, runs["graph"], runs["graph again"], runs["eager"]):
        assert a.numel() == p.numel() + 24 and torch.equal(a[:p.numel()].cpu(), p)
        assert torch.equal(a, b) and torch.equal(a, c)
    other = G.generate_ragged(gpu, prompts, 24, 64, **{**kw, "seed": 12})
    assert any(not torch.equal(a, o) for a, o in zip(runs["graph"], other))
    # eos: each row is cut before its own
    eos = int(runs["graph"][0][prompts[0].numel() + 2])
    cut = G.generate_ragged(gpu, prompts, 24, 64, eos_id=eos, **kw)
    for p, a, c in zip(prompts, runs["graph"], cut):
        gen = a[p.numel():]
        hit = (gen == eos).nonzero()
        assert torch.equal(c, a[:p.numel() + int(hit[0])] if hit.numel() else a)


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_ragged_eager_calls_are_the_oracles(name, monkeypatch, recorded):  # noqa: F811
    monkeypatch.setenv("BLLM_DECODE_GRAPH", "0")
    gpu, _ = _pair(name)
    prompts = _prompts(gpu.cfg.vocab_size)
    res = G.generate_ragged(gpu, prompts, 12, 64, temperature=0.8, top_k=50, top_p=0.9, seed=11, streams=[4, 9, 2, 7])
    assert len(recorded) == 12
    check_calls(recorded, [4, 9, 2, 7], 11, 0.8, 50, 0.9)
    for b, (r, p) in enumerate(zip(res, prompts)):
        assert torch.equal(r.cpu(), torch.cat((p, torch.stack([c["tokens"][b] for c in recorded]).cpu())))


def test_generate_cached_seeded_on_the_gpu(recorded):  # noqa: F811
    gpu, _ = _pair("llama")
    idx = torch.stack([p[:7] for p in _prompts(gpu.cfg.vocab_size)[1:3]])
    out = G.generate_cached(gpu, idx, 20, 16, temperature=0.9, top_p=0.95, seed=4, streams=[11, 12])   # slides
    assert len(recorded) == 20 and out.shape == (2, 27)
    check_calls(recorded, [11, 12], 4, 0.9, 0, 0.95)
    assert torch.equal(out[:, 7:], torch.stack([c["tokens"] for c in recorded], dim=1))
    assert torch.equal(out, G.generate_cached(gpu, idx, 20, 16, temperature=0.9, top_p=0.95, seed=4, streams=[11, 12]))


def test_generate_ragged_seeded_fp32_model_runs_eagerly(recorded):  # noqa: F811
    cfg = _cfgs()["llama"].replace(dtype=F32)
    torch.manual_seed(0)
    m = build_model(cfg, device=DEV)
    m.flatten()
    m.eval()
    assert not m.decode_graph_ok(m.new_kv_cache(1, 64))
    prompts = _prompts(cfg.vocab_size)
    res = G.generate_ragged(m, prompts, 12, 64, temperature=1.0, top_k=20, seed=3)
    assert len(recorded) == 12 and recorded[0]["logits"].dtype == F32 and recorded[0]["logits"].is_cuda
    check_calls(recorded, [0, 1, 2, 3], 3, 1.0, 20, 1.0)
    assert all(r.numel() == p.numel() + 12 for r, p in zip(res, prompts))
