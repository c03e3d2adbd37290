"""Speculative decoding on the GPU: ``attn_extend_rows`` (Q tokens per row over the cache) and
``spec_advance`` against their oracles, their binding checks, the Q-token model step against the
CPU fp32 full forward, ``SpecDecodeGraph`` against the eager step, and
``generate_ragged(speculative=K)``."""
import os
import subprocess
import sys

import pytest
import torch
from numerics import check_close

import speculative_cases as S
from test_generate_ragged_gpu import (BF16, DEV, F16, F32, K_DECODE, K_MODEL, _cfgs, _f, _pair, _refusals, _rnd,
                                      _same_bits, _strided)

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.models.base import pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


# ------------------------------------------------------------------ attn_extend_rows
TMAX = 320


def _positions(Q):
    # the first key, one cached key, a wave edge, the 256-key chunk edge crossed inside the Q
    # tokens, the cache's last slots
    return [0, 1, 64 - Q + 1, 256 - Q // 2, TMAX - Q]


def _case(dt, hd, H, Gk, Q, pos, tmax=TMAX):
    B = len(pos)
    qkv = _rnd(B * Q, (H + 2 * Gk) * hd, dt=dt)
    kc, vc = _rnd(B, Gk, tmax, hd, dt=dt), _rnd(B, Gk, tmax, hd, dt=dt)
    for b, p in enumerate(pos):          # rows >= pos[b] must not be read: NaN
        kc[b, :, p:] = float("nan")
        vc[b, :, p:] = float("nan")
    return qkv, kc, vc, torch.tensor(pos, dtype=torch.int32, device=DEV)


def _check_extend(dt, hd, H, Gk, Q, pos, tmax=TMAX):
    qkv, kc, vc, pt = _case(dt, hd, H, Gk, Q, pos, tmax)
    k0, v0 = kc.clone(), vc.clone()
    out = ops.attn_extend_rows(qkv, kc, vc, pt, Q, H, Gk)
    torch.cuda.synchronize()
    assert out.shape == (len(pos) * Q, H * hd) and torch.isfinite(out.float()).all()
    rows = qkv.view(len(pos), Q, H + 2 * Gk, hd)
    for b, p in enumerate(pos):
        assert _same_bits(kc[b, :, p:p + Q], rows[b, :, H:H + Gk].transpose(0, 1)), b
        assert _same_bits(vc[b, :, p:p + Q], rows[b, :, H + Gk:].transpose(0, 1)), b
        other = torch.ones(tmax, dtype=torch.bool, device=DEV)
        other[p:p + Q] = False
        assert _same_bits(kc[b][:, other], k0[b][:, other]), b
        assert _same_bits(vc[b][:, other], v0[b][:, other]), b
    want = ref.attn_extend_rows(_f(qkv), _f(k0), _f(v0), pt.cpu(), Q, H, Gk)
    check_close(out, want, dt, k=K_DECODE, name=f"extend rows Q{Q}")


@pytest.mark.parametrize("Q", [2, 4, 8])
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,Gk", [(4, 4), (8, 2), (4, 1)])
def test_attn_extend_rows(dt, hd, H, Gk, Q):
    _check_extend(dt, hd, H, Gk, Q, _positions(Q))


@pytest.mark.parametrize("dt,hd,H,Gk,Q", [(BF16, 128, 8, 2, 8), (F16, 64, 4, 4, 2), (BF16, 64, 4, 1, 4),
                                          (F16, 128, 4, 1, 8)])
def test_attn_extend_rows_long_cache(dt, hd, H, Gk, Q):
    """33 key chunks: a row near the start (the other chunks' workgroups leave at once), one across
    the 8,192 edge, one in the last slots."""
    _check_extend(dt, hd, H, Gk, Q, [5, 8190, 8448 - Q], tmax=8448)


def test_attn_extend_rows_more_than_32_queries_takes_the_oracle():
    dt, hd, H, Gk, Q = BF16, 64, 8, 1, 8
    qkv, kc, vc, pt = _case(dt, hd, H, Gk, Q, [3, 40])
    k1, v1 = kc.clone(), vc.clone()
    out = ops.attn_extend_rows(qkv, kc, vc, pt, Q, H, Gk)
    want = ref.attn_extend_rows(qkv, k1, v1, pt, Q, H, Gk)
    assert _same_bits(out, want) and _same_bits(kc, k1) and _same_bits(vc, v1)
    with pytest.raises(RuntimeError, match="attn_extend_rows"):
        torch.ops.bllm.attn_extend_rows(qkv, kc, vc, pt, pt.repeat_interleave(Q), Q, H, Gk)


def test_attn_extend_rows_q1_is_attn_decode_append_rows():
    dt, hd, H, Gk = BF16, 128, 8, 2
    qkv, kc, vc, pt = _case(dt, hd, H, Gk, 1, [0, 63, 255, 319])
    k1, v1 = kc.clone(), vc.clone()
    a = ops.attn_extend_rows(qkv, kc, vc, pt, 1, H, Gk)
    b = ops.attn_decode_append_rows(qkv, k1, v1, pt, H, Gk)
    assert _same_bits(a, b) and _same_bits(kc, k1) and _same_bits(vc, v1)


@pytest.mark.parametrize("dt,hd,H,Gk,Q", [(BF16, 128, 8, 2, 4), (F16, 64, 4, 4, 8)])
def test_attn_extend_rows_row_isolation(dt, hd, H, Gk, Q):
    """Each row of a 4-row call equals its own 1-row call, bit for bit, in output and in cache."""
    pos = [2, 70, 255, 300]
    qkv, kc, vc, pt = _case(dt, hd, H, Gk, Q, pos)
    k0, v0 = kc.clone(), vc.clone()
    out = ops.attn_extend_rows(qkv, kc, vc, pt, Q, H, Gk)
    for b in range(len(pos)):
        k1, v1 = k0[b:b + 1].clone(), v0[b:b + 1].clone()
        one = ops.attn_extend_rows(qkv[b * Q:(b + 1) * Q].clone(), k1, v1, pt[b:b + 1].clone(), Q, H, Gk)
        assert _same_bits(out[b * Q:(b + 1) * Q], one), b
        assert _same_bits(kc[b:b + 1], k1) and _same_bits(vc[b:b + 1], v1), b


def test_attn_extend_rows_graph_replay():
    """Captured once; replayed with other positions and qkv rows written into the captured
    tensors: the result is the eager call's, bit for bit."""
    dt, hd, H, Gk, Q = BF16, 128, 8, 2, 4
    qkv, kc, vc, pos = _case(dt, hd, H, Gk, Q, [TMAX - Q] * 4)
    kc.normal_()
    vc.normal_()
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):                       # warm-up outside the capture
        ops.attn_extend_rows(qkv, kc, vc, pos, Q, H, Gk)
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_extend_rows(qkv, kc, vc, pos, Q, H, Gk)
    for new_pos in ([3, 64, 200, 0], [254, 1, 61, TMAX - Q]):
        q2, k2, v2, p2 = _case(dt, hd, H, Gk, Q, new_pos)
        ke, ve = k2.clone(), v2.clone()
        eager = ops.attn_extend_rows(q2, ke, ve, p2, Q, H, Gk)
        qkv.copy_(q2)
        kc.copy_(k2)
        vc.copy_(v2)
        pos.copy_(p2)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, eager) and _same_bits(kc, ke) and _same_bits(vc, ve)


# ------------------------------------------------------------------ spec_advance
def _same_state(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_spec_advance_kernel_on_the_hand_written_rows():
    for name, r in sorted(S.CASES.items()):
        S.check_case(S.run_rows(ops.spec_advance, [r], device=DEV), 0, r)
    rows = [r for _, r in sorted(S.CASES.items()) if not r["accept"]]          # one batch
    st = S.run_rows(ops.spec_advance, rows, device=DEV)
    for b, r in enumerate(rows):
        S.check_case(st, b, r)


@pytest.mark.parametrize("Q,ngram,eos,accept,lh", [(4, 2, 2, True, 4096), (8, 2, -1, True, 700), (2, 1, 0, True, 300),
                                                    (8, 4, 3, True, 4096), (5, 3, -1, False, 1000), (1, 2, 1, True, 64)])
def test_spec_advance_kernel_equals_oracle_on_random_rows(Q, ngram, eos, accept, lh):
    """16 random rows over a 4-letter alphabet (matches everywhere, the scan wraps its 256-thread
    workgroup up to 16 times), drafts that agree with the sampler for a random prefix, counters
    near the answer's end, some rows finished: every state tensor equals the oracle's, exactly."""
    g = torch.Generator().manual_seed(Q * 100 + ngram)
    B, new = 16, 24
    rows = []
    for b in range(B):
        n = int(torch.randint(1, lh - Q - 1, (1,), generator=g)) if b else lh - Q - 1     # row 0: the longest
        h0 = int(torch.randint(0, n, (1,), generator=g))
        hist = torch.randint(0, 4, (n,), generator=g).tolist()
        samp = torch.randint(0, 4, (Q,), generator=g).tolist()
        agree = int(torch.randint(0, Q + 1, (1,), generator=g))
        idx = [hist[-1]] + [samp[j - 1] if j <= agree else (samp[j - 1] + 1) % 4 for j in range(1, Q)]
        rows.append(S.case(idx=idx, samp=samp, hist=hist, h0=h0, pos=n - 1 - h0,
                           ctr=int(torch.randint(1, new, (1,), generator=g)), new=new, want=None, eos=eos, ngram=ngram,
                           finished=b % 5 == 4, accept=accept, lh=lh))
    want = S.run_rows(ref.spec_advance, rows)
    got = S.run_rows(ops.spec_advance, rows, device=DEV)
    assert not _same_state(got, want)
    if accept and Q > 1:
        assert (want["nsteps"] == 1).any() and (want["ctr"] - torch.tensor([r["ctr"] for r in rows]) > 1).any()


def test_spec_binding_refusals():
    H, Gk, hd, T, B, Q = 2, 1, 64, 16, 2, 2
    qkv = _rnd(B * Q, (H + 2 * Gk) * hd, dt=BF16)
    kc, vc = _rnd(B, Gk, T, hd, dt=BF16), _rnd(B, Gk, T, hd, dt=BF16)
    pos = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
    pr = torch.tensor([3, 4, 5, 6], dtype=torch.int32, device=DEV)
    args = (qkv, kc.clone(), vc.clone(), pos, pr, Q, H, Gk)
    out = torch.ops.bllm.attn_extend_rows(*args)
    want = ref.attn_extend_rows(_f(qkv), _f(kc), _f(vc), pos.cpu(), Q, H, Gk)
    check_close(out, want, BF16, k=K_DECODE, name="extend rows")
    _refusals("attn_extend_rows", args, (
        (0, _strided(qkv)), (0, qkv.to(F32)), (0, qkv.unsqueeze(0)), (0, torch.cat([qkv, qkv[:1]])),
        (1, kc.unsqueeze(0)), (1, _strided(kc)), (2, vc.to(F32)), (2, _rnd(B, Gk, T + 1, hd, dt=BF16)),
        (3, torch.cat([pos, pos[:1]])), (3, pos.to(torch.int64)), (3, _strided(pos)),
        (4, torch.cat([pr, pr[:1]])), (4, pr.to(torch.int64)), (4, _strided(pr)),
        (5, 1), (5, 9), (5, 3),                      # Q: below 2, above 8, not the qkv rows' count
    ))
    r = S.CASES["all_accepted"]
    st = S.run_rows(lambda *a: None, [r, r], device=DEV)
    sargs = (st["idx"].to(DEV), st["samp"].to(DEV), st["hist"].to(DEV), st["h0"].to(DEV), st["pos"].to(DEV),
             st["ctr"].to(DEV), st["nsteps"].to(DEV), st["finished"].to(DEV), st["out"].to(DEV), -1, 2, True)
    torch.ops.bllm.spec_advance_(*[a.clone() if isinstance(a, torch.Tensor) else a for a in sargs])
    i32 = sargs[3]
    _refusals("spec_advance_", sargs, (
        (0, sargs[0].to(torch.int32)), (0, _strided(sargs[0])), (0, torch.zeros(2, 9, dtype=torch.long, device=DEV)),
        (1, sargs[1][:, :3].contiguous()), (1, sargs[1].to(torch.int32)),
        (2, sargs[2].to(torch.long)), (2, _strided(sargs[2])), (2, sargs[2][:1].contiguous()),
        (3, i32.to(torch.long)), (4, torch.cat([i32, i32])), (5, _strided(i32)), (6, i32.to(torch.long)),
        (7, sargs[7].to(torch.uint8)), (8, sargs[8].to(torch.int32)), (8, sargs[8][:1]),
        (10, 0), (10, 5),
    ))


# ------------------------------------------------------------------ model
@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_model_q_token_steps(name):
    """bf16: two steps of Q = 4 tokens per row after a ragged prefill, logits against the CPU fp32
    full forward."""
    gpu, cpu = _pair(name)
    lens, Q, steps = [1, 7, 40, 13], 4, 2
    g = torch.Generator().manual_seed(5)
    full = [torch.randint(0, gpu.cfg.vocab_size, (n + steps * Q,), generator=g) for n in lens]
    with torch.no_grad():
        want = [cpu(f[None])[0] for f in full]
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, lens)], DEV)
    cache = gpu.new_kv_cache(len(lens), 64)
    gpu.forward_prefill_ragged(idx, seq, cache)
    pos = torch.tensor(lens, dtype=torch.int32, device=DEV)
    j = torch.arange(Q, dtype=torch.int32, device=DEV)
    for s in range(steps):
        tok = torch.stack([f[n + s * Q:n + (s + 1) * Q] for f, n in zip(full, lens)]).reshape(-1, 1).to(DEV)
        lg = gpu.forward_cached_rows(tok, cache, (pos[:, None] + j).reshape(-1), q_per_row=Q)
        ref_rows = torch.stack([w[n + s * Q + jj] for w, n in zip(want, lens) for jj in range(Q)])
        check_close(lg, ref_rows, BF16, k=K_MODEL, name=f"{name} Q-token step {s}")
        pos += Q


def _spec_run(gpu, prompts, hints, K, new, capture, steps):
    """Prefill, first token, then ``steps`` SpecDecodeGraph steps -> (logits per step, final state)."""
    B, lens = len(prompts), [int(p.numel()) for p in prompts]
    idx, seq = pack_prompts(prompts, DEV)
    cache = gpu.new_kv_cache(B, 64)
    logits = gpu.forward_prefill_ragged(idx, seq, cache)
    pos = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(B, dtype=torch.int32, device=DEV)
    out = torch.zeros(B, new, dtype=torch.long, device=DEV)
    finished = torch.zeros(B, dtype=torch.bool, device=DEV)
    stream = torch.arange(B, device=DEV)
    first = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    ops.sample_rows(logits.contiguous(), stream, ctr, 3, 0.8, 20, 0.9, next_idx=first, out=out, finished=finished)
    sidx, hist, h0, nsteps = G.spec_state(prompts, lens, hints, K + 1, new, first, pos)
    ops.spec_advance(sidx, sidx.clone(), hist, h0, pos, ctr, nsteps, finished, out, -1, G.SPEC_NGRAM, accept=False)
    dec = G.SpecDecodeGraph(gpu, cache, sidx, hist, h0, pos, ctr, nsteps, finished, out, stream, 3, 0.8, 20, 0.9, -1,
                            capture=capture)
    assert (dec.graph is not None) == capture
    lgs = []
    for _ in range(steps):
        dec.replay()
        lgs.append(dec.logits.clone())
    return lgs, dict(idx=sidx, hist=hist, pos=pos, ctr=ctr, nsteps=nsteps, finished=finished, out=out)


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_spec_decode_graph_equals_eager(name):
    gpu, _ = _pair(name)
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, 8, (n,), generator=g) for n in [2, 7, 30, 13]]     # few letters: drafts do match
    (la, sa), (lb, sb) = (_spec_run(gpu, prompts, None, 3, 20, capture, 5) for capture in (True, False))
    for s, (a, b) in enumerate(zip(la, lb)):
        assert _same_bits(a, b), s
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert sa["nsteps"].tolist() == [5] * 4 and (sa["ctr"] >= 6).all()


def _sim_steps(prompts, res, hints, K, new, eos=None):
    steps = []
    for p, r, h in zip(prompts, res, hints):
        ans = r[p.numel():].tolist()
        if eos is not None and len(ans) < new:
            ans.append(eos)
        steps.append(len(S.simulate(p.tolist(), ans, [] if h is None else h.tolist(), K, G.SPEC_NGRAM)))
    return steps


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_ragged_speculative_bf16(name, monkeypatch):
    """Two graph runs and an eager run give the same tokens, and the step counts are the
    simulation's on those tokens (hints = the plain run's answers, which a bf16 run mostly, not
    always, reproduces: the two runs' GEMMs have different row counts)."""
    gpu, _ = _pair(name)
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, gpu.cfg.vocab_size, (n,), generator=g) for n in [1, 7, 40, 13]]
    new, K = 20, 3
    hints = [r.cpu() for r in G.generate_ragged(gpu, prompts, new, 64)]
    runs, stats = {}, {}
    for tag, flag in (("graph", "1"), ("graph again", "1"), ("eager", "0")):
        monkeypatch.setenv("BLLM_DECODE_GRAPH", flag)
        stats[tag] = {}
        runs[tag] = G.generate_ragged(gpu, prompts, new, 64, speculative=K, draft_hints=hints, stats=stats[tag])
    for p, a, b, c in zip(prompts, runs["graph"], runs["graph again"], runs["eager"]):
        assert a.numel() == p.numel() + new and torch.equal(a[:p.numel()].cpu(), p)
        assert torch.equal(a, b) and torch.equal(a, c)
    want = _sim_steps(prompts, [r.cpu() for r in runs["graph"]], hints, K, new)
    assert stats["graph"]["steps"] == stats["graph again"]["steps"] == stats["eager"]["steps"] == want
    assert stats["graph"]["new_tokens"] == [new] * len(prompts)


def test_generate_ragged_speculative_fp32_equals_plain():
    """fp32 on the GPU (oracle attention, eager): speculative == plain, token for token, unhinted
    and hinted, under the premise of test_generate_ragged_fp32_takes_the_oracle_decode_path: no
    step of the plain run has a runner-up within 1e-4 of its argmax."""
    cfg = _cfgs()["llama"].replace(dtype=F32)
    torch.manual_seed(0)
    m = build_model(cfg, device=DEV)
    m.flatten()
    m.eval()
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in [1, 7, 40, 13]]
    new, K = 12, 3
    plain = G.generate_ragged(m, prompts, new, 64)
    with torch.no_grad():
        for p, o in zip(prompts, plain):
            top = m(o[None])[0, p.numel() - 1:-1].float().topk(2, dim=-1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 1e-4
    for hints in (None, [r.cpu() for r in plain]):
        st = {}
        got = G.generate_ragged(m, prompts, new, 64, speculative=K, draft_hints=hints, stats=st)
        assert all(torch.equal(a, b) for a, b in zip(got, plain))
        assert st["steps"] == _sim_steps(prompts, [r.cpu() for r in got], hints or [None] * 4, K, new)
    assert max(st["steps"]) < new - 1            # hinted: drafts were accepted


# ------------------------------------------------------------------ debug build
CHILD = r"""
import torch
from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.ops import reference as ref
ops.load_ext(required=True)
assert torch.ops.bllm.kernel_debug_build()
dev, H, G, hd, Q, T = "cuda", 4, 2, 64, 4, 300
qkv = torch.randn(2 * Q, (H + 2 * G) * hd, device=dev).bfloat16()
kc, vc = torch.randn(2, G, T, hd, device=dev).bfloat16(), torch.randn(2, G, T, hd, device=dev).bfloat16()
pos = torch.tensor([7, 254], dtype=torch.int32, device=dev)
k1, v1 = kc.float().cpu(), vc.float().cpu()
out = ops.attn_extend_rows(qkv, kc, vc, pos, Q, H, G)
want = ref.attn_extend_rows(qkv.float().cpu(), k1, v1, pos.cpu(), Q, H, G)
assert (out.float().cpu() - want).abs().max() < 0.05, (out.float().cpu() - want).abs().max()
bad = torch.tensor([7, T - Q + 1], dtype=torch.int32, device=dev)       # clamped by the kernel after the check
try:
    ops.attn_extend_rows(qkv, kc, vc, bad, Q, H, G)
    raise SystemExit("attn_extend_rows: no error")
except RuntimeError as e:
    assert "decode cache position" in str(e), e
ops.attn_extend_rows(qkv, kc, vc, pos, Q, H, G)                         # the word was reset
print("DEBUG-MODE-OK")
"""


def test_attn_extend_rows_in_the_debug_build():
    lib = os.path.join(ROOT, "building_llm_from_scratch_amd", "_C_debug.so")
    assert os.path.isfile(lib), "build it with: python tools/build_ext.py --debug"
    env = dict(os.environ, BLLM_KERNEL_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "DEBUG-MODE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
