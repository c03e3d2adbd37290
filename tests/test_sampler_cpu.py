"""The seeded per-row sampler on the CPU: the counter hash, the top-k / top-p filters of the oracle
(``ops.reference.sample_rows_detail``) against an independent sort-and-cumsum implementation, the
distribution of its draws, and the plumbing through ``generate_ragged`` / ``generate_cached`` /
``Trainer.generate_responses`` and the command line."""
import json
import math

import pytest
import torch

from building_llm_from_scratch_amd import cli, ops
from building_llm_from_scratch_amd.data import tokenizer as tokmod
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

from test_generate_ragged_cpu import CTX, ENTRIES, VOCAB, _argv, _model, roomy_debug  # noqa: F401

NINF = float("-inf")


def _ids(n, first=0):
    return torch.arange(first, first + n, dtype=torch.long)


def _zeros(n):
    return torch.zeros(n, dtype=torch.int32)


# ------------------------------------------------------------------ hash
def test_uniforms_are_exact_fp32_inside_the_unit_interval():
    u = ref.sample_uniform(11, _ids(6), torch.tensor([0, 1, 2, 3, 4, 2 ** 31 - 1]), 4096)
    assert u.dtype == torch.float64 and u.shape == (6, 4096)
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert torch.equal(u.float().double(), u)
    assert torch.equal(u * 2 ** 24 % 2, torch.ones_like(u))          # odd multiples of 2^-24
    assert abs(float(u.mean()) - 0.5) < 0.01


def test_uniforms_are_a_function_of_seed_stream_counter_and_index():
    V = 512
    rows = [(3, 0, 0), (3, 0, 1), (3, 1, 0), (4, 0, 0), (3, 2 ** 32, 0), (3 + 2 ** 32, 0, 0), (3, -1, 0)]
    us = [ref.sample_uniform(s, torch.tensor([st]), torch.tensor([c]), V)[0] for s, st, c in rows]
    for a in range(len(us)):
        assert torch.equal(us[a], ref.sample_uniform(*[rows[a][0]], torch.tensor([rows[a][1]]),
                                                     torch.tensor([rows[a][2]]), V)[0])
        for b in range(a + 1, len(us)):
            assert float((us[a] == us[b]).double().mean()) < 0.01, (rows[a], rows[b])
    # a row's uniforms do not depend on the rows around it
    both = ref.sample_uniform(3, torch.tensor([1, 0]), torch.tensor([0, 1]), V)
    assert torch.equal(both[0], us[2]) and torch.equal(both[1], us[1])
    # within a row the indices get different values (2^23 of them: a few collisions at most)
    assert torch.unique(us[0]).numel() > V - 3


def test_equal_logits_different_streams_disagree_equal_streams_agree():
    l = torch.linspace(-1, 1, 50)[None].repeat(3, 1)
    stream = torch.tensor([5, 9, 5])
    toks = torch.stack([ref.sample_rows_detail(l, stream, torch.full((3,), c), 1, 1.0, detail=False)[0]
                        for c in range(64)], dim=1)
    assert torch.equal(toks[0], toks[2])
    assert not torch.equal(toks[0], toks[1])
    assert torch.unique(toks[0]).numel() > 8                          # the counter moves the draw


# ------------------------------------------------------------------ filters
def _kept_by_sorting(row, T, k, p):
    """The contract, literally: sort, walk the groups of equal values from the top."""
    V = len(row)
    kept = [True] * V
    if 0 < k < V:
        vk = sorted(row, reverse=True)[k - 1]
        kept = [x >= vk for x in row]
    ratios = []
    if p < 1.0 and max(row) > NINF:
        mx = max(row)
        w = [math.exp((x - mx) / T) if kp and x > NINF else 0.0 for x, kp in zip(row, kept)]
        total = math.fsum(w)
        vp = None
        for v in sorted({x for x, kp in zip(row, kept) if kp}, reverse=True):
            cum = math.fsum(wi for x, wi in zip(row, w) if x >= v)
            if cum > 0.0 and (not ratios or cum / total > ratios[-1]):
                ratios.append(cum / total)
            if vp is None and cum >= p * total:
                vp = v
        kept = [kp and x >= vp for x, kp in zip(row, kept)]
    return kept, ratios


def _tied_rows(B, V, seed, ninf_share=0.2):
    g = torch.Generator().manual_seed(seed)
    l = torch.randint(-4, 5, (B, V), generator=g).double() / 2          # 9 values: many ties
    l[torch.rand(B, V, generator=g) < ninf_share] = NINF
    l[:, 0] = l[:, 0].clamp_min(-2.0)                                   # one finite entry at least
    return l


@pytest.mark.parametrize("top_k,top_p,T", [(1, 1.0, 1.0), (5, 1.0, 1.0), (40, 1.0, 0.7), (41, 1.0, 1.0), (0, 1.0, 1.0),
                                           (0, 0.3, 1.0), (0, 0.77, 0.7), (0, 0.97, 2.0), (5, 0.6, 1.0),
                                           (12, 0.9, 0.5), (1, 0.5, 1.0)])
def test_filters_match_sort_and_cumsum(top_k, top_p, T):
    B, V = 16, 40
    l = _tied_rows(B, V, seed=top_k * 7 + int(top_p * 100))
    tok, thr, det = ref.sample_rows_detail(l, _ids(B), _zeros(B), 2, T, top_k, top_p)
    for b in range(B):
        row = l[b].tolist()
        kept, ratios = _kept_by_sorting(row, float(torch.tensor(T, dtype=torch.float32)), top_k, top_p)
        # the two implementations sum in different orders: no group boundary may sit on top_p
        assert all(abs(r - top_p) > 1e-9 for r in ratios), (b, ratios)
        assert det[b]["kept"].tolist() == kept, b
        assert torch.allclose(det[b]["ratios"], torch.tensor(ratios, dtype=torch.float64), rtol=1e-11, atol=0), b
        assert kept[int(tok[b])] and row[int(tok[b])] > NINF
        filtered = (0 < top_k < V) or top_p < 1.0
        assert float(thr[b]) == (min(x for x, kp in zip(row, kept) if kp) if filtered else NINF)
        assert bool((det[b]["keys"] > NINF).equal(det[b]["kept"] & (l[b] > NINF)))
        assert int(tok[b]) == int(det[b]["keys"].argmax())
        top2 = torch.topk(det[b]["keys"], 2).values
        assert det[b]["gap"] == (float(top2[0] - top2[1]) if sum(kept) > 1 else float("inf"))


def test_top_k_alone_keeps_what_the_multinomial_path_keeps():
    l = _tied_rows(8, 40, seed=3, ninf_share=0.0).float()
    _, _, det = ref.sample_rows_detail(l, _ids(8), _zeros(8), 0, 1.0, 5, 1.0)
    top, _ = torch.topk(l, 5)
    masked = l < top[:, -1:]                                            # train/generate.py:_sample
    assert torch.equal(torch.stack([d["kept"] for d in det]), ~masked)
    assert (~masked).sum(dim=1).max() > 5                               # ties at the threshold are kept


def test_greedy_and_special_rows():
    l = torch.tensor([[1.0, 3.0, 3.0, -1.0], [NINF, NINF, 0.5, NINF], [NINF] * 4, [2.0] * 4,
                      [float("nan"), 1.0, float("nan"), 1.0], [-0.0, 0.0, -1.0, -1.0]])
    tok, thr, _ = ref.sample_rows_detail(l, _ids(6), _zeros(6), 1, 0.0, 3, 0.5)
    assert tok.tolist() == [1, 2, 0, 0, 1, 0] and bool((thr == NINF).all())
    for k, p in [(0, 1.0), (2, 1.0), (0, 0.5), (3, 0.9)]:
        tok, thr, det = ref.sample_rows_detail(l, _ids(6), _zeros(6), 1, 1.0, k, p)
        assert int(tok[1]) == 2 and int(tok[2]) == 0 and int(tok[4]) in (1, 3) and int(tok[0]) in (0, 1, 2, 3)
        assert bool(det[3]["kept"].all())                               # all equal: top-k / top-p keep all of it
        assert bool(((tok >= 0) & (tok < 4)).all())


# ------------------------------------------------------------------ distribution
def _chi2_bound(dof, p=1.0 - 1e-6):
    """Wilson-Hilferty quantile of the chi-square distribution."""
    z = math.sqrt(2.0) * float(torch.erfinv(torch.tensor(2.0 * p - 1.0, dtype=torch.float64)))
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3


def chi2_case(sample, V=64, T=1.0, top_k=0, top_p=1.0, rows=4096, counters=8, seed=12345, device="cpu"):
    """Pearson chi-square of rows x counters draws from linspace(-2, 2, V) against the exact fp64
    probabilities of the kept set -> (statistic, bound, smallest expected count)."""
    l = torch.linspace(-2, 2, V, dtype=torch.float64)
    kept, _ = _kept_by_sorting(l.tolist(), T, top_k, top_p)
    kept = torch.tensor(kept)
    p = torch.where(kept, torch.softmax(l / T, dim=0), torch.zeros_like(l))
    p = p / p.sum()
    logits = l.float().to(device)[None].repeat(rows, 1)
    counts = torch.zeros(V, dtype=torch.float64)
    for c in range(counters):
        tok = sample(logits, _ids(rows).to(device), torch.full((rows,), c, dtype=torch.int32, device=device), seed, T,
                     top_k, top_p)
        counts += torch.bincount(tok.cpu(), minlength=V).double()
    n = rows * counters
    assert int(counts.sum()) == n and float(counts[~kept].sum()) == 0.0
    e = p[kept] * n
    stat = float(((counts[kept] - e) ** 2 / e).sum())
    return stat, _chi2_bound(int(kept.sum()) - 1), float(e.min())


def test_chi2_bound_is_the_wilson_hilferty_quantile():
    assert 131.0 < _chi2_bound(63) < 133.0


@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 1.0), (1.0, 10, 1.0), (1.0, 0, 0.8), (0.5, 0, 1.0), (2.0, 0, 1.0)])
def test_draws_follow_the_softmax_of_the_kept_set(T, top_k, top_p):
    sample = lambda *a: ref.sample_rows_detail(*a, detail=False)[0]
    stat, bound, emin = chi2_case(sample, T=T, top_k=top_k, top_p=top_p)
    print(f"T={T} top_k={top_k} top_p={top_p}: chi2 {stat:.1f} bound {bound:.1f} smallest expected count {emin:.1f}")
    assert emin > 1.0            # 38 at T = 1, 1.3 at T = 0.5: no cell the chi-square approximation cannot carry
    assert stat < bound


# ------------------------------------------------------------------ plumbing
PROMPT_LENS = [3, 9, 1, 6]


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, VOCAB, (n,), generator=g) for n in PROMPT_LENS]


@pytest.fixture
def recorded(monkeypatch):
    """``ops.sample_rows`` wrapped to record each call's arguments (copies from before the call)."""
    calls = []
    real = ops.sample_rows

    def wrapper(logits, stream, ctr, seed, temperature, top_k=0, top_p=1.0, **kw):
        rec = dict(logits=logits.clone(), stream=stream.clone(), ctr=ctr.clone(), seed=seed, T=temperature,
                   top_k=top_k, top_p=top_p, kw=kw)
        rec["tokens"] = real(logits, stream, ctr, seed, temperature, top_k, top_p, **kw).clone()
        rec["ctr_after"] = ctr.clone()
        calls.append(rec)
        return rec["tokens"]
    monkeypatch.setattr(ops, "sample_rows", wrapper)
    return calls


def check_calls(calls, streams, seed, T, top_k, top_p, max_near_ties=0.01):
    """Every recorded call: the given stream ids, counters 0, 1, 2, ..., and tokens that are the
    oracle's on the recorded logits (near-tie rule of the GPU suite; exact on the CPU)."""
    near = 0
    for step, c in enumerate(calls):
        assert c["stream"].tolist() == list(streams) and c["stream"].dtype == torch.long
        assert c["ctr"].tolist() == [step] * len(streams) and c["ctr_after"].tolist() == [step + 1] * len(streams)
        assert (c["seed"], c["T"], c["top_k"], c["top_p"]) == (seed, T, top_k, top_p)
        want, _, det = ref.sample_rows_detail(c["logits"].cpu(), c["stream"].cpu(), c["ctr"].cpu(), seed, T, top_k, top_p)
        for b, d in enumerate(det):
            tol = 2.0 ** -20 * max(1.0, float(d["keys"][d["keys"] > NINF].abs().max()))
            got = int(c["tokens"][b])
            if d["gap"] < tol:
                near += 1
                assert float(d["keys"].max() - d["keys"][got]) <= tol, (step, b)
            else:
                assert got == int(want[b]), (step, b)
    assert near <= max_near_ties * len(calls) * len(streams)


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_ragged_feeds_the_sampler_streams_and_counters(name, recorded):
    m, new = _model(name), 12
    streams = [7, 2 ** 40, 0, 3]
    res = G.generate_ragged(m, _prompts(), new, CTX, temperature=0.8, top_k=20, top_p=0.9, seed=5, streams=streams)
    assert len(recorded) == new
    check_calls(recorded, streams, 5, 0.8, 20, 0.9)
    for b, (r, p) in enumerate(zip(res, _prompts())):
        assert torch.equal(r, torch.cat((p, torch.stack([c["tokens"][b] for c in recorded]))))
    # every call hands over the same device-side state
    assert all(c["kw"]["out"] is recorded[0]["kw"]["out"] and c["kw"]["finished"] is recorded[0]["kw"]["finished"]
               for c in recorded)
    # deterministic, and a row's stream decides its draws: default streams are the row numbers
    n0 = len(recorded)
    again = G.generate_ragged(m, _prompts(), new, CTX, temperature=0.8, top_k=20, top_p=0.9, seed=5, streams=streams)
    assert all(torch.equal(a, b) for a, b in zip(res, again))
    G.generate_ragged(m, _prompts(), 2, CTX, temperature=0.8, seed=5)
    assert recorded[n0 + new]["stream"].tolist() == [0, 1, 2, 3] and recorded[n0 + new]["top_p"] == 1.0


@pytest.mark.parametrize("check_every", [1, 16])
def test_generate_ragged_sampled_rows_stop_on_their_own_eos(check_every, recorded, monkeypatch):
    monkeypatch.setattr(G, "EOS_CHECK_EVERY", check_every)
    m, new = _model("llama"), 24
    kw = dict(temperature=1.0, top_k=8, seed=9)
    free = G.generate_ragged(m, _prompts(), new, CTX, **kw)
    gen = [f[n:] for f, n in zip(free, PROMPT_LENS)]
    eos = int(gen[0][2])
    recorded.clear()
    got = G.generate_ragged(m, _prompts(), new, CTX, eos_id=eos, **kw)
    first = [(g == eos).nonzero() for g in gen]
    for b, (p, g, f) in enumerate(zip(_prompts(), gen, first)):
        assert torch.equal(got[b], torch.cat((p, g[:int(f[0])] if f.numel() else g))), b
    assert got[0].numel() <= PROMPT_LENS[0] + 2
    drawn = torch.stack([c["tokens"] for c in recorded], dim=1)
    assert torch.equal(recorded[-1]["kw"]["finished"], (drawn == eos).any(dim=1))
    assert all(c["kw"]["eos_id"] == eos for c in recorded)
    if all(f.numel() for f in first):          # every row stopped: the loop ended at the next check
        last = max(int(f[0]) for f in first) + 1
        assert len(recorded) == min(new, -(-last // check_every) * check_every)


def test_without_seed_the_sampler_is_not_called(recorded):
    m = _model("llama")
    G.generate_ragged(m, _prompts(), 4, CTX)
    G.generate_ragged(m, _prompts(), 4, CTX, temperature=1.0, top_k=5, generator=torch.Generator().manual_seed(3))
    G.generate_cached(m, _prompts()[1][None], 4, CTX, temperature=1.0, top_k=5,
                      generator=torch.Generator().manual_seed(3))
    assert recorded == []


def test_sampler_argument_refusals(recorded):
    m, p = _model("llama"), _prompts()
    for fn, first in ((G.generate_ragged, p), (G.generate_cached, p[1][None])):
        B = len(first)
        with pytest.raises(ValueError, match="top_p"):
            fn(m, first, 4, CTX, temperature=1.0, top_p=0.9)
        with pytest.raises(ValueError, match="seed"):
            fn(m, first, 4, CTX, temperature=1.0, streams=list(range(B)))
        for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(temperature=-0.5), dict(seed=1.5),
                    dict(streams=list(range(B + 1))), dict(streams=[2 ** 63] * B)):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(m, first, 4, CTX, **{"temperature": 1.0, "seed": 1, **bad})
    assert recorded == []
    with pytest.raises(ValueError, match="sample_rows"):
        ref.sample_rows(torch.zeros(1, 4), _ids(1), _zeros(1), 0, 1.0, 0, 0.0)


def test_generate_cached_counters_run_across_the_sliding_window(recorded):
    m, ctx, new = _model("gpt2"), 8, 10
    idx = torch.stack([_prompts()[1][:6], _prompts()[3]])
    prefills = []
    fwd = m.forward_cached
    m.forward_cached = lambda i, c, pos: (prefills.append(i.shape[1]), fwd(i, c, pos))[1]
    try:
        out = G.generate_cached(m, idx, new, ctx, temperature=0.9, top_p=0.95, seed=4, streams=[11, 12])
    finally:
        del m.forward_cached
    assert prefills.count(ctx) >= 2                                     # the window slid by re-prefilling
    assert len(recorded) == new
    check_calls(recorded, [11, 12], 4, 0.9, 0, 0.95)
    assert torch.equal(out[:, :6], idx)
    assert torch.equal(out[:, 6:], torch.stack([c["tokens"] for c in recorded], dim=1))
    # a row alone under its stream id draws what it drew in the batch (fp32 on the CPU: same logits)
    one = G.generate_cached(m, idx[1:], new, ctx, temperature=0.9, top_p=0.95, seed=4, streams=[12])
    assert torch.equal(one[0], out[1])


# ------------------------------------------------------------------ Trainer and command line
@pytest.fixture
def id_decode(monkeypatch):
    """The offline byte tokenizer decodes the ids a random-init model emits to nothing: decode to
    the ids themselves."""
    for cls in (tokmod.ByteTokenizer, tokmod.BPETokenizer):
        monkeypatch.setattr(cls, "decode", lambda self, ids: " ".join(str(int(i)) for i in ids))


def _gen_only(tmp_path, extra, out="out"):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(ENTRIES))
    argv = _argv(tmp_path, "llama3_2", ["--generate_only", "--generate_prompts", str(pf)] + extra)
    argv[argv.index("--output_dir") + 1] = str(tmp_path / out)
    return cli.cli(argv), json.load(open(tmp_path / out / "responses.json"))


def test_cli_sampled_answers_are_reproducible(tmp_path, roomy_debug, id_decode, recorded):  # noqa: F811
    flags = ["--generate_temperature", "1", "--generate_top_p", "0.9"]
    tr, a = _gen_only(tmp_path, flags + ["--generate_seed", "3"], "a")
    assert recorded and all(c["seed"] == 3 and c["T"] == 1.0 and c["top_k"] == 0 and c["top_p"] == 0.9 for c in recorded)
    _, b = _gen_only(tmp_path, flags + ["--generate_seed", "3"], "b")
    _, c = _gen_only(tmp_path, flags + ["--generate_seed", "4"], "c")
    assert a == b and [r["prompt"] for r in a] == [r["prompt"] for r in c]
    assert [r["response"] for r in a] != [r["response"] for r in c]
    assert all(len(r["response"].split()) == 5 for r in a)
    # Trainer.generate_responses: prompt i draws from stream i whatever the batches are
    _, texts = cli.load_generate_prompts(tmp_path / "prompts.json")
    lens = [len(tr.loaderObj.tokenizer.encode(t, allowed_special={tr.config["eos_text"]})) for t in texts]
    order = sorted(range(len(texts)), key=lambda i: lens[i])
    for bs in (1, 2, len(texts)):
        recorded.clear()
        got = tr.generate_responses(texts, 5, bs, temperature=1.0, top_p=0.9, seed=3)
        assert got == [r["response"] for r in a], bs
        firsts = [c["stream"].tolist() for c in recorded if int(c["ctr"][0]) == 0]
        assert firsts == [order[s:s + bs] for s in range(0, len(order), bs)]
    recorded.clear()
    greedy = tr.generate_responses(texts, 5, 2)
    assert recorded == [] and greedy == tr.generate_responses(texts, 5, 2, temperature=0.0)


def test_cli_sampling_flag_refusals(tmp_path):
    base = ["--data_dir", str(tmp_path)]
    for flag, bad in (("--generate_temperature", "-1"), ("--generate_temperature", "nan"), ("--generate_top_k", "-2"),
                      ("--generate_top_p", "0"), ("--generate_top_p", "1.01"), ("--generate_seed", str(2 ** 64))):
        with pytest.raises(ValueError, match=flag):
            cli.get_args(base + [flag, bad])
    a = cli.get_args(base)
    assert (a.generate_temperature, a.generate_top_k, a.generate_top_p, a.generate_seed) == (0.0, 0, 1.0, 0)
    a = cli.get_args(base + ["--generate_temperature", "0.7", "--generate_top_k", "40", "--generate_top_p", "0.95",
                             "--generate_seed", "17"])
    assert (a.generate_temperature, a.generate_top_k, a.generate_top_p, a.generate_seed) == (0.7, 40, 0.95, 17)
