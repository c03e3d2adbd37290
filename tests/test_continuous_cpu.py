"""Continuous batching (``train/generate.py::generate_continuous``) on the CPU in fp32: the schedule
against a pure-Python oracle, the answers against one-row ``generate_cached`` runs whatever the
slot count, per-row eos, seeded sampling, the fp8 cache and the weight packs, a slot's stale
predecessor, the slot-mapped oracle fills, the refusals and the command line."""
import json

import pytest
import torch

import continuous_cases as C
from test_generate_ragged_cpu import (CTX, ENTRIES, VOCAB, _argv, _model, _one_row, _streams,  # noqa: F401
                                      roomy_debug)

from building_llm_from_scratch_amd import cli, ops
from building_llm_from_scratch_amd.models.base import pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

_CACHE = {}


def _prompts(name):
    """The nine prompts of ``C.LENS`` from ``_streams``.  Llama's length-3 draw has a runner-up
    1.6e-4 below its argmax at one step, which rounding between batch shapes may flip: it is
    replaced by another 3-token draw (the premise is asserted in ``_ones``)."""
    ps = _streams(C.LENS, 0)
    if name == "llama":
        ps[4] = torch.randint(0, VOCAB, (3,), generator=torch.Generator().manual_seed(100))
    return ps


def _ones(name):
    """One-row greedy ``generate_cached`` runs of the nine prompts, 12 tokens each, computed once
    per family, with the premise that makes tokens comparable across batch shapes: no step has a
    runner-up within 1e-3 of its argmax."""
    if name not in _CACHE:
        m = _model(name)
        runs = []
        for p in _prompts(name):
            seq = _one_row(m, p, C.NEW)
            with torch.no_grad():
                top = m(seq[None])[0, p.numel() - 1:-1].topk(2, dim=-1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 1e-3, p.numel()
            runs.append(seq)
        _CACHE[name] = runs
    return _CACHE[name]


def _budget_list(budgets):
    return [budgets] * len(C.LENS) if isinstance(budgets, int) else list(budgets)


# ------------------------------------------------------------------ the schedule oracle itself
def test_simulate_by_hand():
    # 2 slots, budgets 3 / 1 / 2, no eos, E = 16.  Round 1: prompts 0, 1 admitted; prompt 1 is done
    # at once (run 0).  Round 2: prompt 2 into slot 1; run min(3-1, 2-1) = 1; prompt 2 done.
    # Round 3: nothing waits; run 1; prompt 0 done.
    assert C.simulate([None] * 3, [3, 1, 2], 2, 16, False) == \
        {"replays": 2, "prefills": 2, "slot": [0, 1, 1], "steps": [2, 0, 1]}
    # E caps a run; a budget of 0 never takes a slot
    assert C.simulate([None] * 2, [0, 40], 4, 16, False) == \
        {"replays": 39, "prefills": 1, "slot": [None, 0], "steps": [0, 39]}
    # eos: prompt 0 draws its eos as token 2 of 10; seen at the first look at or after it
    assert C.simulate([2, None], [10, 10], 1, 1, True)["steps"] == [1, 9]
    assert C.simulate([2, None], [10, 10], 1, 4, True)["steps"] == [4, 9]
    assert C.simulate([2, None], [10, 10], 1, 4, False)["steps"] == [9, 9]
    assert C.static_replays(C.BUDGETS, 3) == 11 + 11 + 9


# ------------------------------------------------------------------ same answers, fewer steps
@pytest.mark.parametrize("budgets", [C.NEW, C.BUDGETS], ids=["one_budget", "budgets"])
@pytest.mark.parametrize("slots", [1, 2, 3, 9])
@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_greedy_equals_one_row_runs(name, slots, budgets):
    m, prompts, ones = _model(name), _prompts(name), _ones(name)
    stats = {}
    res = G.generate_continuous(m, prompts, budgets, CTX, slots, stats=stats)
    b = _budget_list(budgets)
    assert len(res) == len(prompts)
    for i, (p, r, one) in enumerate(zip(prompts, res, ones)):
        assert r.dtype == torch.long and torch.equal(r, one[:p.numel() + b[i]]), i
    assert C.stats_match(stats, C.simulate([None] * 9, b, slots, G.EOS_CHECK_EVERY, False)), stats
    assert stats["new_tokens"] == b
    if slots < 9:                              # slots really turn over
        assert stats["prefills"] >= 2
        assert max(stats["slot"].count(s) for s in range(slots)) >= 2
    if slots < 9 and budgets is C.BUDGETS:     # and that is where the steps are saved
        assert stats["replays"] <= C.static_replays(b, slots)


def test_zero_budget_prompts_never_take_a_slot():
    m, prompts, ones = _model("gpt2"), _prompts("gpt2"), _ones("gpt2")
    b = [0, 4, 0, 2, 0, 0, 3, 0, 0]
    stats = {}
    res = G.generate_continuous(m, prompts, b, CTX, 2, stats=stats)
    for i, (p, r, one) in enumerate(zip(prompts, res, ones)):
        assert torch.equal(r, one[:p.numel() + b[i]]), i
    assert C.stats_match(stats, C.simulate([None] * 9, b, 2, G.EOS_CHECK_EVERY, False))
    assert [s is None for s in stats["slot"]] == [n == 0 for n in b]
    stats = {}
    assert all(torch.equal(r, p) for r, p in zip(G.generate_continuous(m, prompts, 0, CTX, 2, stats=stats), prompts))
    assert stats["replays"] == stats["prefills"] == 0


# ------------------------------------------------------------------ per-row eos
def test_rows_stop_on_their_own_eos(monkeypatch):
    m, prompts, ones = _model("llama"), _prompts("llama"), _ones("llama")
    gen = [o[p.numel():].tolist() for o, p in zip(ones, prompts)]
    eos = 0
    # the premise: rows that stop early next to rows that run to their budget
    alen = [g.index(eos) + 1 if eos in g else None for g in gen]
    assert sum(a is not None and a < C.NEW for a in alen) >= 2 and sum(a is None for a in alen) >= 1
    slots, runs = 3, {}
    for every in (1, 16):
        monkeypatch.setattr(G, "EOS_CHECK_EVERY", every)
        stats = {}
        runs[every] = G.generate_continuous(m, prompts, C.NEW, CTX, slots, eos_id=eos, stats=stats)
        for i, (p, r, g, a) in enumerate(zip(prompts, runs[every], gen, alen)):
            want = g if a is None else g[:a - 1]                  # cut before the eos
            assert r.tolist() == p.tolist() + want, (every, i)
        sim = C.simulate(alen, [C.NEW] * 9, slots, every, True)
        assert C.stats_match(stats, sim), (every, stats, sim)
        assert stats["new_tokens"] == [C.NEW if a is None else a for a in alen]
        if every == 1:
            assert stats["replays"] < C.static_replays([C.NEW] * 9, slots)
    assert all(torch.equal(a, b) for a, b in zip(runs[1], runs[16]))


# ------------------------------------------------------------------ seeded sampling
def test_seeded_sampling_does_not_depend_on_the_slots():
    m, prompts = _model("llama"), _prompts("llama")
    kw = dict(temperature=1.0, top_k=5, seed=11)
    streams = list(range(9))
    want = G.generate_ragged(m, prompts, C.NEW, CTX, streams=streams, **kw)
    # the premise, as for the argmax: on the whole-list run's own logits no draw has a runner-up key
    # within 1e-3, and no logit sits within 1e-4 of the top-k threshold from below
    for i, (p, w) in enumerate(zip(prompts, want)):
        with torch.no_grad():
            lg = m(w[None])[0, p.numel() - 1:-1]
        n = lg.shape[0]
        tok, _, det = ref.sample_rows_detail(lg, torch.full((n,), i, dtype=torch.long),
                                             torch.arange(n, dtype=torch.int32), 11, 1.0, 5, 1.0)
        assert tok.tolist() == w[p.numel():].tolist(), i
        assert min(d["gap"] for d in det) > 1e-3, i
        top = lg.topk(6, dim=-1).values
        assert float((top[:, 4] - top[:, 5]).min()) > 1e-4, i
    for slots in (2, 9):
        got = G.generate_continuous(m, prompts, C.NEW, CTX, slots, streams=streams, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), slots
    assert all(torch.equal(a, b) for a, b in zip(G.generate_continuous(m, prompts, C.NEW, CTX, 2, **kw), want))
    # a prompt's answer goes with its stream: the same prompt on stream j draws what it drew there
    perm = [3, 0, 8, 1, 2, 7, 4, 6, 5]
    moved = G.generate_continuous(m, prompts, C.NEW, CTX, 3, streams=perm, **kw)
    alone = [G.generate_ragged(m, [p], C.NEW, CTX, streams=[s], **kw)[0] for p, s in zip(prompts, perm)]
    assert all(torch.equal(a, b) for a, b in zip(moved, alone))
    assert any(not torch.equal(a, b) for a, b in zip(moved, want))


# ------------------------------------------------------------------ fp8 cache and weight packs
@pytest.mark.parametrize("opt", [dict(kv_dtype="fp8"), dict(weight_dtype="fp8"), dict(weight_dtype="mxfp4")],
                         ids=["kv_fp8", "w_fp8", "w_mxfp4"])
def test_quantised_cache_and_weights(opt):
    m, prompts = _model("llama"), _prompts("llama")
    stats = {}
    res = G.generate_continuous(m, prompts, C.BUDGETS, CTX, 3, stats=stats, **opt)
    assert [r.numel() for r in res] == [n + b for n, b in zip(C.LENS, C.BUDGETS)]
    assert all(torch.equal(r[:n], p) for r, n, p in zip(res, C.LENS, prompts))
    assert C.stats_match(stats, C.simulate([None] * 9, C.BUDGETS, 3, G.EOS_CHECK_EVERY, False))
    whole = G.generate_continuous(m, prompts, C.NEW, CTX, 9, **opt)
    want = G.generate_ragged(m, prompts, C.NEW, CTX, **opt)
    assert all(torch.equal(a, b) for a, b in zip(whole, want))
    if "weight_dtype" in opt:                  # a prebuilt pack is taken as it is
        packs = m.new_decode_weights(opt["weight_dtype"])
        again = G.generate_continuous(m, prompts, C.NEW, CTX, 9, weight_dtype=packs)
        assert all(torch.equal(a, b) for a, b in zip(again, want))


# ------------------------------------------------------------------ a slot's predecessor
@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_new_occupant_never_sees_a_stale_slot(name):
    """A 30-token prompt fills one slot and finishes; a 1-token prompt takes the same slot over
    the 30 + 12 positions it left: its answer is its one-row run's."""
    m, prompts, ones = _model(name), _prompts(name), _ones(name)
    stats = {}
    res = G.generate_continuous(m, [prompts[7], prompts[0]], C.NEW, CTX, 1, stats=stats)
    assert stats["slot"] == [0, 0] and stats["prefills"] == 2
    assert torch.equal(res[0], ones[7]) and torch.equal(res[1], ones[0])


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_prefill_into_chosen_rows_matches_the_full_forward(name):
    """``forward_prefill_ragged(rows=)``: prompts of 7 and 40 tokens into rows 2 and 0 of a 3-row
    cache, 6 steps, a 13-token prompt over row 0's 46 used positions, 6 more steps -- every logits
    row of a live slot equals the full forward of its own tokens (fp32, atol 1e-5)."""
    m = _model(name)
    full = {2: _streams([7], 12)[0], 0: _streams([40], 6)[0]}
    start = {2: 7, 0: 40}
    late = torch.randint(0, VOCAB, (13 + 6,), generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want = {s: m(f[None])[0] for s, f in full.items()}
        want_late = m(late[None])[0]
        cache = m.new_kv_cache(3, CTX)
        idx, seq = pack_prompts([full[2][:7], full[0][:40]], "cpu")
        lg = m.forward_prefill_ragged(idx, seq, cache, rows=[2, 0])
        assert lg.shape == (2, VOCAB)
        assert torch.allclose(lg[0], want[2][6], atol=1e-5) and torch.allclose(lg[1], want[0][39], atol=1e-5)
        pos = torch.tensor([40, 0, 7], dtype=torch.int32)
        for s in range(6):
            tok = torch.stack([full[0][40 + s], torch.tensor(0), full[2][7 + s]])[:, None]
            lg = m.forward_cached_rows(tok, cache, pos)
            pos += 1
            assert torch.allclose(lg[0], want[0][40 + s], atol=1e-5) and torch.allclose(lg[2], want[2][7 + s], atol=1e-5)
        idx, seq = pack_prompts([late[:13]], "cpu")
        lg = m.forward_prefill_ragged(idx, seq, cache, rows=torch.tensor([0]))
        assert torch.allclose(lg[0], want_late[12], atol=1e-5)
        pos[0] = 13
        for s in range(6):
            tok = torch.stack([late[13 + s], torch.tensor(0), full[2][13 + s]])[:, None]
            lg = m.forward_cached_rows(tok, cache, pos)
            pos += 1
            assert torch.allclose(lg[0], want_late[13 + s], atol=1e-5), s
            assert torch.allclose(lg[2], want[2][13 + s], atol=1e-5), s
        # without rows= nothing changed: the sequence count must still be the cache's rows
        with pytest.raises(ValueError, match="do not fit"):
            m.forward_prefill_ragged(idx, seq, cache)
        for bad in ([3], [0, 1], [-1], [0.0]):
            with pytest.raises(ValueError, match="ragged prefill"):
                m.forward_prefill_ragged(idx, seq, cache, rows=bad)


# ------------------------------------------------------------------ oracle fills
def _fill_case():
    H, Gk, hd, Tmax = 4, 2, 16, 12
    lens, rows = [3, 0, 7, 1], [5, 0, 3, 2]
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(2 + sum(lens), (H + 2 * Gk) * hd, generator=g)    # two leading rows outside every sequence
    cu = torch.tensor([2, 5, 5, 12, 13], dtype=torch.int32)
    return H, Gk, hd, Tmax, lens, rows, qkv, cu


def test_oracle_fill_into_chosen_rows():
    H, Gk, hd, Tmax, lens, rows, qkv, cu = _fill_case()
    kc = torch.full((6, Gk, Tmax, hd), 7.0)
    vc = torch.full((6, Gk, Tmax, hd), -7.0)
    ops.kv_cache_fill_varlen(qkv, cu, kc, vc, rows=rows)              # CPU tensors: the oracle, through the wrapper
    packed = qkv.view(-1, H + 2 * Gk, hd)
    wk, wv = torch.full_like(kc, 7.0), torch.full_like(vc, -7.0)
    for i, (n, r) in enumerate(zip(lens, rows)):
        r0 = int(cu[i])
        for t in range(n):
            wk[r, :, t] = packed[r0 + t, H:H + Gk]
            wv[r, :, t] = packed[r0 + t, H + Gk:]
    assert torch.equal(kc, wk) and torch.equal(vc, wv)
    assert (kc[1] == 7.0).all() and (kc[4] == 7.0).all() and (kc[0] == 7.0).all()     # untouched / empty sequence
    # rows = 0..n-1 is rows=None
    a, b = (torch.full((4, Gk, Tmax, hd), 1.0) for _ in range(2))
    a2, b2 = a.clone(), b.clone()
    ref.kv_cache_fill_varlen(qkv, cu, a, b)
    ref.kv_cache_fill_varlen(qkv, cu, a2, b2, rows=[0, 1, 2, 3])
    assert torch.equal(a, a2) and torch.equal(b, b2)


def test_oracle_fp8_fill_into_chosen_rows():
    H, Gk, hd, Tmax, lens, rows, qkv, cu = _fill_case()
    k8, v8 = (torch.full((6, Gk, Tmax, hd), 0.5).to(torch.float8_e4m3fn) for _ in range(2))
    ks, vs = torch.full((6, Gk, Tmax), 3.0), torch.full((6, Gk, Tmax), -3.0)
    want = [t.clone() for t in (k8, v8, ks, vs)]
    ops.kv_cache_fill_varlen(qkv, cu, k8, v8, scales=(ks, vs), rows=torch.tensor(rows))
    packed = qkv.view(-1, H + 2 * Gk, hd)
    for i, (n, r) in enumerate(zip(lens, rows)):
        r0 = int(cu[i])
        for t in range(n):
            want[0][r, :, t], want[2][r, :, t] = ref.kv_quantize_rows(packed[r0 + t, H:H + Gk])
            want[1][r, :, t], want[3][r, :, t] = ref.kv_quantize_rows(packed[r0 + t, H + Gk:])
    for got, w in zip((k8, v8, ks, vs), want):
        assert torch.equal(got.view(torch.uint8) if got.dtype != torch.float32 else got,
                           w.view(torch.uint8) if w.dtype != torch.float32 else w)
    assert (ks[1] == 3.0).all() and (ks[4] == 3.0).all() and (ks[5, :, 3:] == 3.0).all()


def test_fill_rows_are_checked_on_the_host():
    H, Gk, hd, Tmax, lens, rows, qkv, cu = _fill_case()
    kc, vc = torch.zeros(6, Gk, Tmax, hd), torch.zeros(6, Gk, Tmax, hd)
    for bad, what in (([5, 0, 3], "one cache row per sequence"), ([5, 0, 3, 2, 1], "one cache row per sequence"),
                      ([5, 0, 3, 3], "distinct"), ([6, 0, 3, 2], "inside"), ([-1, 0, 3, 2], "inside"),
                      ([5.0, 0, 3, 2], "host integers"), (torch.tensor([[5, 0, 3, 2]]), "host integers"),
                      ("5032", "host integers")):
        with pytest.raises(ValueError, match=what):
            ops.kv_cache_fill_varlen(qkv, cu, kc, vc, rows=bad)
    assert not kc.any() and not vc.any()
    made = ops.CacheRows(rows, 4, 6, "cpu")
    assert made.host == rows and made.dev.dtype == torch.int32 and made.dev.tolist() == rows
    ops.kv_cache_fill_varlen(qkv, cu, kc, vc, rows=made)
    assert kc[5, :, :3].any()
    with pytest.raises(ValueError, match="do not go with"):
        ops.kv_cache_fill_varlen(qkv, cu, kc[:5], vc[:5], rows=made)


# ------------------------------------------------------------------ refusals and the command line
def test_refusals():
    m = _model("llama")
    p = torch.arange(5)
    for kw, what in ((dict(slots=0), "slots"), (dict(slots=True), "slots"),
                     (dict(max_new_tokens=[4]), "one int per prompt"),
                     (dict(max_new_tokens=[4, -1]), "budget"), (dict(max_new_tokens=-1), "budget"),
                     (dict(prompts=[p, torch.zeros(0, dtype=torch.long)]), "prompt 1"),
                     (dict(prompts=[]), "non-empty list"),
                     (dict(prompts=[p, torch.arange(30)], max_new_tokens=[4, 19]), r"prompt 1 \(30 tokens\).*19.*48"),
                     (dict(context_size=CTX + 1), "model's context length"),
                     (dict(temperature=1.0), "seed"), (dict(kv_dtype="int8"), "kv_dtype"),
                     (dict(weight_dtype="int4"), "weight_dtype"),
                     (dict(seed=1, temperature=1.0, streams=[0]), "streams")):
        args = dict(prompts=[p, p], max_new_tokens=4, context_size=CTX, slots=2)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            G.generate_continuous(m, **args)
    with pytest.raises(TypeError):             # the device sampler is the only one: no generator argument
        G.generate_continuous(m, [p], 4, CTX, 1, generator=torch.Generator())
    assert G.generate_continuous(m, [p, torch.arange(30)], [4, 18], CTX, 2)[1].numel() == 48      # exactly full


def test_cli_flag(tmp_path):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(ENTRIES))
    base = ["--data_dir", str(tmp_path), "--generate_prompts", str(pf)]
    assert cli.get_args(base).generate_continuous is False
    a = cli.get_args(base + ["--generate_continuous", "--generate_kv_dtype", "fp8", "--generate_weight_dtype", "fp8",
                             "--generate_temperature", "0.7", "--generate_top_k", "5"])
    assert a.generate_continuous is True
    with pytest.raises(ValueError, match="--generate_continuous"):
        cli.get_args(base + ["--generate_continuous", "--generate_speculative", "2"])


@pytest.mark.parametrize("model", ["GPT2", "llama3_2"])
def test_cli_generate_only_writes_the_same_answers(model, tmp_path, roomy_debug, monkeypatch):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(ENTRIES))
    out = tmp_path / "out" / "responses.json"
    cli.cli(_argv(tmp_path, model, ["--generate_only", "--generate_prompts", str(pf)]))
    want = json.load(open(out))
    out.unlink()
    tr = cli.cli(_argv(tmp_path, model, ["--generate_only", "--generate_prompts", str(pf), "--generate_continuous"]))
    assert json.load(open(out)) == want and len(want) == len(ENTRIES)
    # with answers that tell the prompts apart (the byte tokenizer decodes most ids to nothing)
    _, texts = cli.load_generate_prompts(pf)
    monkeypatch.setattr(tr.loaderObj.tokenizer, "decode", lambda ids: " ".join(str(i) for i in ids), raising=False)
    plain = tr.generate_responses(texts, 5, 2)
    assert len(set(plain)) > 1
    assert tr.generate_responses(texts, 5, 2, continuous=True) == plain
    assert tr.generate_responses(texts, 5, 1, continuous=True) == plain
    with pytest.raises(ValueError, match="continuous"):
        tr.generate_responses(texts, 5, 2, continuous=True, speculative=2)
