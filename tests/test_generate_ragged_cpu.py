"""Batched generation from prompts of different lengths, on the CPU in fp32: the ragged prefill
and the per-row decode step against the full forward, ``generate_ragged`` against one-row
``generate_cached`` runs, per-row stopping, the refusals, and the command line."""
import json
import os

import pytest
import torch

from building_llm_from_scratch_amd import builder, cli
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.models import build_model, replace_linear_with_lora
from building_llm_from_scratch_amd.models.base import pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

CTX, VOCAB = 48, 97
SEED = 0            # model seed: the one-row greedy runs below have no near-tied argmax (checked there)


def _cfg(name):
    # the tiny models of tests/test_unpad_cpu.py, with room for 24 prompt + 12 new tokens
    if name.startswith("llama"):
        return get_config("llama3_2", "1B").replace(context_length=CTX, emb_dim=64, n_heads=4, n_kv_groups=2,
                                                    hidden_dim=96, n_layers=2, vocab_size=VOCAB, dtype=torch.float32)
    return get_config("GPT2", "124M").replace(context_length=CTX, emb_dim=64, n_heads=4, n_kv_groups=4, hidden_dim=256,
                                              n_layers=2, vocab_size=VOCAB, dtype=torch.float32, drop_rate=0.0)


_MODELS = {}


def _model(name):
    """One model per family for the whole file; tests only run inference on it."""
    if name not in _MODELS:
        torch.manual_seed(SEED)
        m = build_model(_cfg(name))
        if name == "llama_lora":
            for p in m.parameters():
                p.requires_grad = False
            replace_linear_with_lora(m, rank=4, alpha=8)
            with torch.no_grad():   # LoRA B starts at zero: give the adapters something to do
                for n, p in m.named_parameters():
                    if p.requires_grad:
                        p.copy_(0.05 * torch.randn(p.shape))
        m.flatten()
        m.eval()
        _MODELS[name] = m
    return _MODELS[name]


def _streams(lens, extra):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, VOCAB, (n + extra,), generator=g) for n in lens]


# ------------------------------------------------------------------ oracle ops
def test_oracle_fill_and_rows_match_padded_cache():
    """The two new oracles against plain indexing: the filled cache rows are the packed rows' k / v,
    the rest is untouched, and a per-row append step equals ``attn_decode`` row by row."""
    H, Gk, hd, Tmax = 4, 2, 16, 12
    lens = [3, 0, 7, 1]
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(sum(lens), (H + 2 * Gk) * hd, generator=g)
    cu = torch.tensor([0, 3, 3, 10, 11], dtype=torch.int32)
    kc = torch.full((4, Gk, Tmax, hd), 7.0)
    vc = torch.full((4, Gk, Tmax, hd), -7.0)
    ref.kv_cache_fill_varlen(qkv, cu, kc, vc)
    rows = qkv.view(-1, H + 2 * Gk, hd)
    for b, n in enumerate(lens):
        r0 = int(cu[b])
        assert torch.equal(kc[b, :, :n], rows[r0:r0 + n, H:H + Gk].transpose(0, 1))
        assert torch.equal(vc[b, :, :n], rows[r0:r0 + n, H + Gk:].transpose(0, 1))
        assert (kc[b, :, n:] == 7.0).all() and (vc[b, :, n:] == -7.0).all()
    step = torch.randn(4, (H + 2 * Gk) * hd, generator=g)
    pos = torch.tensor(lens, dtype=torch.int32)
    k0, v0 = kc.clone(), vc.clone()
    out = ref.attn_decode_append_rows(step, kc, vc, pos, H, Gk)
    sv = step.view(4, H + 2 * Gk, hd)
    for b, n in enumerate(lens):
        assert torch.equal(kc[b, :, n], sv[b, H:H + Gk]) and torch.equal(vc[b, :, n], sv[b, H + Gk:])
        keep = torch.arange(Tmax) != n
        assert torch.equal(kc[b][:, keep], k0[b][:, keep]) and torch.equal(vc[b][:, keep], v0[b][:, keep])
        want = ref.attn_decode(sv[b:b + 1, :H], kc[b:b + 1], vc[b:b + 1], n + 1)
        assert torch.equal(out[b:b + 1], want)


# ------------------------------------------------------------------ teacher forcing
@pytest.mark.parametrize("name", ["llama", "gpt2", "llama_lora"])
def test_ragged_prefill_and_row_steps_match_full_forward(name):
    """Prompts of 1, 5, 24 and 9 tokens prefilled in one packed pass, then 6 per-row decode steps
    on a fixed token stream: every logits row equals the full forward of that row's sequence at
    that position (the fp32 tolerance of test_model_grads.py's last-only-vs-full comparison)."""
    m = _model(name)
    lens, steps = [1, 5, 24, 9], 6
    full = _streams(lens, steps)
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, lens)], "cpu")
    assert seq.bounds == [0, 1, 6, 30, 39] and seq.max_len == 24 and idx.shape == (39,)
    with torch.no_grad():
        want = [m(f[None])[0] for f in full]
        cache = m.new_kv_cache(len(lens), CTX)
        got = [m.forward_prefill_ragged(idx, seq, cache)]
        pos = torch.tensor(lens, dtype=torch.int32)
        for s in range(steps):
            tok = torch.stack([f[n + s] for f, n in zip(full, lens)])[:, None]
            got.append(m.forward_cached_rows(tok, cache, pos))
            pos += 1
    for s, lg in enumerate(got):
        assert lg.shape == (len(lens), VOCAB)
        for b, n in enumerate(lens):
            assert torch.allclose(lg[b], want[b][n - 1 + s], atol=1e-5), (s, b)


def test_ragged_prefill_refuses_what_does_not_fit_the_cache():
    m = _model("llama")
    idx, seq = pack_prompts([torch.arange(5), torch.arange(3)], "cpu")
    with pytest.raises(ValueError, match="do not fit"):
        m.forward_prefill_ragged(idx, seq, m.new_kv_cache(2, 4))       # 5 tokens, 4 positions
    with pytest.raises(ValueError, match="do not fit"):
        m.forward_prefill_ragged(idx, seq, m.new_kv_cache(3, CTX))     # 2 sequences, 3 cache rows


# ------------------------------------------------------------------ generate_ragged
PROMPT_LENS = [1, 5, 24, 9]


def _prompts():
    return [f for f in _streams(PROMPT_LENS, 0)]


def _one_row(m, p, new, **kw):
    return G.generate_cached(m, p[None], new, CTX, **kw)[0]


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_ragged_greedy_equals_one_row_runs(name):
    m = _model(name)
    prompts = _prompts()
    # the premise: no step of a one-row run has a runner-up within 1e-3 of the argmax (GEMM
    # rounding differs by ~1e-6 between a 1-row and a 4-row batch), so the tokens are comparable
    for p in prompts:
        seq = _one_row(m, p, 12)
        with torch.no_grad():
            top = m(seq[None])[0, p.numel() - 1:-1].topk(2, dim=-1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
    res = G.generate_ragged(m, prompts, 12, CTX)
    assert len(res) == len(prompts)
    for p, r in zip(prompts, res):
        assert r.dtype == torch.long and torch.equal(r, _one_row(m, p, 12))


def test_generate_ragged_sampling_is_seeded():
    m = _model("llama")
    a, b = (G.generate_ragged(m, _prompts(), 12, CTX, temperature=1.0, top_k=5,
                              generator=torch.Generator().manual_seed(3)) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(x.numel() == n + 12 for x, n in zip(a, PROMPT_LENS))


@pytest.mark.parametrize("check_every", [1, 16])
def test_generate_ragged_rows_stop_on_their_own_eos(check_every, monkeypatch):
    """``eos_id`` = a token row 0 emits early: that row's result ends before it, a row that never
    emits it is what it was without eos, a row that emits it later is cut there; once every row
    has emitted it the loop stops (fewer decode steps than tokens asked for)."""
    monkeypatch.setattr(G, "EOS_CHECK_EVERY", check_every)
    m = _model("llama")
    prompts, new = _prompts(), 24
    free = G.generate_ragged(m, prompts, new, CTX)
    gen = [f[n:] for f, n in zip(free, PROMPT_LENS)]
    assert all(g.numel() == new for g in gen)
    eos = int(gen[0][2])                       # row 0's third token
    steps = []
    fwd = m.forward_cached_rows
    monkeypatch.setattr(m, "forward_cached_rows", lambda *a: (steps.append(1), fwd(*a))[1], raising=False)
    got = G.generate_ragged(m, prompts, new, CTX, eos_id=eos)
    first = [(g == eos).nonzero() for g in gen]
    want = [g[:int(f[0])] if f.numel() else g for g, f in zip(gen, first)]
    assert want[0].numel() <= 2
    for b, (p, w) in enumerate(zip(prompts, want)):
        assert torch.equal(got[b], torch.cat((p, w))), b
    assert len(steps) <= new - 1
    # a batch of the rows that emit it within 15 tokens (row 0 at least): the loop ends at the first
    # check after the last of them has, one decode step per token sampled before that
    hit = [b for b, f in enumerate(first) if f.numel() and int(f[0]) < 15]
    assert 0 in hit
    steps.clear()
    cut = G.generate_ragged(m, [prompts[b] for b in hit], new, CTX, eos_id=eos)
    for b, r in zip(hit, cut):
        assert torch.equal(r, torch.cat((prompts[b], want[b]))), b
    sampled = max(int(first[b][0]) for b in hit) + 1       # tokens up to and including the last row's eos
    stop = -(-sampled // check_every) * check_every
    assert len(steps) == stop - 1 < new - 1


def test_generate_ragged_results_do_not_depend_on_check_interval(monkeypatch):
    m = _model("gpt2")
    prompts = _prompts()
    free = G.generate_ragged(m, prompts, 24, CTX)
    eos = int(free[1][PROMPT_LENS[1] + 1])
    runs = []
    for every in (1, 16):
        monkeypatch.setattr(G, "EOS_CHECK_EVERY", every)
        runs.append(G.generate_ragged(m, prompts, 24, CTX, eos_id=eos))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert runs[0][1].numel() <= PROMPT_LENS[1] + 1


def test_generate_ragged_refusals():
    m = _model("llama")
    p = torch.arange(5)
    with pytest.raises(ValueError, match="non-empty list"):
        G.generate_ragged(m, [], 4, CTX)
    with pytest.raises(ValueError, match="prompt 1"):
        G.generate_ragged(m, [p, torch.zeros(0, dtype=torch.long)], 4, CTX)
    with pytest.raises(ValueError, match="prompt 0"):
        G.generate_ragged(m, [p[None]], 4, CTX)                          # not 1-D
    with pytest.raises(ValueError, match=r"30 tokens.*19.*48"):
        G.generate_ragged(m, [p, torch.arange(30)], 19, CTX)            # 30 + 19 > 48
    with pytest.raises(ValueError, match="model's context length"):
        G.generate_ragged(m, [p], 4, CTX + 1)
    assert G.generate_ragged(m, [p, torch.arange(30)], 18, CTX)[1].numel() == 48   # exactly full
    assert torch.equal(G.generate_ragged(m, [p], 0, CTX)[0], p)


# ------------------------------------------------------------------ command line
ENTRIES = [
    "Every effort moves you",
    {"instruction": "Name a colour.", "input": "", "output": "Blue."},
    {"instruction": "Add the numbers.", "input": "2 and 3", "output": "5", "id": 17},
    "Hi",
]


@pytest.fixture
def roomy_debug(monkeypatch):
    """``--debug`` fixes the context at 10 tokens, shorter than any Alpaca prompt under the offline
    byte tokenizer; the command-line tests keep every other ``--debug`` size and give it 256."""
    dbg = builder.debug_config
    monkeypatch.setattr(builder, "debug_config", lambda cfg: dbg(cfg).replace(context_length=256))


def _argv(tmp_path, model, extra):
    size = {"GPT2": "124M", "llama3_2": "1B"}[model]
    return (["--model", model, "--num_params", size, "--debug", "--device", "cpu", "--no_plot", "--batch_size", "2",
             "--output_dir", str(tmp_path / "out"), "--data_dir", str(tmp_path / "data"), "--num_workers", "0",
             "--generate_max_tokens", "5"] + extra)


def _check_rows(path, n_tokens=5):
    from building_llm_from_scratch_amd.data.datasets import format_input
    rows = json.load(open(path))
    assert len(rows) == len(ENTRIES)
    for it, row in zip(ENTRIES, rows):                      # input order, an entry's own fields kept
        if isinstance(it, str):
            assert row["prompt"] == it and set(row) == {"prompt", "response"}
        else:
            assert row["prompt"] == format_input(it) + "\n\n### Response:\n"
            assert all(row[k] == v for k, v in it.items())
        assert isinstance(row["response"], str)
    return rows


@pytest.mark.parametrize("model", ["GPT2", "llama3_2"])
def test_cli_generate_only(model, tmp_path, roomy_debug, monkeypatch):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(ENTRIES))
    tr = cli.cli(_argv(tmp_path, model, ["--generate_only", "--generate_prompts", str(pf)]))
    _check_rows(tmp_path / "out" / "responses.json")
    assert tr.global_step == -1 and not (tmp_path / "out" / "model_pg_final.pth").exists()   # nothing trained or saved
    assert not (tmp_path / "data").exists()                                                 # no data prepared
    # the same answers from the public method, whatever the batch size
    _, texts = cli.load_generate_prompts(pf)
    rows = json.load(open(tmp_path / "out" / "responses.json"))
    assert tr.generate_responses(texts, 5, 3) == [r["response"] for r in rows]
    # input order, with answers that tell the prompts apart: the byte tokenizer decodes the ids a
    # random-init model emits (mostly >= 256) to nothing, so decode to the ids themselves and compare
    # with each prompt's own one-row run
    tok, cfg = tr.loaderObj.tokenizer, tr.config
    monkeypatch.setattr(tok, "decode", lambda ids: " ".join(str(i) for i in ids), raising=False)
    want = []
    for t in texts:
        p = torch.tensor(tok.encode(t, allowed_special={cfg["eos_text"]}), dtype=torch.long)
        one = G.generate_cached(tr.model, p[None], 5, cfg["context_length"], eos_id=cfg["eos_id"])
        want.append(tok.decode(one[0, p.numel():].tolist()))
    assert len(set(want)) > 1
    assert tr.generate_responses(texts, 5, 3) == want == tr.generate_responses(texts, 5, 1)


def test_cli_generate_after_finetune(tmp_path, roomy_debug):
    pf, out = tmp_path / "prompts.json", tmp_path / "answers" / "r.json"
    pf.write_text(json.dumps(ENTRIES))
    tr = cli.cli(_argv(tmp_path, "llama3_2", ["--finetune", "--dataset", "alpaca", "--synthetic_data", "--max_steps", "2",
                                              "--n_epochs", "1", "--eval_freq", "100", "--print_sample_iter", "100",
                                              "--sample_tokens", "2", "--skip_final_save", "--generate_prompts", str(pf),
                                              "--generate_out", str(out)]))
    assert tr.global_step >= 1
    _check_rows(out)


def test_cli_generate_refusals(tmp_path, roomy_debug):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(ENTRIES))
    with pytest.raises(ValueError, match="--generate_only needs --generate_prompts"):
        cli.get_args(["--data_dir", str(tmp_path), "--generate_only"])
    with pytest.raises(FileNotFoundError):
        cli.get_args(["--data_dir", str(tmp_path), "--generate_prompts", str(tmp_path / "nope.json")])
    with pytest.raises(ValueError, match="--generate_max_tokens"):
        cli.get_args(["--data_dir", str(tmp_path), "--generate_prompts", str(pf), "--generate_max_tokens", "0"])
    # --generate_only reads no training data: a missing --data_dir is not an error there
    a = cli.get_args(["--data_dir", str(tmp_path / "nope"), "--generate_only", "--generate_prompts", str(pf)])
    assert a.generate_out is None and a.generate_max_tokens == 256
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps(["ok", {"text": "no instruction"}]))
    with pytest.raises(ValueError, match="item 1"):
        cli.load_generate_prompts(bad)
    # a prompt that does not fit context_length - generate_max_tokens: refused by index, before generation
    with pytest.raises(ValueError, match="prompt 1 "):
        cli.cli(_argv(tmp_path, "llama3_2", ["--generate_only", "--generate_prompts", str(pf),
                                             "--generate_max_tokens", "200"]))
    assert not os.path.exists(tmp_path / "out" / "responses.json")
