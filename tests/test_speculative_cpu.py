"""Exact speculative decoding (prompt lookup) on the CPU in fp32: the ``spec_advance`` oracle on
hand-written rows, the Q-token model step against the full forward, ``generate_ragged(speculative=K)``
token for token against the plain loop (greedy and seeded, with and without hints and eos), its
step counts against a simulation on the returned tokens, the refusals and the command line."""
import json

import pytest
import torch

import speculative_cases as S
from test_generate_ragged_cpu import CTX, ENTRIES, VOCAB, _argv, _model, _streams, roomy_debug  # noqa: F401

from building_llm_from_scratch_amd import cli
from building_llm_from_scratch_amd.models.base import pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G


# ------------------------------------------------------------------ spec_advance oracle
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_spec_advance_oracle_on_hand_written_rows(name):
    r = S.CASES[name]
    S.check_case(S.run_rows(ref.spec_advance, [r]), 0, r)


def test_spec_advance_oracle_rows_are_independent():
    """The draft-only cases as one batch: every row as alone."""
    rows = [r for _, r in sorted(S.CASES.items()) if not r["accept"]]
    st = S.run_rows(ref.spec_advance, rows)
    for b, r in enumerate(rows):
        S.check_case(st, b, r)


# ------------------------------------------------------------------ the Q-token model step
@pytest.mark.parametrize("Q", [2, 4, 8])
@pytest.mark.parametrize("name", ["llama", "gpt2", "llama_lora"])
def test_q_token_steps_match_full_forward(name, Q):
    """Prompts of 1, 5, 24 and 9 tokens prefilled, then two steps of Q tokens per row on a fixed
    token stream: logits row b*Q + j equals the full forward of row b's sequence at that position
    (the comparison of test_ragged_prefill_and_row_steps_match_full_forward)."""
    m = _model(name)
    lens, steps = [1, 5, 24, 9], 2
    full = _streams(lens, steps * Q)
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, lens)], "cpu")
    with torch.no_grad():
        want = [m(f[None])[0] for f in full]
        cache = m.new_kv_cache(len(lens), CTX)
        m.forward_prefill_ragged(idx, seq, cache)
        pos = torch.tensor(lens, dtype=torch.int32)
        for s in range(steps):
            tok = torch.stack([f[n + s * Q:n + (s + 1) * Q] for f, n in zip(full, lens)]).reshape(-1, 1)
            pos_rows = (pos[:, None] + torch.arange(Q, dtype=torch.int32)).reshape(-1)
            lg = m.forward_cached_rows(tok, cache, pos_rows, q_per_row=Q)
            assert lg.shape == (len(lens) * Q, VOCAB)
            for b, n in enumerate(lens):
                for j in range(Q):
                    assert torch.allclose(lg[b * Q + j], want[b][n + s * Q + j], atol=1e-5), (s, b, j)
            pos += Q


def test_q_token_step_refusals():
    m = _model("llama")
    cache = m.new_kv_cache(2, CTX)
    tok, pos_rows = torch.zeros(4, 1, dtype=torch.long), torch.tensor([3, 4, 5, 6], dtype=torch.int32)
    with pytest.raises(ValueError, match="q_per_row"):
        m.forward_cached_rows(tok, cache, pos_rows, q_per_row=3)            # 4 rows, 3 per row
    with pytest.raises(ValueError, match="fp8 cache"):
        m.forward_cached_rows(tok, m.new_kv_cache(2, CTX, kv_dtype="fp8"), pos_rows, q_per_row=2)
    with pytest.raises(ValueError, match="weights"):
        m.forward_cached_rows(tok, cache, pos_rows, weights=m.new_decode_weights(), q_per_row=2)


# ------------------------------------------------------------------ generate_ragged(speculative=K)
PROMPT_LENS = [1, 5, 24, 9]
NEW = 12
MODES = {"greedy": {}, "seeded": dict(temperature=0.8, top_k=20, top_p=0.9, seed=11)}
_PLAIN = {}


def _prompts():
    return _streams(PROMPT_LENS, 0)


def _plain(name, mode):
    """The plain run of a (model, sampling mode), computed once, with its premise checked: no
    step's sampler gap (top key minus runner-up; the logit gap when greedy) is below 1e-4, so GEMM
    rounding between a 1-token and a Q-token step cannot change a token."""
    if (name, mode) not in _PLAIN:
        m, kw = _model(name), MODES[mode]
        res = G.generate_ragged(m, _prompts(), NEW, CTX, **kw)
        for b, (r, n) in enumerate(zip(res, PROMPT_LENS)):
            assert r.numel() == n + NEW
            with torch.no_grad():
                lg = m(r[None])[0, n - 1:-1]
            for c in range(NEW):
                if kw:
                    tok, _, info = ref.sample_rows_detail(lg[c:c + 1], torch.tensor([b]), torch.tensor([c], dtype=torch.int32),
                                                          kw["seed"], kw["temperature"], kw["top_k"], kw["top_p"])
                    assert int(tok[0]) == int(r[n + c]) and info[0]["gap"] >= 1e-4, (b, c, info[0]["gap"])
                else:
                    top = lg[c].topk(2).values
                    assert int(lg[c].argmax()) == int(r[n + c]) and float(top[0] - top[1]) >= 1e-4, (b, c)
        _PLAIN[(name, mode)] = res
    return _PLAIN[(name, mode)]


def _hints(name, mode, kind):
    plain = _plain(name, mode)
    if kind == "none":
        return None
    hints = [torch.cat((p, r[p.numel():])) for p, r in zip(_prompts(), plain)]   # = the plain result
    if kind == "corrupt":
        for h in hints:                      # two places inside the answer part
            h[-3] = (int(h[-3]) + 1) % VOCAB
            h[-8] = (int(h[-8]) + 1) % VOCAB
    return hints


@pytest.mark.parametrize("kind", ["none", "self", "corrupt"])
@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("mode", ["greedy", "seeded"])
@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_speculative_tokens_equal_plain(name, mode, K, kind):
    m = _model(name)
    plain = _plain(name, mode)
    st = {}
    got = G.generate_ragged(m, _prompts(), NEW, CTX, speculative=K, draft_hints=_hints(name, mode, kind), stats=st,
                            **MODES[mode])
    for b, (a, w) in enumerate(zip(got, plain)):
        assert a.dtype == torch.long and torch.equal(a, w), b
    assert st["new_tokens"] == [NEW] * len(plain)
    # step counts: a function of the returned tokens alone
    hints = _hints(name, mode, kind) or [torch.zeros(0, dtype=torch.long)] * len(plain)
    sims = [S.simulate(p.tolist(), r[p.numel():].tolist(), h.tolist(), K, G.SPEC_NGRAM)
            for p, r, h in zip(_prompts(), got, hints)]
    assert st["steps"] == [len(s) for s in sims]
    if kind == "self":
        # the condition of the step-count check: drafts are accepted in every row, all K somewhere
        assert all(sum(s) >= 1 for s in sims) and any(a == K for s in sims for a in s)
        assert max(st["steps"]) < NEW - 1


@pytest.mark.parametrize("mode", ["greedy", "seeded"])
@pytest.mark.parametrize("kind", ["none", "self"])
def test_speculative_with_an_eos_some_row_hits(mode, kind, monkeypatch):
    """eos = row 0's fourth token: rows that emit it end there (inside a run of accepted drafts
    when hinted), the others are what they are without it."""
    monkeypatch.setattr(G, "EOS_CHECK_EVERY", 2)
    m = _model("llama")
    plain = _plain("llama", mode)
    eos = int(plain[0][PROMPT_LENS[0] + 3])
    want = G.generate_ragged(m, _prompts(), NEW, CTX, eos_id=eos, **MODES[mode])
    assert want[0].numel() <= PROMPT_LENS[0] + 3
    for K in (1, 3, 7):
        st = {}
        got = G.generate_ragged(m, _prompts(), NEW, CTX, eos_id=eos, speculative=K, stats=st,
                                draft_hints=_hints("llama", mode, kind), **MODES[mode])
        assert all(torch.equal(a, w) for a, w in zip(got, want))
        hints = _hints("llama", mode, kind) or [torch.zeros(0, dtype=torch.long)] * len(want)
        for b, (p, r, h) in enumerate(zip(_prompts(), got, hints)):
            ans = r[p.numel():].tolist()
            ans = ans + [eos] if len(ans) < NEW else ans          # a short row drew its eos last
            assert st["new_tokens"][b] == len(ans)
            assert st["steps"][b] == len(S.simulate(p.tolist(), ans, h.tolist(), K, G.SPEC_NGRAM)), (K, b)


def test_speculative_refusals():
    m = _model("llama")
    p = [torch.arange(5), torch.arange(30)]
    for K in (0, 8, -1, 2.0, True):
        with pytest.raises(ValueError, match="speculative must be"):
            G.generate_ragged(m, p, 4, CTX, speculative=K)
    with pytest.raises(ValueError, match="seed"):
        G.generate_ragged(m, p, 4, CTX, speculative=2, temperature=0.7)
    with pytest.raises(ValueError, match="kv_dtype"):
        G.generate_ragged(m, p, 4, CTX, speculative=2, kv_dtype="fp8")
    with pytest.raises(ValueError, match="weight_dtype"):
        G.generate_ragged(m, p, 4, CTX, speculative=2, weight_dtype="fp8")
    with pytest.raises(ValueError, match=r"30 tokens.*16.*speculative \(3\).*48"):
        G.generate_ragged(m, p, 16, CTX, speculative=3)                  # 30 + 16 + 3 > 48
    assert G.generate_ragged(m, p, 15, CTX, speculative=3)[1].numel() == 45          # exactly full
    with pytest.raises(ValueError, match="draft_hints belong"):
        G.generate_ragged(m, p, 4, CTX, draft_hints=[None, None])
    with pytest.raises(ValueError, match="one entry per prompt"):
        G.generate_ragged(m, p, 4, CTX, speculative=2, draft_hints=[None])
    with pytest.raises(ValueError, match="draft hint 1"):
        G.generate_ragged(m, p, 4, CTX, speculative=2, draft_hints=[None, torch.zeros(3)])
    st = {}
    assert torch.equal(G.generate_ragged(m, p[:1], 0, CTX, speculative=2, stats=st)[0], p[0]) and st["steps"] == [0]


# ------------------------------------------------------------------ command line
def test_cli_speculative_answers_are_the_plain_ones(tmp_path, roomy_debug):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(ENTRIES))
    base = ["--generate_only", "--generate_prompts", str(pf)]
    tr = cli.cli(_argv(tmp_path, "llama3_2", base))
    plain = json.load(open(tmp_path / "out" / "responses.json"))
    cli.cli(_argv(tmp_path, "llama3_2", base + ["--generate_speculative", "3", "--generate_out",
                                                  str(tmp_path / "spec.json")]))
    assert json.load(open(tmp_path / "spec.json")) == plain
    _, texts = cli.load_generate_prompts(pf)
    assert tr.generate_responses(texts, 5, 3, speculative=3) == [r["response"] for r in plain]
    with pytest.raises(ValueError, match="--generate_speculative must be"):
        cli.get_args(["--data_dir", str(tmp_path), "--generate_speculative", "8"])
    with pytest.raises(ValueError, match="--generate_speculative runs on"):
        cli.get_args(["--data_dir", str(tmp_path), "--generate_speculative", "2", "--generate_kv_dtype", "fp8"])
    with pytest.raises(ValueError, match="--generate_speculative runs on"):
        cli.get_args(["--data_dir", str(tmp_path), "--generate_speculative", "2", "--generate_weight_dtype", "fp8"])
