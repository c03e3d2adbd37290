"""FP8 decode weights without a GPU: the pack format (``ops.w8_pack`` / ``w8_unpack`` against
``kv_quantize_rows``), the fp64 oracle ``ops.reference.linear_w8``, the LoRA fold of
``FusedLinear.w8_pack``, a model step on the packs against a twin model that holds the dequantised
weights, and the entry points (``weight_dtype`` / ``--generate_weight_dtype``)."""
import inspect
import json

import pytest
import torch
from numerics import check_close

from building_llm_from_scratch_amd import builder, cli, ops
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.models.base import DecodeWeights, pack_prompts
from building_llm_from_scratch_amd.models.lora import replace_linear_with_lora
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

F32, F8 = torch.float32, torch.float8_e4m3fn
TN, KG = ops.W8_ROW_TILE, ops.W8_K_GRANULE
CTX = 64


def _u8(t):
    return t.contiguous().view(torch.uint8)


def _same_pack(q, s, q0, s0):
    return q.dtype == F8 and q.shape == q0.shape and torch.equal(_u8(q), _u8(q0)) and \
        s.dtype == F32 and torch.equal(s.view(torch.int32), s0.view(torch.int32))


# ------------------------------------------------------------------ pack format
@pytest.mark.parametrize("K", [KG, 3 * KG])
@pytest.mark.parametrize("N", [1, TN - 1, TN, TN + 1, 97])
def test_pack_contract(N, K):
    g = torch.Generator().manual_seed(N * 1000 + K)
    W = torch.randn(N, K, generator=g)
    z = N // 2 if N > 1 else None                      # an all-zero row: scale 1, zero bytes
    if z is not None:
        W[z] = 0
    W[N - 1, 0], W[N - 1, K - 1] = 3.0e4, -3.0e4       # a row holding +max and -max
    pack = ops.w8_pack(W)
    assert isinstance(pack, ops.W8Pack) and pack.tiled and (pack.N, pack.K) == (N, K)
    assert pack.data.dtype == torch.uint8 and pack.data.numel() == -(-N // TN) * TN * K
    q, s = ops.w8_unpack(pack)
    q0, s0 = ref.kv_quantize_rows(W)
    assert _same_pack(q, s, q0, s0)
    assert z is None or (float(s[z]) == 1.0 and not _u8(q[z]).any())
    assert float(q[N - 1, 0].float()) == 448.0 and float(q[N - 1, K - 1].float()) == -448.0
    # the layout the kernel reads: tile t, block kb, lane 16 g + r, byte b
    t, kb, gq, r, b = (N - 1) // TN, K // KG - 1, 3, (N - 1) % TN, 15
    at = (((t * (K // KG) + kb) * 4 + gq) * TN + r) * 16 + b
    assert int(pack.data[at]) == int(_u8(q0)[N - 1, KG * kb + 16 * gq + b])
    # padding rows hold zero bytes
    rows = pack.data.view(-(-N // TN), K // KG, 4, TN, 16)[-1]
    assert not rows[:, :, (N - 1) % TN + 1:].any()


def test_pack_of_other_widths_runs_the_oracle():
    """K = 10 (``--debug``) is no multiple of the granule: the pack keeps the bytes row-major and
    ``linear_w8`` composes the oracle."""
    W, x = torch.randn(7, 10), torch.randn(3, 10)
    pack = ops.w8_pack(W)
    assert not pack.tiled
    q, s = ops.w8_unpack(pack)
    assert _same_pack(q, s, *ref.kv_quantize_rows(W))
    assert torch.equal(ops.linear_w8(x, pack), ref.linear_w8(x, q, s))
    with pytest.raises(ValueError, match="linear_w8"):
        ops.linear_w8(torch.randn(3, 11), pack)


# ------------------------------------------------------------------ oracle
def test_oracle_is_the_fp64_product():
    g = torch.Generator().manual_seed(1)
    W, x = torch.randn(37, 2 * KG, generator=g), torch.randn(5, 2 * KG, generator=g).double()
    bias, res = torch.randn(37, generator=g).double(), torch.randn(5, 37, generator=g).double()
    q, s = ref.kv_quantize_rows(W)
    base = x @ (q.double() * s.double()[:, None]).t()
    for b, r in ((None, None), (bias, None), (None, res), (bias, res)):
        want = base + (0 if b is None else b) + (0 if r is None else r)
        got = ref.linear_w8(x, q, s, b, r)
        assert got.dtype == torch.float64
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert ref.linear_w8(x.to(torch.bfloat16), q, s).dtype == torch.bfloat16
    assert torch.equal(ops.linear_w8(x.float(), ops.w8_pack(W), bias.float()), ref.linear_w8(x.float(), q, s, bias.float()))


# ------------------------------------------------------------------ models
def _cfgs():
    """The tiny models of tests/test_kv_fp8_gpu.py."""
    llama = get_config("llama3_2", "1B").replace(context_length=CTX, emb_dim=256, n_heads=4, n_kv_groups=2,
                                                 hidden_dim=384, n_layers=2, vocab_size=512, dtype=F32)
    gpt = get_config("GPT2", "124M").replace(context_length=CTX, emb_dim=256, n_heads=4, n_kv_groups=4, hidden_dim=1024,
                                             n_layers=2, vocab_size=512, drop_rate=0.0, dtype=F32)
    return {"llama": llama, "gpt2": gpt}


_MODELS = {}


def _model(name, lora=False, seed=0):
    key = (name, lora, seed)
    if key not in _MODELS:
        torch.manual_seed(seed)
        m = build_model(_cfgs()[name])
        if lora:
            replace_linear_with_lora(m, rank=16, alpha=32)
            with torch.no_grad():
                for n, p in m.named_parameters():
                    if n.endswith("lora.B"):
                        p.normal_(0.0, 0.02)
        m.flatten()
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


def _groups(m):
    return [fl for c in m.computes[1:-1] for fl in c.w8_groups()] + [m.computes[-1].head]


def _packs(w):
    return [p for blk in w.blocks for p in blk] + [w.head]


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_lora_fold(name):
    """The pack of a LoRA group is the quantised W + scaling (A B)^T, and ``forward_w8`` differs
    from ``forward`` by no more than the format allows: a dequantised weight is w (1 + d) with
    |d| <= 2^-4 (e4m3's three mantissa bits, half an ulp) or, below the smallest normal 2^-6 of the
    scaled row, off by half a subnormal step 2^-10 s -- the per-element error the FP8 KV cache
    documents -- so |y8 - y| <= sum_k |x| max(2^-4 |w_eff|, 2^-10 s) plus the fp32 rounding of the
    two computations."""
    m = _model(name, lora=True)
    w = m.new_decode_weights("fp8")
    x_g = torch.Generator().manual_seed(2)
    for fl, pk in zip(_groups(m), _packs(w)):
        assert fl.has_lora
        W_eff = fl.W().float().clone()
        for (c0, c1), s in zip(fl.cols, fl.specs):
            W_eff[c0:c1] += s.scaling * (fl.unit.data(s.lora_A).float() @ fl.unit.data(s.lora_B).float()).t()
        assert not torch.equal(W_eff, fl.W().float())
        q, s = ops.w8_unpack(pk.pack)
        assert _same_pack(q, s, *ref.kv_quantize_rows(W_eff))
        assert (pk.bias is None) == (fl.b() is None) and (pk.bias is None or torch.equal(pk.bias, fl.b()))
        x = torch.randn(6, W_eff.shape[1], generator=x_g)
        y, _ = fl.forward(x)
        y8 = fl.forward_w8(x, pk)
        bound = x.abs().double() @ torch.maximum(W_eff.abs().double() / 16, s.double()[:, None] / 1024).t()
        slack = 64 * 2.0 ** -24 * (x.abs().double() @ W_eff.abs().double().t() + 1.0)
        assert bool(((y8.double() - y.double()).abs() <= bound + slack).all())
        assert not torch.equal(y8, y)


def _dequantised_twin(name, m, w):
    """A second model with the same parameters whose projection weights are the dequantised packs."""
    twin = _model(name, seed=1)
    twin.load_state_dict(m.state_dict())
    with torch.no_grad():
        for fl, pk in zip(_groups(twin), _packs(w)):
            q, s = ops.w8_unpack(pk.pack)
            fl.W().copy_(ref.kv_dequantize(q, s))
    return twin


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_model_step_on_the_packs(name):
    """After one ragged prefill (exact weights), 4 teacher-forced ``forward_cached_rows`` steps with
    ``weights=`` against the twin that holds the dequantised weights, on a copy of the same cache."""
    m = _model(name)
    w = m.new_decode_weights("fp8")
    assert isinstance(w, DecodeWeights) and len(w.blocks) == 2 and all(len(b) == 4 for b in w.blocks)
    assert w.head.pack.N == 512 and all(p.pack.tiled for p in _packs(w))
    assert [p.bias is not None for p in _packs(w)] == [fl.b() is not None for fl in _groups(m)]
    assert (w.blocks[0][3].bias is not None) == (name == "gpt2")
    twin = _dequantised_twin(name, m, w)
    lens, steps = [1, 7, 40, 13], 4
    g = torch.Generator().manual_seed(5)
    full = [torch.randint(0, 512, (n + steps,), generator=g) for n in lens]
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, lens)], "cpu")
    with torch.no_grad():
        cache = m.new_kv_cache(len(lens), CTX)
        first = m.forward_prefill_ragged(idx, seq, cache)
        cache_t = [tuple(t.clone() for t in kv) for kv in cache]
        cache_e = [tuple(t.clone() for t in kv) for kv in cache]
        pos, pos_t, pos_e = (torch.tensor(lens, dtype=torch.int32) for _ in range(3))
        assert not torch.equal(twin.forward_prefill_ragged(idx, seq, twin.new_kv_cache(len(lens), CTX)), first)
        for s in range(steps):
            tok = torch.stack([f[n + s] for f, n in zip(full, lens)])[:, None]
            got = m.forward_cached_rows(tok, cache, pos, weights=w)
            want = twin.forward_cached_rows(tok, cache_t, pos_t)
            exact = m.forward_cached_rows(tok, cache_e, pos_e)
            check_close(got, want.double(), F32, name=f"{name} step {s} on the packs")
            assert not torch.equal(got, exact)
            pos += 1
            pos_t += 1
            pos_e += 1
    with pytest.raises(ValueError, match="new_decode_weights"):
        m.forward_cached_rows(tok, cache, pos - 1, weights=w.blocks)


# ------------------------------------------------------------------ entry points
def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (n,), generator=g) for n in (5, 24, 9)]


def test_generate_ragged_weight_dtype(monkeypatch):
    m = _model("llama")
    prompts, new = _prompts(), 6
    with pytest.raises(ValueError, match="weight_dtype"):
        G.generate_ragged(m, prompts, new, CTX, weight_dtype="int4")
    with pytest.raises(ValueError, match="weight_dtype"):
        m.new_decode_weights("bf16")
    built = []
    real = m.new_decode_weights
    monkeypatch.setattr(m, "new_decode_weights", lambda *a, **k: built.append(1) or real(*a, **k))
    batch = G.generate_ragged(m, prompts, new, CTX, weight_dtype="fp8", kv_dtype="fp8")
    assert built == [1]
    for p, r in zip(prompts, batch):
        assert r.numel() == p.numel() + new and torch.equal(r[:p.numel()], p)
    w = real("fp8")
    a = G.generate_ragged(m, prompts, new, CTX, weight_dtype=w, temperature=0.8, top_k=20, seed=3)
    b = G.generate_ragged(m, prompts, new, CTX, weight_dtype="fp8", temperature=0.8, top_k=20, seed=3)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and built == [1, 1]
    # the first new token comes from the prefill on the exact weights
    default = G.generate_ragged(m, prompts, new, CTX)
    packed = G.generate_ragged(m, prompts, new, CTX, weight_dtype=w)
    assert all(int(x[p.numel()]) == int(y[p.numel()]) for p, x, y in zip(prompts, default, packed))
    assert all(torch.equal(x, y) for x, y in zip(default, G.generate_ragged(m, prompts, new, CTX, weight_dtype=None)))


def test_fixed_position_paths_do_not_take_the_pack():
    m = _model("llama")
    w = m.new_decode_weights("fp8")
    cache = m.new_kv_cache(1, CTX)
    idx = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises((TypeError, ValueError)):
        m.forward_cached(idx, cache, 0, weights=w)
    with pytest.raises((TypeError, ValueError)):
        m.forward_cached_dev(idx[:, :1], cache, torch.zeros(1, dtype=torch.int32), weights=w)
    with pytest.raises((TypeError, ValueError)):
        G.generate_cached(m, idx, 2, CTX, weight_dtype="fp8")
    assert "weight_dtype" not in inspect.signature(G.generate_cached).parameters


@pytest.fixture
def roomy_debug(monkeypatch):
    """``--debug`` with a context of 256 tokens (tests/test_generate_ragged_cpu.py)."""
    dbg = builder.debug_config
    monkeypatch.setattr(builder, "debug_config", lambda cfg: dbg(cfg).replace(context_length=256))


def test_cli_flag_parsing(tmp_path):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(["Hi"]))
    base = ["--data_dir", str(tmp_path), "--generate_prompts", str(pf)]
    assert cli.get_args(base).generate_weight_dtype == "model"
    a = cli.get_args(base + ["--generate_weight_dtype", "fp8", "--generate_kv_dtype", "fp8", "--generate_temperature",
                             "0.7", "--generate_top_k", "5"])
    assert a.generate_weight_dtype == "fp8" and a.generate_kv_dtype == "fp8"
    with pytest.raises(ValueError, match="--generate_weight_dtype"):
        cli.get_args(base + ["--generate_weight_dtype", "int4"])


def test_generate_responses_builds_one_pack(tmp_path, roomy_debug, monkeypatch):
    """``--generate_weight_dtype fp8`` end to end on the CPU (``--debug``: K = 10, the oracle path),
    and three batches of ``generate_responses`` share one pack."""
    pf = tmp_path / "prompts.json"
    entries = ["Every effort moves you", {"instruction": "Name a colour.", "input": "", "output": "Blue."}, "Hi"]
    pf.write_text(json.dumps(entries))
    argv = ["--model", "llama3_2", "--num_params", "1B", "--debug", "--device", "cpu", "--no_plot", "--batch_size", "1",
            "--output_dir", str(tmp_path / "out"), "--data_dir", str(tmp_path / "data"), "--num_workers", "0",
            "--generate_max_tokens", "5", "--generate_only", "--generate_prompts", str(pf),
            "--generate_weight_dtype", "fp8"]
    tr = cli.cli(argv)
    rows = json.load(open(tmp_path / "out" / "responses.json"))
    assert len(rows) == len(entries) and all(isinstance(r["response"], str) for r in rows)
    _, texts = cli.load_generate_prompts(pf)
    built, seen = [], []
    real_new, real_gen = tr.model.new_decode_weights, G.generate_ragged
    monkeypatch.setattr(tr.model, "new_decode_weights", lambda *a, **k: built.append(1) or real_new(*a, **k))

    def spy(*a, **kw):
        seen.append(kw.get("weight_dtype"))
        return real_gen(*a, **kw)

    from building_llm_from_scratch_amd.train import trainer as T
    monkeypatch.setattr(T, "generate_ragged", spy)
    assert tr.generate_responses(texts, 5, 1, weight_dtype="fp8") == [r["response"] for r in rows]
    assert built == [1] and len(seen) == 3 and all(isinstance(s, DecodeWeights) and s is seen[0] for s in seen)
    tr.generate_responses(texts, 5, 1)
    assert built == [1] and all(s is None for s in seen[3:])
    with pytest.raises(ValueError, match="weight_dtype"):
        tr.generate_responses(texts, 5, 1, weight_dtype="int4")
