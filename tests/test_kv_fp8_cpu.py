"""FP8 KV cache on the CPU: the format's round-trip bound, the oracles of the quantised fill and
append + decode step, ``generate_ragged(kv_dtype="fp8")`` on tiny fp32 models, the refusals of
the paths that keep the cache in the activation dtype, and the command-line flag."""
import json

import pytest
import torch

from building_llm_from_scratch_amd import builder, cli, ops
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.models.base import cached_attention, pack_prompts
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

F8 = torch.float8_e4m3fn
CTX, VOCAB = 48, 97


def _u8(t):
    return t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------ the format
def _rows(scale, dt, outlier, g, n=64, hd=64):
    x = torch.randn(n, hd, generator=g) * scale
    if outlier:
        x[torch.arange(n), torch.randint(0, hd, (n,), generator=g)] *= 100.0
    big = torch.finfo(dt).max                  # fp16 at scale 3e4: the few values past 65,504 sit at it
    return x.clamp(-big, big).to(dt)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("outlier", [False, True])
def test_round_trip_bound(dt, outlier):
    """|deq - x| <= max(2^-4 |x|, 2^-10 s) (1 + 2^-20) for every element: e4m3 has 3 mantissa bits
    (half an ulp is 2^-4 relative) and subnormal spacing 2^-9 (half of it 2^-10, in units of s);
    the factor covers the fp32 rounding of the quotient and of the product."""
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for scale in (1e-3, 1.0, 50.0, 3e4):
        x = _rows(scale, dt, outlier, g)
        assert torch.isfinite(x.float()).all()
        q, s = ops.kv_quantize_rows(x)
        assert q.dtype == F8 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == x.shape[:-1]
        want_s = (x.float().abs().amax(-1).double() / 448.0).float()
        assert torch.equal(s, want_s)
        d = ops.kv_dequantize(q, s)
        assert d.dtype == torch.float32 and torch.isfinite(d).all()
        x64, d64, s64 = x.double(), d.double(), s.double()[:, None]
        bound = torch.maximum(2.0 ** -4 * x64.abs(), 2.0 ** -10 * s64) * (1 + 2.0 ** -20)
        err = (d64 - x64).abs()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (scale, float((err / bound).max()))
        # the row maximum maps to +-448 exactly
        assert (q.float().abs().amax(-1) == 448.0).all()
    print(f"round trip {dt} outlier {outlier}: worst error / bound {worst:.4f}")


def test_zero_row_and_exact_values():
    x = torch.zeros(3, 64)
    x[1] = torch.randn(64)
    q, s = ops.kv_quantize_rows(x)
    assert s[0] == 1.0 and s[2] == 1.0 and (_u8(q[0]) == 0).all() and (_u8(q[2]) == 0).all()
    assert torch.isfinite(ops.kv_dequantize(q, s)).all() and (ops.kv_dequantize(q, s)[0] == 0).all()
    # every finite e4m3 value times a power-of-two scale, a row holding +-448: bitwise round trip
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    vals = codes.view(F8).float()
    for sc in (1.0, 2.0 ** -7, 2.0 ** 9):
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            xr = (vals * sc).to(dt)[None]
            if not torch.isfinite(xr.float()).all() or not torch.equal(xr.float(), vals[None] * sc):
                continue                                # not representable in dt at this scale
            q, s = ops.kv_quantize_rows(xr)
            assert float(s[0]) == sc
            d = ops.kv_dequantize(q, s, dt)
            assert d.dtype == dt and torch.equal(d.float(), xr.float())
            nz = vals != 0
            assert torch.equal(_u8(q)[0][nz], codes[nz])


# ------------------------------------------------------------------ oracle semantics
def _fp8_cache(B, Gk, Tmax, hd, g):
    """A cache with every slot holding a valid quantised random row."""
    k8, ks = ops.kv_quantize_rows(torch.randn(B, Gk, Tmax, hd, generator=g))
    v8, vs = ops.kv_quantize_rows(torch.randn(B, Gk, Tmax, hd, generator=g) * 3.0)
    return k8, v8, ks, vs


def test_oracle_append_rows():
    H, Gk, hd, Tmax = 4, 2, 16, 12
    g = torch.Generator().manual_seed(2)
    pos = [3, 0, 7, 11]
    B = len(pos)
    k8, v8, ks, vs = _fp8_cache(B, Gk, Tmax, hd, g)
    before = [t.clone() for t in (k8, v8, ks, vs)]
    step = torch.randn(B, (H + 2 * Gk) * hd, generator=g)
    pos_t = torch.tensor(pos, dtype=torch.int32)
    out = ops.attn_decode_append_rows(step, k8, v8, pos_t, H, Gk, scales=(ks, vs))
    sv = step.view(B, H + 2 * Gk, hd)
    for b, p in enumerate(pos):
        for c8, cs, src in ((k8, ks, sv[b, H:H + Gk]), (v8, vs, sv[b, H + Gk:])):
            q, s = ops.kv_quantize_rows(src)
            assert torch.equal(_u8(c8[b, :, p]), _u8(q)) and torch.equal(cs[b, :, p], s)
        keep = torch.arange(Tmax) != p
        for now, was in zip((k8, v8, ks, vs), before):
            assert torch.equal(_u8(now[b][:, keep]), _u8(was[b][:, keep]))
    # the existing reference on the dequantised cache (its own append of the dequantised new row
    # rewrites the same values)
    kd, vd = ops.kv_dequantize(k8, ks), ops.kv_dequantize(v8, vs)
    deq_step = step.clone().view(B, H + 2 * Gk, hd)
    for b, p in enumerate(pos):
        deq_step[b, H:H + Gk] = kd[b, :, p]
        deq_step[b, H + Gk:] = vd[b, :, p]
    want = ref.attn_decode_append_rows(deq_step.view(B, -1), kd, vd, pos_t, H, Gk)
    assert torch.equal(out, want)


def test_oracle_fill():
    H, Gk, hd, Tmax = 4, 2, 16, 12
    lens = [3, 0, 7, 1]
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(sum(lens), (H + 2 * Gk) * hd, generator=g)
    cu = torch.tensor([0, 3, 3, 10, 11], dtype=torch.int32)
    k8 = torch.full((4, Gk, Tmax, hd), 0x55, dtype=torch.uint8).view(F8)
    v8 = torch.full((4, Gk, Tmax, hd), 0x2A, dtype=torch.uint8).view(F8)
    ks, vs = torch.full((4, Gk, Tmax), 7.0), torch.full((4, Gk, Tmax), -7.0)
    ops.kv_cache_fill_varlen(qkv, cu, k8, v8, scales=(ks, vs))
    rows = qkv.view(-1, H + 2 * Gk, hd)
    for b, n in enumerate(lens):
        r0 = int(cu[b])
        qk, sk = ops.kv_quantize_rows(rows[r0:r0 + n, H:H + Gk].transpose(0, 1))
        qv, sv = ops.kv_quantize_rows(rows[r0:r0 + n, H + Gk:].transpose(0, 1))
        assert torch.equal(_u8(k8[b, :, :n]), _u8(qk)) and torch.equal(ks[b, :, :n], sk)
        assert torch.equal(_u8(v8[b, :, :n]), _u8(qv)) and torch.equal(vs[b, :, :n], sv)
        assert (_u8(k8[b, :, n:]) == 0x55).all() and (_u8(v8[b, :, n:]) == 0x2A).all()
        assert (ks[b, :, n:] == 7.0).all() and (vs[b, :, n:] == -7.0).all()


def test_ops_refuse_mismatched_scales():
    H, Gk, hd, Tmax = 2, 1, 16, 4
    k8, v8, ks, vs = _fp8_cache(1, Gk, Tmax, hd, torch.Generator().manual_seed(0))
    step = torch.randn(1, (H + 2 * Gk) * hd)
    pos = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs scales"):
        ops.attn_decode_append_rows(step, k8, v8, pos, H, Gk)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.attn_decode_append_rows(step, k8.float(), v8.float(), pos, H, Gk, scales=(ks, vs))
    with pytest.raises(ValueError, match="scales must be fp32"):
        ops.attn_decode_append_rows(step, k8, v8, pos, H, Gk, scales=(ks, vs[:, :, :-1]))
    with pytest.raises(ValueError, match="scales must be fp32"):
        ops.kv_cache_fill_varlen(step, torch.tensor([0, 1], dtype=torch.int32), k8, v8, scales=(ks.double(), vs))


# ------------------------------------------------------------------ models and generation
def _cfg(name):
    if name == "llama":
        return get_config("llama3_2", "1B").replace(context_length=CTX, emb_dim=64, n_heads=4, n_kv_groups=2,
                                                    hidden_dim=96, n_layers=2, vocab_size=VOCAB, dtype=torch.float32)
    return get_config("GPT2", "124M").replace(context_length=CTX, emb_dim=64, n_heads=4, n_kv_groups=4, hidden_dim=256,
                                              n_layers=2, vocab_size=VOCAB, dtype=torch.float32, drop_rate=0.0)


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        torch.manual_seed(0)
        m = build_model(_cfg(name))
        m.flatten()
        m.eval()
        _MODELS[name] = m
    return _MODELS[name]


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, VOCAB, (n,), generator=g) for n in (5, 24, 9)]


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_new_kv_cache_fp8(name):
    m = _model(name)
    cfg = m.cfg
    Gk = cfg.n_kv_groups if cfg.is_llama else cfg.n_heads
    plain = m.new_kv_cache(3, CTX)
    assert all(len(kv) == 2 and kv[0].dtype == torch.float32 for kv in plain)
    cache = m.new_kv_cache(3, CTX, kv_dtype="fp8")
    assert len(cache) == cfg.n_layers and cache[0][0].shape[2] == CTX
    for k8, v8, ks, vs in cache:
        assert k8.dtype == v8.dtype == F8 and k8.shape == v8.shape == (3, Gk, CTX, cfg.head_dim)
        assert ks.dtype == vs.dtype == torch.float32 and ks.shape == vs.shape == (3, Gk, CTX)
    assert not m.decode_graph_ok(cache)                    # CPU
    with pytest.raises(ValueError, match="kv_dtype"):
        m.new_kv_cache(3, CTX, kv_dtype="int8")


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_ragged_fp8(name):
    """It runs; row b alone is row b of a batch of 3; the default is bitwise what it was."""
    m = _model(name)
    prompts, new = _prompts(), 12
    batch = G.generate_ragged(m, prompts, new, CTX, kv_dtype="fp8")
    for p, r in zip(prompts, batch):
        assert r.numel() == p.numel() + new and torch.equal(r[:p.numel()], p)
        assert int(r.min()) >= 0 and int(r.max()) < VOCAB
        alone = G.generate_ragged(m, [p], new, CTX, kv_dtype="fp8")[0]
        assert torch.equal(alone, r)
    # seeded sampling goes through the same cache
    a = G.generate_ragged(m, prompts, new, CTX, temperature=0.8, top_k=20, seed=3, kv_dtype="fp8")
    b = G.generate_ragged(m, prompts, new, CTX, temperature=0.8, top_k=20, seed=3, kv_dtype="fp8")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    default = G.generate_ragged(m, prompts, new, CTX)
    explicit = G.generate_ragged(m, prompts, new, CTX, kv_dtype=None)
    assert all(torch.equal(x, y) for x, y in zip(default, explicit))
    with pytest.raises(ValueError, match="kv_dtype"):
        G.generate_ragged(m, prompts, new, CTX, kv_dtype="bf16")


@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_fp8_logits_follow_the_exact_cache(name):
    """Teacher-forced row steps on both caches: the prefill logits are bitwise equal (the prefill
    attends over the exact K / V), the later ones differ, by little."""
    m = _model(name)
    lens, steps = [1, 5, 24], 6
    g = torch.Generator().manual_seed(6)
    full = [torch.randint(0, VOCAB, (n + steps,), generator=g) for n in lens]
    idx, seq = pack_prompts([f[:n] for f, n in zip(full, lens)], "cpu")
    runs = {}
    with torch.no_grad():
        for kd in (None, "fp8"):
            cache = m.new_kv_cache(len(lens), CTX, kv_dtype=kd)
            got = [m.forward_prefill_ragged(idx, seq, cache)]
            pos = torch.tensor(lens, dtype=torch.int32)
            for s in range(steps):
                tok = torch.stack([f[n + s] for f, n in zip(full, lens)])[:, None]
                got.append(m.forward_cached_rows(tok, cache, pos))
                pos += 1
            runs[kd] = torch.stack(got)
    assert torch.equal(runs[None][0], runs["fp8"][0])
    rel = float((runs["fp8"][1:] - runs[None][1:]).norm() / runs[None][1:].norm())
    assert 0.0 < rel < 0.1, rel


def test_fixed_position_paths_refuse_an_fp8_cache():
    m = _model("llama")
    cache = m.new_kv_cache(1, CTX, kv_dtype="fp8")
    idx = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="generate_ragged"):
        m.forward_cached(idx, cache, 0)
    with pytest.raises(ValueError, match="generate_ragged"):
        m.forward_cached_dev(idx[:, :1], cache, torch.zeros(1, dtype=torch.int32))
    cfg = m.cfg
    qkv = torch.zeros(1, (cfg.n_heads + 2 * cfg.n_kv_groups) * cfg.head_dim)
    with pytest.raises(ValueError, match="generate_ragged"):
        cached_attention(qkv, 1, 1, 0, cfg.n_heads, cfg.n_kv_groups, cfg.head_dim, cache[0])
    import inspect
    assert "kv_dtype" not in inspect.signature(G.generate_cached).parameters


# ------------------------------------------------------------------ command line
@pytest.fixture
def roomy_debug(monkeypatch):
    """``--debug`` with a context of 256 tokens (tests/test_generate_ragged_cpu.py)."""
    dbg = builder.debug_config
    monkeypatch.setattr(builder, "debug_config", lambda cfg: dbg(cfg).replace(context_length=256))


def test_cli_flag_parsing(tmp_path):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(["Hi"]))
    base = ["--data_dir", str(tmp_path), "--generate_prompts", str(pf)]
    assert cli.get_args(base).generate_kv_dtype == "model"
    assert cli.get_args(base + ["--generate_kv_dtype", "fp8"]).generate_kv_dtype == "fp8"
    with pytest.raises(ValueError, match="--generate_kv_dtype"):
        cli.get_args(base + ["--generate_kv_dtype", "int4"])


def test_cli_generate_only_fp8(tmp_path, roomy_debug, monkeypatch):
    pf = tmp_path / "prompts.json"
    entries = ["Every effort moves you", {"instruction": "Name a colour.", "input": "", "output": "Blue."}, "Hi"]
    pf.write_text(json.dumps(entries))
    seen = []
    real = G.generate_ragged

    def spy(*a, **kw):
        seen.append(kw.get("kv_dtype"))
        return real(*a, **kw)

    from building_llm_from_scratch_amd.train import trainer as T
    monkeypatch.setattr(T, "generate_ragged", spy)
    argv = ["--model", "llama3_2", "--num_params", "1B", "--debug", "--device", "cpu", "--no_plot", "--batch_size", "2",
            "--output_dir", str(tmp_path / "out"), "--data_dir", str(tmp_path / "data"), "--num_workers", "0",
            "--generate_max_tokens", "5", "--generate_only", "--generate_prompts", str(pf),
            "--generate_kv_dtype", "fp8"]
    tr = cli.cli(argv)
    rows = json.load(open(tmp_path / "out" / "responses.json"))
    assert len(rows) == len(entries) and all(isinstance(r["response"], str) for r in rows)
    assert seen and all(k == "fp8" for k in seen)
    _, texts = cli.load_generate_prompts(pf)
    assert tr.generate_responses(texts, 5, 2, kv_dtype="fp8") == [r["response"] for r in rows]
    n = len(seen)
    tr.generate_responses(texts, 5, 2)
    assert all(k is None for k in seen[n:])
