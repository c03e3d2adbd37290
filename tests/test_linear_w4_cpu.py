"""MXFP4 decode weights without a GPU: the block format (``ops.reference.mx4_quantize_rows`` on
hand-written blocks, its error bound), the pack layout (``ops.w4_pack`` / ``w4_unpack``), the fp64
oracle ``ops.reference.linear_w4``, generation on the packs against a twin model that holds the
dequantised weights, and the entry points (``weight_dtype`` / ``--generate_weight_dtype``)."""
import json

import pytest
import torch

from building_llm_from_scratch_amd import builder, cli, ops
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.models import build_model
from building_llm_from_scratch_amd.models.base import DecodeWeights, pack_prompts
from building_llm_from_scratch_amd.models.linear import LinearW4, LinearW8
from building_llm_from_scratch_amd.models.lora import replace_linear_with_lora
from building_llm_from_scratch_amd.ops import reference as ref
from building_llm_from_scratch_amd.train import generate as G

F32 = torch.float32
TN, KG, BLK = ops.W4_ROW_TILE, ops.W4_K_GRANULE, ops.W4_BLOCK
CTX = 64


# ------------------------------------------------------------------ the block format
def _block(head, fill=0.0):
    """One 32-wide block: ``head`` then ``fill``."""
    x = torch.full((1, BLK), float(fill), dtype=F32)
    x[0, :len(head)] = torch.tensor(head, dtype=F32)
    return x


def _codes(x):
    """-> (the 32 codes of a one-block row, its scale byte)"""
    c, s = ref.mx4_quantize_rows(x)
    assert c.dtype == torch.uint8 and s.dtype == torch.uint8 and c.shape == (1, BLK // 2) and s.shape == (1, 1)
    return torch.stack([c[0] & 15, c[0] >> 4], -1).reshape(-1).tolist(), int(s[0, 0])


def test_constants():
    assert (KG, BLK, TN) == (128, 32, 16) and ref.MX4_VALUES == (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def test_block_all_zero():
    assert _codes(_block([])) == ([0] * BLK, 127)
    assert _codes(_block([-0.0, 0.0])) == ([0] * BLK, 127)


def test_block_maximum_exactly_six_times_the_scale():
    """a = 6 * 2^-3: e = -3, the maximum is code 7 and is not clipped; 2^-3 itself is code 2."""
    codes, byte = _codes(_block([0.75, -0.75, 0.125]))
    assert byte == 127 - 3 and codes == [7, 15, 2] + [0] * (BLK - 3)
    for e in (-20, 0, 9):
        codes, byte = _codes(_block([6.0 * 2.0 ** e]))
        assert byte == 127 + e and codes[0] == 7


def test_block_maximum_one_ulp_above():
    """The next fp32 after 6 * 2^-3 needs e = -2, where it is 3 (1 + 2^-23): code 5."""
    up32 = float(torch.nextafter(torch.tensor(0.75), torch.tensor(1.0)))
    assert up32 > 0.75
    codes, byte = _codes(_block([up32, -0.5]))
    assert byte == 127 - 2 and codes == [5, 8 | 4] + [0] * (BLK - 2)


def test_block_ties_go_to_the_even_code():
    """With a maximum of 6 the scale is 1: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2,
    3.5 -> 4, 5 -> 4, both signs; a value that rounds to zero has code 0 whatever its sign."""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]
    codes, byte = _codes(_block([6.0] + ties + [-t for t in ties]))
    assert byte == 127
    assert codes == [7] + want + [0] + [8 | c for c in want[1:]] + [0] * (BLK - 15)
    d = ref.mx4_dequantize(*ref.mx4_quantize_rows(_block([6.0] + ties + [-t for t in ties])))
    vals = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert d[0, :15].tolist() == [6.0] + vals + [-v for v in vals]
    # just off a tie goes to the nearer neighbour
    lo, hi = (float(torch.nextafter(torch.tensor(2.5), torch.tensor(s))) for s in (0.0, 9.0))
    assert _codes(_block([6.0, lo, hi]))[0][:3] == [7, 4, 5]
    # the same at another scale
    codes, byte = _codes(_block([6.0 * 2 ** -5] + [t * 2 ** -5 for t in ties]))
    assert byte == 127 - 5 and codes[:8] == [7] + want


def test_block_with_an_outlier():
    """One element 100 times the others: 100 = 0.78 * 2^7 gives e = 5, the outlier is 3.125 -> 3
    (96) and the ones, 1 / 32 of the scale, are below the first midpoint: they become zero."""
    codes, byte = _codes(_block([1.0, -1.0, 100.0], fill=1.0))
    assert byte == 127 + 5 and codes == [0, 0, 5] + [0] * (BLK - 3)
    assert ref.mx4_dequantize(*ref.mx4_quantize_rows(_block([1.0, -1.0, 100.0], fill=1.0)))[0, 2] == 96.0


def test_block_of_tiny_values_and_the_clamp():
    """1e-30 = 0.63 * 2^-99: e = -102 by the rule (byte 25), 1e-30 / 2^-102 = 5.07 -> 6.  The
    clamp at -126 is reached from 6 * 2^-126 down: 3 * 2^-126 would have e = -127 and keeps -126
    (code 5), and a subnormal block has byte 1 and zero codes.  Byte 255 is never written, nor 0."""
    assert _codes(_block([], fill=1e-30)) == ([7] * BLK, 25)
    assert _codes(_block([3 * 2.0 ** -126, -(2.0 ** -126)])) == ([5, 8 | 2] + [0] * (BLK - 2), 1)
    assert _codes(_block([], fill=1e-40)) == ([0] * BLK, 1)
    big = torch.finfo(F32).max
    codes, byte = _codes(_block([big, -big]))
    assert byte == 127 + 126 and codes[:2] == [6, 14]          # 2^128 (1 - 2^-24) / 2^126 = 4 (1 - 2^-24) -> 4


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_weights_raise(bad):
    x = torch.randn(3, 2 * KG)
    x[1, 70] = bad
    with pytest.raises(ValueError, match="non-finite"):
        ref.mx4_quantize_rows(x)
    with pytest.raises(ValueError, match="non-finite"):
        ops.w4_pack(x)
    with pytest.raises(ValueError, match="non-finite"):
        ops.w4_pack(x.to(torch.bfloat16))


def test_storage_order():
    """Element 2 i in the low nibble of byte i."""
    x = _block([6.0, -1.0, 0.5, 3.0])
    c, _ = ref.mx4_quantize_rows(x)
    assert c[0, :2].tolist() == [7 | (10 << 4), 1 | (5 << 4)]
    assert ref.mx4_dequantize(*ref.mx4_quantize_rows(x))[0, :4].tolist() == [6.0, -1.0, 0.5, 3.0]


def _random_rows():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(40, 3 * KG, generator=g) * torch.logspace(-2, 1, 40)[:, None]
    x[3, 32:64] = 0                                  # a zero block inside a row
    x[5] *= torch.logspace(-3, 3, 3 * KG)            # blocks of very different size in one row
    return x


def test_error_bound():
    """|x - dequantised| <= max(|x| / 4, 2^e / 4) per element, and the maximum of a block moves by
    no more than a fifth (5 -> 4 is the worst case: it is never clipped to 6 from above)."""
    x = _random_rows()
    c, s = ref.mx4_quantize_rows(x)
    d = ref.mx4_dequantize(c, s)
    assert d.dtype == F32 and d.shape == x.shape
    two_e = (2.0 ** (s.double() - 127)).repeat_interleave(BLK, -1)
    err = (x.double() - d.double()).abs()
    assert bool((err <= torch.maximum(x.abs().double() / 4, two_e / 4)).all())
    xb, db = x.view(40, -1, BLK).abs().amax(-1), d.view(40, -1, BLK).abs().amax(-1)
    assert bool(((xb.double() - db.double()).abs() <= xb.double() / 5).all())
    assert bool((xb <= 6 * 2.0 ** (s.double() - 127)).all()) and bool((xb[xb > 0] > 3 * 2.0 ** (s.double() - 127)[xb > 0]).all())
    assert not (s == 255).any() and not (s == 0).any()
    # bf16 holds every dequantised value, and bf16 / fp16 inputs are read as their fp32 values
    assert torch.equal(ref.mx4_dequantize(c, s, torch.bfloat16).float(), d)
    cb, sb = ref.mx4_quantize_rows(x.to(torch.bfloat16))
    c0, s0 = ref.mx4_quantize_rows(x.to(torch.bfloat16).float())
    assert torch.equal(cb, c0) and torch.equal(sb, s0)


def test_requantising_is_idempotent():
    """The dequantised rows quantise to themselves.  (The bytes may differ: a block whose maximum
    became 3 * 2^e is stored as 6 * 2^(e-1).)"""
    d = ref.mx4_dequantize(*ref.mx4_quantize_rows(_random_rows()))
    d2 = ref.mx4_dequantize(*ref.mx4_quantize_rows(d))
    assert torch.equal(d2, d)
    c2, s2 = ref.mx4_quantize_rows(d2)
    c3, s3 = ref.mx4_quantize_rows(ref.mx4_dequantize(c2, s2))
    assert torch.equal(c3, c2) and torch.equal(s3, s2)


def test_shapes_the_quantiser_refuses():
    for shape in ((4, 48), (4, 16), (0,)):
        with pytest.raises(ValueError, match="mx4_quantize_rows"):
            ref.mx4_quantize_rows(torch.zeros(shape))
    c, s = ref.mx4_quantize_rows(torch.randn(2, 3, 64))
    assert c.shape == (2, 3, 32) and s.shape == (2, 3, 2)


# ------------------------------------------------------------------ pack layout
def _weight(N, K):
    g = torch.Generator().manual_seed(N * 1000 + K)
    return torch.randn(N, K, generator=g) * torch.logspace(-1, 1, N)[:, None]


@pytest.mark.parametrize("K", [KG, 3 * KG])
@pytest.mark.parametrize("N", [1, TN - 1, TN, TN + 1, 53])
def test_pack_contract(N, K):
    W = _weight(N, K)
    pack = ops.w4_pack(W)
    T, nkb = -(-N // TN), K // KG
    assert isinstance(pack, ops.W4Pack) and pack.tiled and (pack.N, pack.K) == (N, K)
    assert pack.data.dtype == torch.uint8 and pack.data.shape == (T * TN * K // 2,)
    assert pack.scale.dtype == torch.uint8 and pack.scale.shape == (T * TN * K // BLK,)
    c, s = ops.w4_unpack(pack)
    c0, s0 = ref.mx4_quantize_rows(W)
    assert c.dtype == torch.uint8 and s.dtype == torch.uint8 and torch.equal(c, c0) and torch.equal(s, s0)
    # the layout the kernel reads: tile t, block kb, lane 16 g + r: 16 code bytes and one scale byte
    data, scale = pack.data.view(T, nkb, 4, TN, 16), pack.scale.view(T, nkb, 4, TN)
    for n in {0, N // 2, N - 1}:
        for kb in {0, nkb - 1}:
            for gq in range(4):
                assert torch.equal(data[n // TN, kb, gq, n % TN], c0[n, 64 * kb + 16 * gq:64 * kb + 16 * gq + 16])
                assert int(scale[n // TN, kb, gq, n % TN]) == int(s0[n, 4 * kb + gq])
    # padding rows: zero codes, scale byte 127
    pad = (N - 1) % TN + 1
    assert not data[-1, :, :, pad:].any() and bool((scale[-1, :, :, pad:] == 127).all())
    # packing is a bijection of the bytes
    again = ops.W4Pack(pack.data.clone(), pack.scale.clone(), N, K, True)
    assert all(torch.equal(a, b) for a, b in zip(ops.w4_unpack(again), (c0, s0)))


def test_pack_of_other_widths_runs_the_oracle():
    """K = 192 is whole MX blocks but no multiple of the kernel's granule: the pack keeps the bytes
    row-major and ``linear_w4`` composes the oracle.  A K that is not whole blocks has no pack."""
    W, x = torch.randn(7, 192), torch.randn(3, 192)
    pack = ops.w4_pack(W)
    assert not pack.tiled and pack.data.shape == (7 * 96,) and pack.scale.shape == (7 * 6,)
    c, s = ops.w4_unpack(pack)
    c0, s0 = ref.mx4_quantize_rows(W)
    assert torch.equal(c, c0) and torch.equal(s, s0)
    y = ops.linear_w4(x, pack)
    assert torch.equal(y, ref.linear_w4(x, c, s)) and y.dtype == F32
    assert torch.equal(y, (x.double() @ ref.mx4_dequantize(c, s).double().t()).float())
    with pytest.raises(ValueError, match="linear_w4"):
        ops.linear_w4(torch.randn(3, 160), pack)
    for shape in ((7, 10), (7, 200), (192,)):
        with pytest.raises(ValueError, match="w4_pack"):
            ops.w4_pack(torch.randn(shape))


def test_oracle_is_the_fp64_product():
    g = torch.Generator().manual_seed(1)
    W, x = torch.randn(37, 2 * KG, generator=g), torch.randn(5, 2 * KG, generator=g).double()
    bias, res = torch.randn(37, generator=g).double(), torch.randn(5, 37, generator=g).double()
    c, s = ref.mx4_quantize_rows(W)
    base = x @ ref.mx4_dequantize(c, s).double().t()
    for b, r in ((None, None), (bias, None), (None, res), (bias, res)):
        want = base + (0 if b is None else b) + (0 if r is None else r)
        got = ref.linear_w4(x, c, s, b, r)
        assert got.dtype == torch.float64
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert ref.linear_w4(x.to(torch.bfloat16), c, s).dtype == torch.bfloat16
    assert torch.equal(ops.linear_w4(x.float(), ops.w4_pack(W), bias.float()), ref.linear_w4(x.float(), c, s, bias.float()))
    # fp16 x: the weight is rounded to fp16 first, which changes nothing inside 2^-13 <= 2^e <= 2^13
    assert int(s.min()) >= 127 - 13 and int(s.max()) <= 127 + 13
    xh = x.to(torch.float16)
    assert torch.equal(ref.linear_w4(xh, c, s), (xh.double() @ ref.mx4_dequantize(c, s).double().t()).to(torch.float16))


# ------------------------------------------------------------------ models
def _cfgs():
    """The tiny models of tests/test_linear_w8_cpu.py, and a Llama whose down projection reads
    K = 320: whole fp8 granules, no whole MXFP4 granule."""
    llama = get_config("llama3_2", "1B").replace(context_length=CTX, emb_dim=256, n_heads=4, n_kv_groups=2,
                                                 hidden_dim=384, n_layers=2, vocab_size=512, dtype=F32)
    gpt = get_config("GPT2", "124M").replace(context_length=CTX, emb_dim=256, n_heads=4, n_kv_groups=4, hidden_dim=1024,
                                             n_layers=2, vocab_size=512, drop_rate=0.0, dtype=F32)
    return {"llama": llama, "gpt2": gpt, "llama320": llama.replace(hidden_dim=320)}


def _build(name, lora, seed=0):
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
    return m


_MODELS = {}


def _model(name, lora=False):
    if (name, lora) not in _MODELS:
        _MODELS[name, lora] = _build(name, lora)
    return _MODELS[name, lora]


def _groups(m):
    return [fl for c in m.computes[1:-1] for fl in c.w8_groups()] + [m.computes[-1].head]


def _packs(w):
    return [p for blk in w.blocks for p in blk] + [w.head]


def _dequantised(pk):
    if isinstance(pk, LinearW4):
        return ref.mx4_dequantize(*ops.w4_unpack(pk.pack))
    assert isinstance(pk, LinearW8)
    return ref.kv_dequantize(*ops.w8_unpack(pk.pack))


def _dequantised_twin(name, lora, m, w):
    """A copy of the model whose projection weights are the dequantised packs (LoRA, folded into
    the packs, switched off by a zero B)."""
    twin = _build(name, lora, seed=1)
    twin.load_state_dict(m.state_dict())
    with torch.no_grad():
        for fl, pk in zip(_groups(twin), _packs(w)):
            fl.W().copy_(_dequantised(pk))
            for s in fl.specs:
                if s.lora_A is not None:
                    fl.unit.data(s.lora_B).zero_()
    return twin


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (n,), generator=g) for n in (5, 24, 9)]


def _greedy_loop(m, twin, prompts, new):
    """What ``generate_ragged(weight_dtype=...)`` documents: the prefill and the first token on the
    exact weights, every later step on the (here: dequantised) packed ones."""
    lens = [int(p.numel()) for p in prompts]
    idx, seq = pack_prompts(prompts, "cpu")
    with torch.no_grad():
        cache = m.new_kv_cache(len(prompts), CTX)
        logits = m.forward_prefill_ragged(idx, seq, cache)
        pos = torch.tensor(lens, dtype=torch.int32)
        toks = []
        for s in range(new):
            tok = logits.argmax(-1)
            toks.append(tok)
            if s + 1 < new:
                logits = twin.forward_cached_rows(tok[:, None], cache, pos)
                pos += 1
    out = torch.stack(toks, 1)
    return [torch.cat([p, o]) for p, o in zip(prompts, out)]


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_generate_on_the_packs_is_the_dequantised_model(name, lora):
    m = _model(name, lora)
    w = m.new_decode_weights("mxfp4")
    assert isinstance(w, DecodeWeights) and len(w.blocks) == 2 and all(len(b) == 4 for b in w.blocks)
    assert all(isinstance(p, LinearW4) and p.pack.tiled for blk in w.blocks for p in blk)
    assert isinstance(w.head, LinearW8) and w.head.pack.N == 512
    assert [p.bias is not None for p in _packs(w)] == [fl.b() is not None for fl in _groups(m)]
    if lora:     # LoRA is folded in fp32 before quantising
        fl, pk = _groups(m)[0], _packs(w)[0]
        W_eff = fl.W().float().clone()
        for (c0, c1), s in zip(fl.cols, fl.specs):
            W_eff[c0:c1] += s.scaling * (fl.unit.data(s.lora_A).float() @ fl.unit.data(s.lora_B).float()).t()
        assert not torch.equal(W_eff, fl.W().float())
        assert all(torch.equal(a, b) for a, b in zip(ops.w4_unpack(pk.pack), ref.mx4_quantize_rows(W_eff)))
    twin = _dequantised_twin(name, lora, m, w)
    prompts, new = _prompts(), 6
    want = _greedy_loop(m, twin, prompts, new)
    got = G.generate_ragged(m, prompts, new, CTX, weight_dtype="mxfp4")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(G.generate_ragged(m, prompts, new, CTX, weight_dtype=w), want))
    # it is a different model from the exact one and from the fp8 one, after the shared first token
    exact = _greedy_loop(m, m, prompts, new)
    assert all(int(a[p.numel()]) == int(b[p.numel()]) for p, a, b in zip(prompts, got, exact))
    w8 = m.new_decode_weights("fp8")
    assert all(isinstance(p, LinearW8) for p in _packs(w8))
    tok = torch.zeros(3, 1, dtype=torch.long)
    pos = torch.tensor([5, 24, 9], dtype=torch.int32)
    with torch.no_grad():
        cache = m.new_kv_cache(3, CTX)
        m.forward_prefill_ragged(*pack_prompts(prompts, "cpu"), cache)
        steps = [m.forward_cached_rows(tok, [tuple(t.clone() for t in kv) for kv in cache], pos, weights=x)
                 for x in (None, w8, w)]
    assert not torch.equal(steps[2], steps[0]) and not torch.equal(steps[2], steps[1])


def test_groups_the_kernel_cannot_take_keep_their_fp8_pack():
    """K = 320 is no multiple of 128: that group (the down projection) and the head are LinearW8,
    the others LinearW4, and the mixed weights generate what the dequantised twin does."""
    m = _model("llama320")
    w = m.new_decode_weights("mxfp4")
    for blk in w.blocks:
        assert [type(p) for p in blk] == [LinearW4, LinearW4, LinearW4, LinearW8]
        assert blk[3].pack.K == 320 and blk[3].pack.tiled
    assert isinstance(w.head, LinearW8)
    twin = _dequantised_twin("llama320", False, m, w)
    prompts, new = _prompts(), 5
    got = G.generate_ragged(m, prompts, new, CTX, weight_dtype="mxfp4")
    assert all(torch.equal(a, b) for a, b in zip(got, _greedy_loop(m, twin, prompts, new)))


# ------------------------------------------------------------------ entry points
def test_generate_ragged_weight_dtype(monkeypatch):
    m = _model("llama")
    prompts, new = _prompts(), 4
    with pytest.raises(ValueError, match="weight_dtype.*'fp8', 'mxfp4'"):
        G.generate_ragged(m, prompts, new, CTX, weight_dtype="int4")
    with pytest.raises(ValueError, match="weight_dtype.*'fp8' or 'mxfp4'"):
        m.new_decode_weights("bf16")
    with pytest.raises(ValueError, match="weight_dtype"):
        G.generate_ragged(m, prompts, new, CTX, speculative=2, weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="weight_dtype"):
        G.generate_ragged(m, prompts, new, CTX, speculative=2, weight_dtype=m.new_decode_weights("mxfp4"))
    built = []
    real = m.new_decode_weights
    monkeypatch.setattr(m, "new_decode_weights", lambda *a, **k: built.append(a) or real(*a, **k))
    batch = G.generate_ragged(m, prompts, new, CTX, weight_dtype="mxfp4", kv_dtype="fp8")
    assert built == [("mxfp4",)]
    for p, r in zip(prompts, batch):
        assert r.numel() == p.numel() + new and torch.equal(r[:p.numel()], p)
    a = G.generate_ragged(m, prompts, new, CTX, weight_dtype=real("mxfp4"), temperature=0.8, top_k=20, seed=3)
    b = G.generate_ragged(m, prompts, new, CTX, weight_dtype="mxfp4", temperature=0.8, top_k=20, seed=3)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and len(built) == 2


def test_cli_flag_parsing(tmp_path):
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(["Hi"]))
    base = ["--data_dir", str(tmp_path), "--generate_prompts", str(pf)]
    a = cli.get_args(base + ["--generate_weight_dtype", "mxfp4", "--generate_kv_dtype", "fp8"])
    assert a.generate_weight_dtype == "mxfp4" and a.generate_kv_dtype == "fp8"
    with pytest.raises(ValueError, match="--generate_weight_dtype must be 'model', 'fp8' or 'mxfp4'"):
        cli.get_args(base + ["--generate_weight_dtype", "int4"])
    with pytest.raises(ValueError, match="--generate_speculative runs on"):
        cli.get_args(base + ["--generate_speculative", "2", "--generate_weight_dtype", "mxfp4"])


@pytest.fixture
def roomy_debug(monkeypatch):
    """``--debug`` with a context of 256 tokens (tests/test_generate_ragged_cpu.py)."""
    dbg = builder.debug_config
    monkeypatch.setattr(builder, "debug_config", lambda cfg: dbg(cfg).replace(context_length=256))


def test_cli_round_trip_and_one_pack_for_all_batches(tmp_path, roomy_debug, monkeypatch):
    """``--generate_weight_dtype mxfp4`` end to end on the CPU.  ``--debug`` has K = 10, so every
    group keeps its fp8 pack and the answers are those of ``weight_dtype="fp8"``; three batches of
    ``generate_responses`` share one set of packs."""
    pf = tmp_path / "prompts.json"
    entries = ["Every effort moves you", {"instruction": "Name a colour.", "input": "", "output": "Blue."}, "Hi"]
    pf.write_text(json.dumps(entries))
    argv = ["--model", "llama3_2", "--num_params", "1B", "--debug", "--device", "cpu", "--no_plot", "--batch_size", "1",
            "--output_dir", str(tmp_path / "out"), "--data_dir", str(tmp_path / "data"), "--num_workers", "0",
            "--generate_max_tokens", "5", "--generate_only", "--generate_prompts", str(pf),
            "--generate_weight_dtype", "mxfp4"]
    tr = cli.cli(argv)
    rows = json.load(open(tmp_path / "out" / "responses.json"))
    assert len(rows) == len(entries) and all(isinstance(r["response"], str) for r in rows)
    _, texts = cli.load_generate_prompts(pf)
    built, seen = [], []
    real_new, real_gen = tr.model.new_decode_weights, G.generate_ragged
    monkeypatch.setattr(tr.model, "new_decode_weights", lambda *a, **k: built.append(a) or real_new(*a, **k))

    def spy(*a, **kw):
        seen.append(kw.get("weight_dtype"))
        return real_gen(*a, **kw)

    from building_llm_from_scratch_amd.train import trainer as T
    monkeypatch.setattr(T, "generate_ragged", spy)
    assert tr.generate_responses(texts, 5, 1, weight_dtype="mxfp4") == [r["response"] for r in rows]
    assert built == [("mxfp4",)] and len(seen) == 3
    assert all(isinstance(s, DecodeWeights) and s is seen[0] for s in seen)
    assert all(isinstance(p, LinearW8) and not p.pack.tiled for p in _packs(seen[0]))
    assert tr.generate_responses(texts, 5, 1, weight_dtype="fp8") == [r["response"] for r in rows]
    with pytest.raises(ValueError, match="weight_dtype must be None, 'fp8' or 'mxfp4'"):
        tr.generate_responses(texts, 5, 1, weight_dtype="int4")
