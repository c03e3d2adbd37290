"""Unpadded instruction finetuning on the GPU: the variable-length attention kernels and the
RoPE-by-position kernel against their fp32 oracles, isolation between the sequences of a packed
batch, and the packed model (``seq_lens``) against the padded CPU fp32 model."""
import pytest
import torch
from numerics import check_close, check_elem

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.data.datasets import custom_collate_fn, unpad_lengths
from building_llm_from_scratch_amd.models import build_model, replace_linear_with_lora
from building_llm_from_scratch_amd.models.head import MIN_CHUNK_ROWS
from building_llm_from_scratch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LSE_TOL = dict(rtol=1e-5, atol=2e-5)   # tests/test_kernels_gpu.py: fp32 log-sum-exp
# single row, sub-tile, exact tile multiples (64-key / 128-query tiles), one past a tile, empty, tail
LENS = [1, 31, 64, 129, 0, 200, 128]
CTX = 256


@pytest.fixture(autouse=True)
def _ext():
    assert ops.load_ext(required=True)
    torch.manual_seed(0)


def _cu(lens):
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32)
    return cu, pos


def _tables(hd):
    return ops.rope_tables(hd, CTX, 500000.0, device=DEV)


def _inputs(lens, H, G, hd, dt, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = sum(lens)
    qkv = torch.randn(N, (H + 2 * G) * hd, device=DEV, generator=g).to(dt)
    do = torch.randn(N, H * hd, device=DEV, generator=g).to(dt)
    return qkv, do


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,G", [(4, 4), (8, 2), (4, 1)])
def test_varlen_attention_vs_oracle(dt, hd, H, G):
    """Forward, lse and dqkv (with and without the fused inverse RoPE, whose positions restart at
    every sequence) against the fp32 oracle; the grid sized by the exact maximum and by a larger
    max_len (whole workgroups beyond every sequence)."""
    cu, pos = _cu(LENS)
    qkv, do = _inputs(LENS, H, G, hd, dt)
    cos, sin = _tables(hd)
    o0, lse0 = ref.flash_attn_varlen_fwd(qkv.cpu().float(), cu, 200, H, G, hd)
    d0 = {r: ref.flash_attn_varlen_bwd(qkv.cpu().float(), o0, lse0, do.cpu().float(), cu, pos, 200, H, G, hd,
                                       (cos.cpu(), sin.cpu()) if r else None) for r in (False, True)}
    cud, posd = cu.to(DEV), pos.to(DEV)
    for max_len in (200, 256):
        o, lse = ops.flash_attn_varlen_fwd(qkv, cud, max_len, H, G, hd)
        check_close(o, o0, dt, k=3.0, name=f"o max_len {max_len}")
        check_elem(lse, lse0, **LSE_TOL, name=f"lse max_len {max_len}")
        for r in (False, True):
            dqkv = ops.flash_attn_varlen_bwd(qkv, o, lse, do, cud, posd, max_len, H, G, hd,
                                             rope=(cos, sin) if r else None)
            check_close(dqkv, d0[r], dt, k=5.0, name=f"dqkv max_len {max_len} rope {r}")


@pytest.mark.parametrize("hd", [128, 64])
def test_varlen_attention_fused_gqa_heads(hd):
    """128 sequences of 128 rows at 16 / 8 heads: the shape at which the dK/dV kernel sums the
    query heads of a kv head in one workgroup instead of writing fp32 partials."""
    H, G, dt = 16, 8, torch.bfloat16
    lens = [128] * 128
    cu, pos = _cu(lens)
    qkv, do = _inputs(lens, H, G, hd, dt)
    cos, sin = _tables(hd)
    cud, posd = cu.to(DEV), pos.to(DEV)
    o, lse = ops.flash_attn_varlen_fwd(qkv, cud, 128, H, G, hd)
    dqkv = ops.flash_attn_varlen_bwd(qkv, o, lse, do, cud, posd, 128, H, G, hd, rope=(cos, sin))
    # fp32 oracle on the GPU (same torch ops as on the CPU)
    o0, lse0 = ref.flash_attn_varlen_fwd(qkv.float(), cu, 128, H, G, hd)
    d0 = ref.flash_attn_varlen_bwd(qkv.float(), o0, lse0, do.float(), cu, posd, 128, H, G, hd, (cos, sin))
    check_close(o, o0, dt, k=3.0, name="o")
    check_elem(lse, lse0, **LSE_TOL, name="lse")
    check_close(dqkv, d0, dt, k=5.0, name="dqkv")
    # equal lengths: lse / delta are laid out as the uniform kernels' [B, H, T]
    o1, lse1 = ops.flash_attn_fwd(qkv, 128, 128, H, G, hd, True)
    check_elem(lse, lse1.reshape(-1), **LSE_TOL, name="lse vs uniform")
    d1 = ops.flash_attn_bwd(qkv, o1, lse1, do, 128, 128, H, G, hd, True, rope=(cos, sin))
    print("bitwise equal to the uniform kernels:", torch.equal(o, o1), torch.equal(lse, lse1.reshape(-1)),
          torch.equal(dqkv, d1))


@pytest.mark.parametrize("hd,H,G", [(64, 8, 2), (128, 4, 4)])
def test_varlen_attention_isolation_and_determinism(hd, H, G):
    """Replacing the rows of one sequence changes no output row of any other (bitwise), and two
    identical runs agree bitwise everywhere."""
    dt = torch.bfloat16
    cu, pos = _cu(LENS)
    cud, posd = cu.to(DEV), pos.to(DEV)
    cos, sin = _tables(hd)

    def run(qkv, do):
        o, lse = ops.flash_attn_varlen_fwd(qkv, cud, 200, H, G, hd)
        return o, lse, ops.flash_attn_varlen_bwd(qkv, o, lse, do, cud, posd, 200, H, G, hd, rope=(cos, sin))

    qkv, do = _inputs(LENS, H, G, hd, dt)
    a, b = run(qkv, do), run(qkv.clone(), do.clone())
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    r0, r1 = int(cu[3]), int(cu[4])
    qkv2, do2 = qkv.clone(), do.clone()
    other, _ = _inputs(LENS, H, G, hd, dt, seed=1)
    qkv2[r0:r1] = other[r0:r1]
    do2[r0:r1] = -do[r0:r1]
    c = run(qkv2, do2)
    keep = torch.ones(sum(LENS), dtype=torch.bool, device=DEV)
    keep[r0:r1] = False
    assert torch.equal(a[0][keep], c[0][keep]) and torch.equal(a[2][keep], c[2][keep])
    assert not torch.equal(a[0][~keep], c[0][~keep])
    lkeep = torch.ones(H * sum(LENS), dtype=torch.bool, device=DEV)
    lkeep[H * r0:H * r1] = False
    assert torch.equal(a[1][lkeep], c[1][lkeep])


@pytest.mark.parametrize("dt,hd", [(torch.float32, 64), (torch.bfloat16, 32)])
def test_varlen_attention_other_dtypes_and_head_dims(dt, hd):
    """fp32 (the CLI default) and head dims without MFMA kernels: one uniform-kernel call per sequence."""
    H, G = 4, 2
    lens = [5, 0, 70, 33]
    cu, pos = _cu(lens)
    qkv, do = _inputs(lens, H, G, hd, dt)
    cos, sin = _tables(hd)
    o0, lse0 = ref.flash_attn_varlen_fwd(qkv.cpu().float(), cu, 70, H, G, hd)
    d0 = ref.flash_attn_varlen_bwd(qkv.cpu().float(), o0, lse0, do.cpu().float(), cu, pos, 70, H, G, hd,
                                   (cos.cpu(), sin.cpu()))
    o, lse = ops.flash_attn_varlen_fwd(qkv, cu.to(DEV), 70, H, G, hd, bounds=cu.tolist())
    dqkv = ops.flash_attn_varlen_bwd(qkv, o, lse, do, cu.to(DEV), pos.to(DEV), 70, H, G, hd, rope=(cos, sin))
    check_close(o, o0, dt, k=3.0, name="o")
    check_elem(lse, lse0, **LSE_TOL, name="lse")
    check_close(dqkv, d0, dt, k=5.0, name="dqkv")


def test_varlen_binding_refuses_bad_arguments():
    qkv = torch.zeros(8, 3 * 64, device=DEV, dtype=torch.bfloat16)
    cu = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        torch.ops.bllm.flash_attn_varlen_fwd(qkv.float(), cu, 8, 1, 1, 64)       # dtype
    with pytest.raises(RuntimeError):
        torch.ops.bllm.flash_attn_varlen_fwd(qkv, cu.long(), 8, 1, 1, 64)        # cu dtype
    with pytest.raises(RuntimeError):
        torch.ops.bllm.flash_attn_varlen_fwd(qkv.view(8, 6, 32), cu, 8, 2, 2, 32)  # head dim / shape


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("hd,H,G", [(64, 4, 4), (128, 8, 2), (2, 16, 8)])
def test_rope_pos(dt, hd, H, G):
    """Forward against the oracle and the inverse round trip, in the bands of test_rope."""
    lens = [17, 1, 0, 30]
    _, pos = _cu(lens)
    cos, sin = ops.rope_tables(hd, 32, 500000.0, {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                                  "original_context_length": 8192}, device=DEV)
    qkv = torch.randn(sum(lens), (H + 2 * G) * hd, device=DEV).to(dt)
    q0 = ref.rope_pos_(qkv.cpu().float().clone(), cos.cpu(), sin.cpu(), pos, H, G, hd)
    q1 = ops.rope_pos_(qkv.clone(), cos, sin, pos.to(DEV), H, G, hd)
    check_close(q1, q0, dt, k=2.0, name="rope_pos")
    back = ops.rope_pos_(q1.clone(), cos, sin, pos.to(DEV), H, G, hd, inverse=True)
    check_close(back, qkv.float(), dt, k=3.0, name="rope_pos inverse")
    # positions restart at every sequence: rows 17 and 18 sit at position 0 (cos 1, sin 0)
    assert torch.equal(q1[17:19], qkv[17:19]) and not torch.equal(q1[16], qkv[16])


# ------------------------------------------------------------------ model
def _cfgs():
    # tests/test_model_gpu.py::_cfgs
    llama = get_config("llama3_1", "8B").replace(context_length=256, emb_dim=512, n_heads=8, n_kv_groups=2,
                                                 hidden_dim=768, n_layers=2, vocab_size=1000)
    llama128 = get_config("llama3", "8B").replace(context_length=256, emb_dim=512, n_heads=4, n_kv_groups=1,
                                                  hidden_dim=512, n_layers=2, vocab_size=1000)
    return {"llama_hd64": llama, "llama_hd128": llama128}


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ragged_batch():
    g = torch.Generator().manual_seed(11)
    recs = [(3, torch.randint(0, 999, (n,), generator=g).tolist()) for n in (40, 255, 7, 130)]
    x, y = custom_collate_fn(recs, pad_token_id=999)
    lens = unpad_lengths(y)
    assert x.shape == (4, 255) and lens.tolist() == [40, 255, 7, 130]
    return x, y, lens


def _check_model(ref_m, gpu_m, dt):
    x, y, lens = _ragged_batch()
    lr = ref_m(x, y)                              # padded, CPU fp32
    lr.backward()
    lg = gpu_m(x, y, seq_lens=lens)               # packed: 432 real rows in 512
    lg.backward()
    assert gpu_m.rctx.seq.N == 2 * MIN_CHUNK_ROWS and gpu_m.rctx.seq.max_len == 255
    tol = 2e-2 if dt == torch.bfloat16 else 1e-4
    gtol = 5e-2 if dt == torch.bfloat16 else 1e-3
    assert abs(lg.item() - lr.item()) < tol * abs(lr.item()), (lg.item(), lr.item())
    named = dict(ref_m.named_parameters())
    n = 0
    for k, p in gpu_m.named_parameters():
        if not p.requires_grad:
            continue
        e = _rel(p.grad, named[k].grad)
        assert e < gtol, (k, e)
        n += 1
    assert n


@pytest.mark.parametrize("name", ["llama_hd64", "llama_hd128"])
@pytest.mark.parametrize("ckpt", ["none", "selective", "full"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_unpadded_gpu_model_matches_padded_cpu_reference(name, ckpt, dt):
    cfg = _cfgs()[name]
    torch.manual_seed(0)
    ref_m = build_model(cfg.replace(dtype=torch.float32), use_actv_ckpt=ckpt)
    gpu_m = build_model(cfg.replace(dtype=dt), use_actv_ckpt=ckpt, device="cuda")
    gpu_m.load_state_dict(ref_m.state_dict())
    _check_model(ref_m, gpu_m, dt)


def test_unpadded_gpu_lora_model_kaug_path():
    """Frozen bf16 base with rank-16 LoRA: the norms write into the K-augmented [x | s t] operands."""
    cfg = _cfgs()["llama_hd64"]
    ms = []
    for dt, dev in ((torch.float32, None), (torch.bfloat16, "cuda")):
        torch.manual_seed(0)
        m = build_model(cfg.replace(dtype=dt), device=dev) if dev else build_model(cfg.replace(dtype=dt))
        for p in m.parameters():
            p.requires_grad = False
        replace_linear_with_lora(m, rank=16, alpha=32)
        for mod in m.modules():
            if hasattr(mod, "B") and isinstance(mod.B, torch.nn.Parameter):
                torch.nn.init.normal_(mod.B, std=0.05)
        m.flatten()
        ms.append(m)
    ms[1].load_state_dict(ms[0].state_dict())
    blk = ms[1].computes[1]
    assert blk.qkv.kaug_input(torch.zeros(MIN_CHUNK_ROWS, cfg.emb_dim, device=DEV, dtype=torch.bfloat16),
                              cfg.emb_dim) is not None
    _check_model(ms[0], ms[1], torch.bfloat16)
