"""Unpadded instruction finetuning (``seq_lens`` / ``--unpad``) on the CPU: the length helper, the
variable-length oracle ops, and the packed model against the padded one (loss and every gradient),
which is a tight oracle -- the trailing ignored positions of a collated batch cannot reach the
loss."""
import json
import os
import subprocess
import sys

import pytest
import torch

from building_llm_from_scratch_amd import cli
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.data.datasets import custom_collate_fn, unpad_lengths
from building_llm_from_scratch_amd.models import build_model, replace_linear_with_lora
from building_llm_from_scratch_amd.models.head import MIN_CHUNK_ROWS
from building_llm_from_scratch_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 96   # pad token id of the tiny vocabulary (97 entries)


def _records(lengths, instr=2):
    """(instruction length, token ids) items as InstructionDataset yields them."""
    g = torch.Generator().manual_seed(7)
    return [(min(instr, n), torch.randint(0, PAD, (n,), generator=g).tolist()) for n in lengths]


def _loop_lengths(targets, ignore_index=-100):
    out = []
    for row in targets.tolist():
        n = 0
        for i, t in enumerate(row):
            if t != ignore_index:
                n = i + 1
        out.append(n)
    return out


# ------------------------------------------------------------------ unpad_lengths
def test_unpad_lengths_matches_loop():
    # one record that fills allowed_max_length (truncated: no end-of-text target survives), a
    # one-token record, ordinary ones
    x, y = custom_collate_fn(_records([9, 40, 1, 20, 31]), pad_token_id=PAD, allowed_max_length=32)
    lens = unpad_lengths(y)
    assert lens.dtype == torch.long and lens.device.type == "cpu" and lens.tolist() == _loop_lengths(y)
    assert lens.max().item() == 32 and x.shape == (5, 32)
    assert lens.tolist()[2] == 1          # the one-token record keeps its end-of-text target


def test_unpad_lengths_all_ignored():
    y = torch.full((3, 11), -100)
    assert unpad_lengths(y).tolist() == [0, 0, 0]
    # instruction as long as the record: every target but the end-of-text one is masked
    _, y = custom_collate_fn(_records([6, 6], instr=6), pad_token_id=PAD)
    assert unpad_lengths(y).tolist() == _loop_lengths(y)
    assert unpad_lengths(torch.full((2, 5), 7), ignore_index=7).tolist() == [0, 0]


# ------------------------------------------------------------------ oracle ops
LENS = [9, 31, 0, 2, 20]
H, G, HD = 4, 2, 16


def _packed(T=31):
    """Padded [B*T, ...] qkv and its packed rows, with cu / pos_ids."""
    g = torch.Generator().manual_seed(3)
    B = len(LENS)
    qkv = torch.randn(B * T, (H + 2 * G) * HD, generator=g)
    do = torch.randn(B * T, H * HD, generator=g)
    rows = torch.cat([torch.arange(b * T, b * T + n) for b, n in enumerate(LENS)])
    cu = torch.tensor([0] + torch.tensor(LENS).cumsum(0).tolist(), dtype=torch.int32)
    pos = torch.cat([torch.arange(n) for n in LENS]).to(torch.int32)
    return qkv, do, rows, cu, pos, B, T


def test_oracle_rope_pos_matches_padded():
    qkv, _, rows, _, pos, B, T = _packed()
    cos, sin = ref.rope_tables(HD, 32, 10000.0)
    for inverse in (False, True):
        want = ref.rope_(qkv.clone(), cos, sin, T, H, G, HD, inverse)[rows]
        got = ref.rope_pos_(qkv[rows].clone(), cos, sin, pos, H, G, HD, inverse)
        assert torch.equal(got, want)


def test_oracle_varlen_attention_matches_padded():
    qkv, do, rows, cu, pos, B, T = _packed()
    cos, sin = ref.rope_tables(HD, 32, 10000.0)
    o_pad, lse_pad = ref.flash_attn_fwd(qkv, B, T, H, G, HD, True)
    o, lse = ref.flash_attn_varlen_fwd(qkv[rows].contiguous(), cu, max(LENS), H, G, HD)
    assert o.shape == (sum(LENS), H * HD) and lse.shape == (H * sum(LENS),)
    assert torch.allclose(o, o_pad[rows], atol=1e-6, rtol=1e-5)
    for b, n in enumerate(LENS):      # lse block of sequence b: [H, len_b] at H * cu[b]
        blk = lse[H * int(cu[b]):H * int(cu[b + 1])].view(H, n)
        assert torch.allclose(blk, lse_pad[b, :, :n], atol=1e-6, rtol=1e-5)
    # backward: a real row's dq / dk / dv only sums over real rows when the padded rows' dout is 0
    do_pad = torch.zeros_like(do)
    do_pad[rows] = do[rows]
    for rope in (None, (cos, sin)):
        want = ref.flash_attn_bwd(qkv, o_pad, lse_pad, do_pad, B, T, H, G, HD, True)
        if rope is not None:
            ref.rope_(want, cos, sin, T, H, G, HD, inverse=True)
        got = ref.flash_attn_varlen_bwd(qkv[rows].contiguous(), o, lse, do[rows].contiguous(), cu, pos, max(LENS),
                                        H, G, HD, rope)
        assert torch.allclose(got, want[rows], atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------ model parity
def _small_llama(name="llama3_2", **kw):
    # tests/test_model_grads.py::_small_llama with context_length 32
    cfg = get_config(name, {"llama2": "7B", "llama3": "8B", "llama3_1": "8B", "llama3_2": "1B"}[name])
    return cfg.replace(context_length=32, emb_dim=64, n_heads=4, n_kv_groups=2 if name != "llama2" else 4,
                       hidden_dim=96, n_layers=2, vocab_size=97, dtype=torch.float32, **kw)


def _ragged_batch():
    return custom_collate_fn(_records([9, 31, 2, 20]), pad_token_id=PAD, allowed_max_length=32)


def _pair(cfg, ckpt, lora=False):
    """Two models with the same state."""
    ms = []
    for _ in range(2):
        torch.manual_seed(0)
        m = build_model(cfg, use_actv_ckpt=ckpt)
        if lora:   # the LoRA model of test_model_grads.py::test_lora_grads
            for p in m.parameters():
                p.requires_grad = False
            replace_linear_with_lora(m, rank=4, alpha=8)
            for mod in m.modules():
                if hasattr(mod, "B") and isinstance(mod.B, torch.nn.Parameter):
                    torch.nn.init.normal_(mod.B, std=0.05)
        m.flatten()
        ms.append(m)
    ms[1].load_state_dict(ms[0].state_dict())
    return ms


def _assert_same(m_pad, m_unp, x, y, lens):
    loss_pad = m_pad(x, y)
    loss_pad.backward()
    loss = m_unp(x, y, seq_lens=lens)
    loss.backward()
    assert torch.allclose(loss, loss_pad, atol=2e-5, rtol=1e-5), (loss, loss_pad)
    named = dict(m_pad.named_parameters())
    checked = 0
    for k, p in m_unp.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and named[k].grad is not None, k
        assert torch.allclose(p.grad.float(), named[k].grad.float(), atol=2e-5, rtol=1e-4), \
            (k, (p.grad.float() - named[k].grad.float()).abs().max())
        checked += 1
    assert checked


@pytest.mark.parametrize("ckpt", ["none", "selective", "full"])
@pytest.mark.parametrize("name", ["llama3_2", "llama2"])
def test_model_parity(name, ckpt):
    m_pad, m_unp = _pair(_small_llama(name), ckpt)
    x, y = _ragged_batch()
    lens = unpad_lengths(y)
    assert sorted(lens.tolist()) == [2, 9, 20, 31]
    _assert_same(m_pad, m_unp, x, y, lens)
    # the packed batch is a whole number of dW K granules; a list of lengths works too
    assert m_unp.rctx.seq.N % MIN_CHUNK_ROWS == 0 and m_unp.rctx.seq.N >= int(lens.sum())
    with torch.no_grad():
        assert torch.allclose(m_unp(x, y, seq_lens=lens.tolist()), m_pad(x, y), atol=2e-5, rtol=1e-5)
    assert m_pad.rctx.seq is None


@pytest.mark.parametrize("ckpt", ["none", "full"])
def test_model_parity_lora(ckpt):
    m_pad, m_unp = _pair(_small_llama(), ckpt, lora=True)
    x, y = _ragged_batch()
    _assert_same(m_pad, m_unp, x, y, unpad_lengths(y))
    assert all(".lora." in n for n, p in m_unp.named_parameters() if p.requires_grad)


def test_all_ignored_batch():
    _, m = _pair(_small_llama(), "none")
    x, y = _ragged_batch()
    y = torch.full_like(y, -100)
    lens = unpad_lengths(y)
    assert lens.tolist() == [0, 0, 0, 0]
    loss = m(x, y, seq_lens=lens)
    loss.backward()
    assert loss.item() == 0.0 and m.rctx.seq.N == MIN_CHUNK_ROWS
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.count_nonzero(p.grad).item() == 0, k


# ------------------------------------------------------------------ refusals
def test_refusals():
    x, y = _ragged_batch()
    lens = unpad_lengths(y)
    gpt = get_config("GPT2", "124M").replace(context_length=32, emb_dim=64, n_heads=4, n_kv_groups=4, hidden_dim=256,
                                             n_layers=2, vocab_size=97, dtype=torch.float32, drop_rate=0.0)
    with pytest.raises(NotImplementedError):
        build_model(gpt)(x, y, seq_lens=lens)
    with pytest.raises(ValueError):
        build_model(_small_llama())(x, seq_lens=lens)
    with pytest.raises(ValueError):
        build_model(_small_llama())(x, y, seq_lens=[40, 1, 1, 1])   # longer than the row


def test_cli_refusals(tmp_path):
    base = ["--data_dir", str(tmp_path), "--num_params"]
    with pytest.raises(ValueError, match="--unpad"):
        cli.perform_checks(cli.get_args(base + ["1B", "--model", "llama3_2", "--unpad"]))
    with pytest.raises(ValueError, match="--unpad"):
        cli.perform_checks(cli.get_args(base + ["124M", "--model", "GPT2", "--finetune", "--unpad"]))
    cli.perform_checks(cli.get_args(base + ["1B", "--model", "llama3_2", "--finetune", "--unpad"]))


# ------------------------------------------------------------------ CLI end to end
def _run(args, tmp_path, timeout=600):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONUNBUFFERED="1", CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "main.py")] + args
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_cli_unpad_matches_padded(tmp_path):
    rows = {}
    for tag, extra in (("pad", []), ("unpad", ["--unpad"])):
        _run(["--model", "llama3_2", "--num_params", "1B", "--debug", "--finetune", "--dataset", "alpaca",
              "--synthetic_data", "--device", "cpu", "--max_steps", "6", "--eval_freq", "2", "--no_plot",
              "--data_dir", str(tmp_path / "alpaca"), "--output_dir", str(tmp_path / f"ckpt_{tag}"),
              "--metrics_file", str(tmp_path / f"{tag}.jsonl"), "--n_epochs", "1", "--batch_size", "2",
              "--save_ckpt_freq", "100", "--print_sample_iter", "100", "--sample_tokens", "3",
              "--skip_final_save"] + extra, tmp_path)
        rows[tag] = [json.loads(line) for line in open(tmp_path / f"{tag}.jsonl")]
    assert rows["pad"] and len(rows["pad"]) == len(rows["unpad"])
    compared = 0
    for a, b in zip(rows["pad"], rows["unpad"]):
        assert a.keys() == b.keys()            # no metrics key added or renamed
        for key in ("train_loss", "val_loss"):
            if key in a and a[key] is not None:
                assert abs(a[key] - b[key]) <= 1e-5 * abs(a[key]), (key, a[key], b[key])
                compared += 1
    assert compared >= 2
