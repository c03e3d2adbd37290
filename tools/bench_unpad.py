#!/usr/bin/env python3
"""Padded vs unpadded instruction-finetuning step (GPU): the ``llama32_1b_lora_alpaca`` workload of
bench.py -- Llama-3.2-1B bf16, frozen base, LoRA r=16 alpha=32 on every linear, synthetic Alpaca
records through InstructionDataset and the reference collate at context 1024, FusedAdamW -- run in
ONE process, the same batches fed to ``model(x, y)`` and to ``model(x, y, seq_lens=...)``,
interleaved A B A B.

One repeat = the same ``--steps`` batches in order, each batch first padded then unpadded; the
first repeat is the warm-up (every batch shape in both forms) and is not reported.  A repeat's
figure is its mean ms/step over those batches, so the repeats of one arm differ only by noise:
the unpadded step counts as faster only if its mean lies below the padded one by more than the
spread (max - min) of the padded repeats.

Also timed, once: the attention kernels on uniform lengths (B = 96, T = 256, H / G = 32 / 8,
hd 64) through the uniform op and through the variable-length op.

Prints one JSON line.  Usage: python tools/bench_unpad.py [--batch_size 96] [--steps 8]
[--repeats 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time
from functools import partial

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_llm_from_scratch_amd import ops  # noqa: E402
from building_llm_from_scratch_amd.config import get_config  # noqa: E402
from building_llm_from_scratch_amd.data.datasets import InstructionDataset, custom_collate_fn, unpad_lengths  # noqa: E402
from building_llm_from_scratch_amd.data.synthetic import alpaca_records  # noqa: E402
from building_llm_from_scratch_amd.data.tokenizer import build_tokenizer  # noqa: E402
from building_llm_from_scratch_amd.models import build_model, replace_linear_with_lora  # noqa: E402
from building_llm_from_scratch_amd.train.optim import FusedAdamW  # noqa: E402


def batches(cfg, model_name, batch_size, n):
    """The first ``n`` shuffled batches of the preset's loader (host tensors)."""
    from torch.utils.data import DataLoader
    tok = build_tokenizer(model_name, cfg, None)
    ds = InstructionDataset(alpaca_records(4096, seed=123), tok)
    collate = partial(custom_collate_fn, pad_token_id=cfg.eos_id, allowed_max_length=cfg.context_length)
    dl = DataLoader(ds, batch_size=batch_size, shuffle=True, drop_last=True, collate_fn=collate,
                    generator=torch.Generator().manual_seed(1000))
    out = []
    for xy in dl:
        out.append(xy)
        if len(out) == n:
            break
    return out, type(tok).__name__


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def attention_kernels(iters=20, B=96, T=256, H=32, G=8, hd=64):
    """Uniform lengths through both ops, interleaved: ms per call and whether the results agree."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * T, (H + 2 * G) * hd, device=dev, generator=g).to(torch.bfloat16)
    do = torch.randn(B * T, H * hd, device=dev, generator=g).to(torch.bfloat16)
    cos, sin = ops.rope_tables(hd, T, 500000.0, device=dev)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * T
    pos = (torch.arange(B * T, device=dev) % T).to(torch.int32)
    o, lse = ops.flash_attn_fwd(qkv, B, T, H, G, hd, True)
    ov, lsev = ops.flash_attn_varlen_fwd(qkv, cu, T, H, G, hd)
    d = ops.flash_attn_bwd(qkv, o, lse, do, B, T, H, G, hd, True, rope=(cos, sin))
    dv = ops.flash_attn_varlen_bwd(qkv, ov, lsev, do, cu, pos, T, H, G, hd, rope=(cos, sin))
    fns = {"fwd_uniform": lambda: ops.flash_attn_fwd(qkv, B, T, H, G, hd, True),
           "fwd_varlen": lambda: ops.flash_attn_varlen_fwd(qkv, cu, T, H, G, hd),
           "bwd_uniform": lambda: ops.flash_attn_bwd(qkv, o, lse, do, B, T, H, G, hd, True, rope=(cos, sin)),
           "bwd_varlen": lambda: ops.flash_attn_varlen_bwd(qkv, ov, lsev, do, cu, pos, T, H, G, hd, rope=(cos, sin))}
    ms = {k: [] for k in fns}
    for _ in range(3):                      # three interleaved rounds of every arm
        for k, fn in fns.items():
            ms[k].append(round(timeit(fn, iters), 4))
    return {"shape": dict(B=B, T=T, H=H, G=G, hd=hd, dtype="bf16"), "iters": iters, "ms": ms,
            "bitwise_equal": bool(torch.equal(o, ov) and torch.equal(lse.reshape(-1), lsev) and torch.equal(d, dv))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_size", type=int, default=96)
    ap.add_argument("--steps", type=int, default=8, help="batches per repeat")
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats (one more runs first as warm-up)")
    ap.add_argument("--model", default="llama3_2")
    ap.add_argument("--num_params", default="1B")
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--lora_rank", type=int, default=16)
    ap.add_argument("--lora_alpha", type=int, default=32)
    ap.add_argument("--layers", type=int, default=None, help="(debug only) override n_layers")
    ap.add_argument("--no_kernels", action="store_true", help="skip the attention-kernel timing")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unpad.py measures on the GPU; none found")
    ops.load_ext(required=True)
    dev = torch.device("cuda", 0)
    cfg = get_config(a.model, a.num_params, context_length=a.seq_len).replace(dtype=torch.bfloat16)
    if a.layers:
        cfg = cfg.replace(n_layers=a.layers)
    torch.manual_seed(123)
    model = build_model(cfg, use_actv_ckpt="none", device=dev)
    for p in model.parameters():
        p.requires_grad = False
    replace_linear_with_lora(model, rank=a.lora_rank, alpha=a.lora_alpha)
    model.flatten()
    opt = FusedAdamW(model, lr=3e-4, weight_decay=0.1)
    data, tok_name = batches(cfg, a.model, a.batch_size, a.steps)
    lens = [unpad_lengths(y) for _, y in data]
    real = sum(int(n.sum()) for n in lens)
    padded = sum(x.numel() for x, _ in data)

    def step(i, unpad):
        x, y = data[i]
        opt.zero_grad()
        if unpad:    # lengths and packing on the host tensors, as Trainer(unpad=True) does
            loss = model(x, y, seq_lens=unpad_lengths(y))
        else:
            loss = model(x.to(dev, non_blocking=True), y.to(dev, non_blocking=True))
        loss.backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        return loss

    ms = {"padded": [], "unpadded": []}
    losses = {"padded": [], "unpadded": []}
    for rep in range(a.repeats + 1):
        tot = {"padded": 0.0, "unpadded": 0.0}
        for i in range(len(data)):
            for arm, unpad in (("padded", False), ("unpadded", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = step(i, unpad)
                torch.cuda.synchronize()
                tot[arm] += time.perf_counter() - t0
                if rep == 0:
                    losses[arm].append(round(loss.item(), 4))
        if rep:
            for arm in tot:
                ms[arm].append(round(1e3 * tot[arm] / len(data), 3))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    spread = max(ms["padded"]) - min(ms["padded"])
    res = {"tool": "bench_unpad", "model": f"{a.model} {a.num_params}", "layers": cfg.n_layers,
           "lora": {"rank": a.lora_rank, "alpha": a.lora_alpha}, "batch_size": a.batch_size, "context": a.seq_len,
           "tokenizer": tok_name, "batches_per_repeat": len(data), "repeats": a.repeats,
           "real_row_share": round(real / padded, 4), "padded_rows_per_step": padded / len(data),
           "real_rows_per_step": real / len(data),
           "ms_per_step": ms, "ms_per_step_mean": {k: round(v, 3) for k, v in mean.items()},
           "padded_spread_ms": round(spread, 3),
           "real_tokens_per_s": {k: round(real / len(data) / (v * 1e-3), 1) for k, v in mean.items()},
           "speedup": round(mean["padded"] / mean["unpadded"], 4),
           "unpadded_faster": bool(mean["padded"] - mean["unpadded"] > spread),
           # the two arms share the weights, so these differ by the updates in between: a sanity trace only
           "first_losses": losses,
           "peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
           "device": torch.cuda.get_device_name(0)}
    if not a.no_kernels:
        res["attention_kernels_uniform_lengths"] = attention_kernels()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
