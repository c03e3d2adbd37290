"""Gradient accumulation (``--grad_accum_steps``, train/accum.py) on the CPU, fp32: K micro-batches
must take the step that one batch made of their rows takes -- driver, hygiene, Trainer accounting,
the engines on gloo, the collective plan, fp16 loss scaling, resume and the CLI."""
import functools
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile
from collections import Counter
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from building_llm_from_scratch_amd import cli
from building_llm_from_scratch_amd.config import get_config
from building_llm_from_scratch_amd.data.datasets import custom_collate_fn
from building_llm_from_scratch_amd.parallel import setup_engine
from building_llm_from_scratch_amd.train.accum import accumulate_step, micro_weights
from building_llm_from_scratch_amd.train.optim import FusedAdamW
from building_llm_from_scratch_amd.train.trainer import DynamicLossScaler, Trainer

import test_distributed as td
from test_unpad_cpu import PAD, _pair, _records, _small_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = (1, 3, 2)   # rows per micro-batch: unequal non-ignored target counts


def _gpt2():
    return get_config("GPT2", "124M").replace(context_length=32, emb_dim=64, n_heads=4, n_kv_groups=4, hidden_dim=256,
                                             n_layers=2, vocab_size=97, dtype=torch.float32, drop_rate=0.0)


def _six():
    return custom_collate_fn(_records([9, 31, 2, 20, 14, 5]), pad_token_id=PAD, allowed_max_length=32)


def _split(x, y, sizes=SPLIT):
    out, r = [], 0
    for n in sizes:
        out.append((x[r:r + n], y[r:r + n]))
        r += n
    assert r == x.shape[0]
    return out


def _assert_step_equal(m_one, m_acc, loss_one, loss_acc):
    assert torch.allclose(loss_acc, loss_one, atol=2e-5, rtol=1e-5), (loss_acc, loss_one)
    named = dict(m_one.named_parameters())
    checked = 0
    for k, p in m_acc.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and named[k].grad is not None, k
        assert torch.allclose(p.grad.float(), named[k].grad.float(), atol=2e-5, rtol=1e-4), \
            (k, (p.grad.float() - named[k].grad.float()).abs().max())
        checked += 1
    assert checked


MODELS = {"llama3_2": (lambda: _small_llama("llama3_2"), False), "llama2": (lambda: _small_llama("llama2"), False),
          "gpt2": (_gpt2, False), "lora": (lambda: _small_llama("llama3_2"), True)}


# ------------------------------------------------------------------ 1. driver against one batch
@pytest.mark.parametrize("ckpt", ["none", "selective", "full"])
@pytest.mark.parametrize("name", list(MODELS))
def test_driver_matches_one_batch(name, ckpt):
    cfg, lora = MODELS[name]
    m_one, m_acc = _pair(cfg(), ckpt, lora=lora)
    x, y = _six()
    micro = _split(x, y)
    w, n = micro_weights(micro)
    assert len(set(n)) == 3 and abs(sum(w) - 1.0) < 1e-12     # the n_i really differ
    loss_one = m_one(x, y)
    loss_one.backward()
    loss_acc = accumulate_step(m_acc, micro)
    assert m_acc.rctx.accumulate is False
    _assert_step_equal(m_one, m_acc, loss_one, loss_acc)


@pytest.mark.parametrize("ckpt", ["none", "full"])
@pytest.mark.parametrize("name", ["llama3_2", "lora"])
def test_driver_unpad_matches_padded_batch(name, ckpt):
    cfg, lora = MODELS[name]
    m_one, m_acc = _pair(cfg(), ckpt, lora=lora)
    x, y = _six()
    loss_one = m_one(x, y)
    loss_one.backward()
    loss_acc = accumulate_step(m_acc, _split(x, y), unpad=True)
    assert m_acc.rctx.seq is not None            # the packed path ran
    _assert_step_equal(m_one, m_acc, loss_one, loss_acc)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("name", ["llama3_2", "gpt2"])
def test_group_with_all_ignored_micro_batch(name, which):
    m_one, m_acc = _pair(MODELS[name][0](), "none")
    x, y = _six()
    y = y.clone()
    r0 = sum(SPLIT[:which])
    y[r0:r0 + SPLIT[which]] = -100
    micro = _split(x, y)
    assert micro_weights(micro)[0][which] == 0.0
    loss_one = m_one(x, y)
    loss_one.backward()
    _assert_step_equal(m_one, m_acc, loss_one, accumulate_step(m_acc, micro))


@pytest.mark.parametrize("unpad", [False, True])
def test_all_ignored_group(unpad):
    _, m = _pair(_small_llama(), "none")
    x, y = _six()
    # a real step first: the all-ignored group must overwrite its gradients, not keep them
    accumulate_step(m, _split(x, y))
    loss = accumulate_step(m, _split(x, torch.full_like(y, -100)), unpad=unpad)
    assert loss.item() == 0.0
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.count_nonzero(p.grad).item() == 0, k


# ------------------------------------------------------------------ 2. hygiene
@pytest.mark.parametrize("name", ["llama3_2", "gpt2"])
def test_plain_step_after_accumulated_step_overwrites(name):
    m_fresh, m = _pair(MODELS[name][0](), "selective")
    x, y = _six()
    accumulate_step(m, _split(x, y))
    x2, y2 = custom_collate_fn(_records([12, 7, 25]), pad_token_id=PAD, allowed_max_length=32)
    m(x2, y2).backward()                                   # the K = 1 path of the Trainer
    m_fresh(x2, y2).backward()
    named = dict(m_fresh.named_parameters())
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, named[k].grad), k


def test_exception_in_micro_step_leaves_accumulate_off():
    _, m = _pair(_small_llama(), "none")
    x, y = _six()
    real, calls = m.forward, []

    def forward(*a, **kw):
        calls.append(m.rctx.accumulate)
        if len(calls) == 2:
            raise RuntimeError("boom")
        return real(*a, **kw)

    m.forward = forward
    with pytest.raises(RuntimeError, match="boom"):
        accumulate_step(m, _split(x, y))
    assert calls == [False, True]             # it was thrown inside micro-step 1, accumulate on
    assert m.rctx.accumulate is False


# ------------------------------------------------------------------ 3. Trainer
class _Loader(SimpleNamespace):
    def get_total_steps_epoch(self, files):
        return sum(self.counts[f] for f in files)


def _trainer(m, k, tmp_path, **kw):
    opt = FusedAdamW(m, lr=1e-2, weight_decay=0.1)
    loader = _Loader(batch_size=2, tokenizer=None, counts={"a": 5, "b": 4})
    kw.setdefault("max_grad_norm", 0.5)
    return Trainer(m, opt, m.cfg, ["a", "b"], loader, tmp_path, warmup_steps=2, device="cpu", eval_freq=10 ** 6,
                   save_ckpt_freq=0, print_sample_iter=0, grad_accum_steps=k, **kw)


def _instr_batches(n, rows=2):
    """``n`` micro-batches of ``rows`` rows; each consecutive pair is one collated batch cut in two
    (the collate pads to the batch's longest record), so a pair concatenates back to it."""
    g = torch.Generator().manual_seed(3)
    out = []
    for _ in range(n // 2):
        lens = torch.randint(3, 30, (2 * rows,), generator=g).tolist()
        x, y = custom_collate_fn(_records(lens), pad_token_id=PAD, allowed_max_length=32)
        out += [(x[:rows], y[:rows]), (x[rows:], y[rows:])]
    return out


def test_trainer_matches_concatenated_batches(tmp_path):
    m1, m2 = _pair(_small_llama(), "none")
    t1, t2 = _trainer(m1, 1, tmp_path), _trainer(m2, 2, tmp_path)
    for t in (t1, t2):
        t.count_target_tokens = True
        t._setup_schedule(1)
    # 9 loader batches in files of 5 and 4: 9 optimizer steps at K = 1, 3 + 2 at K = 2
    assert t1.total_training_steps == 9 and t2.total_training_steps == 5
    micro = _instr_batches(6)
    t1.total_training_steps = t2.total_training_steps
    losses = []
    for s in range(3):
        a, b = micro[2 * s], micro[2 * s + 1]
        l1 = t1.train_batch(torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]))
        l2 = t2.train_group([a, b])
        losses.append((float(l1.detach()), float(l2)))
    for l1, l2 in losses:
        assert abs(l1 - l2) < 1e-4, losses
    t1._flush_tokens(), t2._flush_tokens()
    assert t1.global_step == t2.global_step == 2
    assert len(t1.track_lrs) == len(t2.track_lrs) == 3 and t1.track_lrs == t2.track_lrs
    assert len(set(t1.track_lrs)) == 3                      # warm-up then cosine: the LR really moved
    assert t1.tokens_seen == t2.tokens_seen == sum(int((y != -100).sum()) for _, y in micro)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.allclose(sd1[k], sd2[k], atol=1e-4, rtol=1e-4), (k, (sd1[k] - sd2[k]).abs().max())
    assert m2.rctx.accumulate is False


def test_train_epoch_groups_and_short_last_group(tmp_path):
    _, m = _pair(_small_llama(), "none")
    tr = _trainer(m, 2, tmp_path)
    tr._setup_schedule(1)
    sizes = []
    real = tr.train_group
    tr.train_group = lambda group: (sizes.append(len(group)), real(group))[1]
    g = torch.Generator().manual_seed(5)
    data = [torch.randint(0, 97, (2, 17), generator=g) for _ in range(5)]
    batches = [(b[:, :-1], b[:, 1:]) for b in data]
    tr.global_step = 0       # (step 0 is an eval point of the loop; not what this test is about)
    tr.train_epoch(0, batches, batches, file_index=0)
    assert sizes == [2, 2, 1] and tr.global_step == 3
    assert tr.pos == (0, 0, 5)                              # loader batches consumed
    tr._flush_tokens()
    assert tr.tokens_seen == 5 * 2 * 16


# ------------------------------------------------------------------ 4. engines on gloo
@functools.lru_cache(maxsize=None)
def _reference(family, lora, odd=False, rows=4):
    return td._reference(family, lora, odd=odd, rows=rows)


def _engine_worker(rank, world, kind, family, lora, out, store, opts):
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    try:
        cfg, m = td._build(family, lora, odd=opts.get("odd", False))
        eng = setup_engine(m, kind, device="cpu", bucket_mb=0.05, reduce_dtype=opts.get("reduce_dtype"), prefetch=1)
        opt = FusedAdamW(m, lr=1e-2, weight_decay=0.1, engine=eng)
        freed = []
        if kind == "fsdp":
            real = eng.finish_backward

            def finish_backward():
                real()
                freed.append(all(u.train.grad.untyped_storage().size() == 0
                                 for u in eng.units if u.train is not None))
            eng.finish_backward = finish_backward
        rows, K = opts.get("rows", 4), 2
        per = rows // world
        half = per // K
        losses = []
        for b in td._data(cfg, rows):
            mine = b[rank * per:(rank + 1) * per]
            micro = [(mine[i * half:(i + 1) * half, :-1], mine[i * half:(i + 1) * half, 1:]) for i in range(K)]
            opt.zero_grad()
            loss = accumulate_step(m, micro)
            opt.clip_grad_norm_(0.5)
            opt.step()
            losses.append(loss.float().item())
        if kind == "fsdp":
            assert len(freed) == td.STEPS * K and all(freed), freed
        assert m.rctx.accumulate is False
        t = torch.tensor(losses)
        dist.all_reduce(t)
        sd = eng.full_state_dict() if hasattr(eng, "full_state_dict") else \
            {k: v.detach().clone() for k, v in m.state_dict().items()}
        if rank == 0:
            torch.save({"sd": sd, "losses": (t / world).tolist()}, out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn_engine(world, kind, family, lora, **opts):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "r.pt")
        mp.start_processes(_engine_worker, args=(world, kind, family, lora, out, os.path.join(d, "store"), opts),
                           nprocs=world, join=True, start_method="spawn")
        return torch.load(out, weights_only=True)


@pytest.mark.parametrize("kind", ["ddp", "zero1", "fsdp"])
@pytest.mark.parametrize("family,lora", [("llama", False), ("gpt2", False), ("llama", True)])
def test_engine_k2_matches_single_process(kind, family, lora):
    ref_sd, ref_losses = _reference(family, lora)
    td._check(_spawn_engine(2, kind, family, lora), ref_sd, ref_losses)


def test_fsdp_world4_padding_forcing_flats():
    ref_sd, ref_losses = _reference("llama", False, odd=True, rows=8)
    td._check(_spawn_engine(4, "fsdp", "llama", False, odd=True, rows=8), ref_sd, ref_losses)


@pytest.mark.parametrize("kind", ["zero1", "fsdp"])
def test_engine_k2_bf16_reduce_dtype(kind):
    ref_sd, ref_losses = _reference("llama", False)
    res = _spawn_engine(2, kind, "llama", False, reduce_dtype=torch.bfloat16)
    td._check(res, ref_sd, ref_losses, tol=3e-2)   # the bound of test_bf16_hybrid_reduce_dtype
    assert max((res["sd"][k].float() - ref_sd[k].float()).abs().max().item() for k in ref_sd) > 0.0


def _order_worker(rank, world, store, out):
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    try:
        from building_llm_from_scratch_amd.parallel.commplan import step_plan
        from building_llm_from_scratch_amd.parallel.seqcheck import CollectiveSequence
        cfg, m = td._build("llama", False)
        eng = setup_engine(m, "fsdp", device="cpu", prefetch=1)
        opt = FusedAdamW(m, lr=1e-3, weight_decay=0.0, engine=eng)
        tr = Trainer(m, opt, cfg, [], SimpleNamespace(batch_size=1, tokenizer=None), "/tmp", device="cpu", rank=rank,
                     world_size=world, engine=eng, comm_adapt_steps=1, grad_accum_steps=2)
        tr._seq_timeout_s = 60.0
        counts, verify = [], CollectiveSequence.verify
        CollectiveSequence.verify = lambda self, tag: (counts.append(verify(self, tag)), counts[-1])[1]
        for b in td._data(cfg, 4):
            mine = b[2 * rank:2 * rank + 2]
            tr.train_group([(mine[:1, :-1], mine[:1, 1:]), (mine[1:, :-1], mine[1:, 1:])])
        out[rank] = (tr._seq.checks, counts, len(step_plan(eng, grad_accum_steps=2)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_order_check_records_the_whole_optimizer_step():
    """The warm-up collective-order check (parallel/seqcheck.py) wraps all K micro-steps: what it
    compares across ranks for a steady-state step is the whole K = 2 plan."""
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_order_worker, args=(2, os.path.join(d, "store"), out), nprocs=2, join=True,
                           start_method="spawn")
    res = dict(out)
    for r in (0, 1):
        checks, counts, plan = res[r]
        assert checks == 2 and len(counts) == 2, res      # steps 0 and 1 (comm_adapt_steps=1)
        assert counts[1] == plan > 0, res


# ------------------------------------------------------------------ 5. collective plan
def _plan_worker(kind, q):
    try:
        from torch.testing._internal.distributed.fake_pg import FakeStore

        from building_llm_from_scratch_amd.models import build_model
        from building_llm_from_scratch_amd.parallel.commplan import Recorder, step_plan

        dist.init_process_group("fake", rank=3, world_size=8, store=FakeStore())
        cfg = get_config("llama3_2", "1B").replace(context_length=32, emb_dim=128, n_heads=4, n_kv_groups=2,
                                                   hidden_dim=192, n_layers=3, vocab_size=301, dtype=torch.float32)
        torch.manual_seed(0)
        m = build_model(cfg, use_actv_ckpt="selective")
        rec = Recorder(execute=True)
        with rec.active():
            eng = setup_engine(m, kind, device="cpu", bucket_mb=0.05, prefetch=1)
            opt = FusedAdamW(m, lr=1e-3, weight_decay=0.1, engine=eng)
            idx = torch.randint(0, cfg.vocab_size, (6, 17))
            micro = [(idx[2 * i:2 * i + 2, :-1], idx[2 * i:2 * i + 2, 1:]) for i in range(3)]
            for step in range(2):
                rec.phase = f"step{step}"
                accumulate_step(m, micro)
                opt.clip_grad_norm_(1.0)
                opt.step()
        got = [(e["op"], e["bytes"]) for e in rec.log if e["phase"] == "step1"]
        want = [(e["op"], e["bytes"]) for e in step_plan(eng, grad_accum_steps=3)]
        assert got and Counter(got) == Counter(want), (sorted(Counter(got).items()), sorted(Counter(want).items()))
        one = step_plan(eng)
        assert one == step_plan(eng, grad_accum_steps=1)
        if kind == "fsdp":
            c1, c3 = Counter((e["op"], e["phase"]) for e in one), Counter((e["op"], e["phase"]) for e in
                                                                          step_plan(eng, grad_accum_steps=3))
            assert c3[("all_reduce", "clip")] == c1[("all_reduce", "clip")] == 1
            for key in (("all_gather", "forward"), ("all_gather", "backward"), ("reduce_scatter", "backward")):
                assert c3[key] == 3 * c1[key] > 0
        else:
            assert one == step_plan(eng, grad_accum_steps=3)
        dist.destroy_process_group()
        q.put("ok")
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put(traceback.format_exc())


@pytest.mark.parametrize("kind", ["ddp", "zero1", "fsdp"])
def test_recorded_collectives_match_k3_plan(kind):
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_plan_worker, args=(kind, q))
    p.start()
    p.join(600)
    assert p.exitcode == 0, p.exitcode
    res = q.get(timeout=5)
    assert res == "ok", res


# ------------------------------------------------------------------ 6. fp16
def _fp16_pair():
    return _pair(_small_llama().replace(dtype=torch.float16), "none")


def test_fp16_overflow_in_one_micro_batch_skips_the_step(tmp_path):
    _, m = _fp16_pair()
    tr = _trainer(m, 2, tmp_path, loss_scaler=DynamicLossScaler(init_scale=1024.0))
    tr._setup_schedule(1)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    micro = _instr_batches(2)
    real, calls = m.forward, []

    def forward(*a, **kw):
        calls.append(1)
        if len(calls) == 2:      # micro-step 1 adds onto a gradient that already holds an inf
            m.trainable_buffers()[-1].grad[3] = float("inf")
        return real(*a, **kw)

    m.forward = forward
    tr.train_group(micro)
    assert tr.loss_scaler.scale == 512.0 and tr.global_step == 0
    after = m.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    # the next, clean group steps at the halved scale
    tr.train_group(micro)
    assert tr.loss_scaler.scale == 512.0 and tr.loss_scaler.clean == 1
    assert any(not torch.equal(before[k], v) for k, v in m.state_dict().items())


def test_fp16_scaled_group_matches_unscaled():
    """fp16 keeps 11 significant bits (eps 4.9e-4).  Both runs round every product and sum of the
    same backward, and once more per micro-step, at different magnitudes, so an entry may differ by
    a few eps of the tensor's largest entry: the bound is 1e-2 of it (20 eps)."""
    m_a, m_b = _fp16_pair()
    micro = _instr_batches(2)
    la = accumulate_step(m_a, micro)
    lb = accumulate_step(m_b, micro, loss_scale=1024.0)
    assert m_b.rctx.loss_scale == 1024.0
    assert abs(float(la) - float(lb)) <= 1e-3 * abs(float(la))
    named = dict(m_a.named_parameters())
    for k, p in m_b.named_parameters():
        ga, gb = named[k].grad.float(), p.grad.float() / 1024.0
        assert torch.isfinite(gb).all(), k
        assert (ga - gb).abs().max() <= 1e-2 * ga.abs().max(), (k, (ga - gb).abs().max(), ga.abs().max())


# ------------------------------------------------------------------ 7. resume
def _main(args, cwd, check=True, timeout=900):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONUNBUFFERED="1", CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=timeout)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_resume_k2_matches_uninterrupted_and_refuses_k3(tmp_path):
    steps, half = 6, 3
    common = ["--model", "GPT2", "--num_params", "124M", "--debug", "--data_dir", str(tmp_path / "data"),
              "--synthetic_data", "--n_epochs", "1", "--eval_freq", "1", "--print_sample_iter", "100", "--batch_size",
              "2", "--device", "cpu", "--no_plot", "--sample_tokens", "2", "--save_resume_state", "--max_steps",
              str(steps), "--save_ckpt_freq", str(half), "--num_workers", "0"]
    k2 = ["--grad_accum_steps", "2"]
    a, b = tmp_path / "a", tmp_path / "b"
    _main(common + k2 + ["--output_dir", str(a), "--metrics_file", str(tmp_path / "a.jsonl")], tmp_path)
    ck = a / f"model_pg_{half}.pth"
    assert ck.exists()
    _main(common + k2 + ["--output_dir", str(b), "--metrics_file", str(tmp_path / "b.jsonl"), "--resume", str(ck)],
          tmp_path)
    la = {r["step"]: r["batch_loss"] for r in map(json.loads, open(tmp_path / "a.jsonl"))}
    lb = {r["step"]: r["batch_loss"] for r in map(json.loads, open(tmp_path / "b.jsonl"))}
    assert sorted(lb) == list(range(half + 1, steps)), sorted(lb)
    for s in lb:
        assert abs(la[s] - lb[s]) <= 1e-6, (s, la[s], lb[s])
    sa = torch.load(a / "model_pg_final.pth", weights_only=True)
    sb = torch.load(b / "model_pg_final.pth", weights_only=True)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.allclose(sa[k].float(), sb[k].float(), atol=1e-6, rtol=0), (k, (sa[k] - sb[k]).abs().max())
    r = _main(common + ["--grad_accum_steps", "3", "--output_dir", str(tmp_path / "c"), "--resume", str(ck)],
              tmp_path, check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "--grad_accum_steps 2" in r.stderr, r.stderr[-2000:]


def test_trainer_state_k_mismatch_and_old_states(tmp_path):
    _, m = _pair(_small_llama(), "none")
    st = _trainer(m, 2, tmp_path).trainer_state()
    assert st["grad_accum_steps"] == 2
    _trainer(m, 2, tmp_path).load_trainer_state(st)
    with pytest.raises(ValueError, match="grad_accum_steps"):
        _trainer(m, 3, tmp_path).load_trainer_state(st)
    old = dict(st)
    old.pop("grad_accum_steps")                  # written before the key existed: K = 1
    _trainer(m, 1, tmp_path).load_trainer_state(old)
    with pytest.raises(ValueError, match="grad_accum_steps"):
        _trainer(m, 2, tmp_path).load_trainer_state(old)


# ------------------------------------------------------------------ 8. CLI
def test_cli_refuses_k0(tmp_path):
    base = ["--data_dir", str(tmp_path), "--num_params", "1B", "--model", "llama3_2"]
    with pytest.raises(ValueError, match="--grad_accum_steps"):
        cli.perform_checks(cli.build_parser().parse_args(base + ["--grad_accum_steps", "0"]))
    assert cli.get_args(base).grad_accum_steps == 1
    with pytest.raises(ValueError):
        Trainer(None, SimpleNamespace(param_groups=[{"lr": 1.0}]), None, [], None, tmp_path, grad_accum_steps=0)


@pytest.mark.parametrize("mode", ["finetune_unpad", "pretrain"])
def test_cli_k2_counts_optimizer_steps(tmp_path, mode):
    """K = 2 for 4 optimizer steps reads the 8 loader batches that K = 1 reads in 8 steps (the
    shuffle is seeded per epoch and file): the token count after step s is K = 1's after 2s + 1.
    The debug model's context is 10 tokens, shorter than an instruction prompt, so the debug
    finetune has no non-ignored target and its counts are all 0 (every group is the all-ignored
    one, packed by ``--unpad``); the pretraining run is the one with a count to get wrong."""
    what = (["--finetune", "--dataset", "alpaca", "--unpad"] if mode == "finetune_unpad" else ["--synthetic_mb", "0.05"])
    rows = {}
    for tag, extra in (("k1", ["--max_steps", "8"]), ("k2", ["--grad_accum_steps", "2", "--max_steps", "4"])):
        r = _main(["--model", "llama3_2", "--num_params", "1B", "--debug", "--synthetic_data", "--device", "cpu",
                   "--eval_freq", "1", "--no_plot", "--data_dir", str(tmp_path / "data"), "--output_dir",
                   str(tmp_path / f"ckpt_{tag}"), "--metrics_file", str(tmp_path / f"{tag}.jsonl"), "--n_epochs", "1",
                   "--batch_size", "2", "--save_ckpt_freq", "100", "--print_sample_iter", "100", "--sample_tokens",
                   "3", "--skip_final_save", "--num_workers", "0"] + what + extra, tmp_path)
        rows[tag] = [json.loads(line) for line in open(tmp_path / f"{tag}.jsonl")]
    assert "2 rows x 2 micro-batches x 1 rank(s) = 4 rows per optimizer step" in r.stdout + r.stderr
    assert [r["step"] for r in rows["k2"]] == [0, 1, 2, 3]
    assert [r["step"] for r in rows["k1"]] == list(range(8))
    for s, r in enumerate(rows["k2"]):
        assert r["tokens_seen"] == rows["k1"][2 * s + 1]["tokens_seen"], (s, r)
        assert r["lr"] == rows["k1"][s]["lr"]      # warm-up (10 steps) counts optimizer steps
    if mode == "pretrain":
        assert rows["k2"][3]["tokens_seen"] == 8 * 2 * 10 and rows["k2"][3]["batch_loss"] > 0
    assert rows["k2"][0].keys() == rows["k1"][0].keys()
