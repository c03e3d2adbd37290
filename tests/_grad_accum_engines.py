"""Gradient accumulation under the engines on ONE MI355X with real kernels (run as a subprocess by
tests/test_grad_accum_gpu.py), in the two rehearsals of tests/_rehearse_engines.py and
tests/_world2_one_gpu.py:

  ``rccl``  one process, RCCL world 1 with ``BLLM_FORCE_COMM=1``: the engines' real collectives;
  ``gloo2`` two processes sharing cuda:0 over gloo: real shards and two different gradients.

FSDP / ZeRO-1 / DDP take every optimizer step over K = 2 micro-batches (train/accum.py) of half
this rank's rows -- bf16 Llama, full activation checkpointing, 3 AdamW steps -- and are compared
with one process stepping the local engine on the whole batch, K = 1.  Prints one JSON line."""
import json
import os
import socket
import sys
from datetime import timedelta

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_llm_from_scratch_amd import ops  # noqa: E402
from building_llm_from_scratch_amd.config import get_config  # noqa: E402
from building_llm_from_scratch_amd.models import build_model  # noqa: E402
from building_llm_from_scratch_amd.parallel import nccl_pg_options, setup_engine  # noqa: E402
from building_llm_from_scratch_amd.train.accum import accumulate_step  # noqa: E402
from building_llm_from_scratch_amd.train.optim import FusedAdamW  # noqa: E402

CFG = dict(context_length=256, emb_dim=512, n_heads=4, n_kv_groups=2, hidden_dim=1024, n_layers=3,
           vocab_size=1024, dtype=torch.bfloat16)
K = 2


def train(kind, dev, batches, rank, world, k):
    torch.manual_seed(0)
    cfg = get_config("llama3_2", "1B").replace(**CFG)
    m = build_model(cfg, use_actv_ckpt="full", device=dev)
    eng = setup_engine(m, kind, device=dev, prefetch=1)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.1, engine=eng)
    losses = []
    for b in batches:
        n = b.shape[0] // world
        mine = b[rank * n:(rank + 1) * n]
        rows = n // k
        micro = [(mine[i * rows:(i + 1) * rows, :-1], mine[i * rows:(i + 1) * rows, 1:]) for i in range(k)]
        opt.zero_grad()
        loss = accumulate_step(m, micro)
        opt.clip_grad_norm_(1.0)
        opt.step()
        lt = loss.detach().float().reshape(1)
        if world > 1:
            dist.all_reduce(lt)
            lt /= world
        losses.append(lt.item())
    sd = eng.full_state_dict() if hasattr(eng, "full_state_dict") else m.state_dict()
    if sd is not None:
        sd = {k_: v.detach().float().cpu() for k_, v in sd.items() if not k_.endswith(("mask", "cos", "sin"))}
    info = {"no_shard": getattr(eng, "no_shard", None), "no_comm": getattr(eng, "no_comm", None)}
    del m, eng, opt
    torch.cuda.empty_cache()
    return losses, sd, info


def _batches(dev):
    g = torch.Generator(device=dev).manual_seed(5)
    return [torch.randint(0, 1024, (4, 257), device=dev, generator=g) for _ in range(3)]


def _compare(sd, ref_sd):
    return {"max_param_diff": max((sd[k] - ref_sd[k]).abs().max().item() for k in ref_sd),
            "max_rel_diff": max(((sd[k] - ref_sd[k]).norm() / (ref_sd[k].norm() + 1e-12)).item() for k in ref_sd),
            "keys_match": set(sd) == set(ref_sd)}


def rccl(kinds):
    ops.load_ext(required=True)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            timeout=timedelta(minutes=2), device_id=dev, pg_options=nccl_pg_options())
    try:
        batches = _batches(dev)
        ref_losses, ref_sd, _ = train("local", dev, batches, 0, 1, 1)
        out = {"ref_losses": ref_losses}
        for kind in kinds:
            os.environ["BLLM_FORCE_COMM"] = "1"
            losses, sd, info = train(kind, dev, batches, 0, 1, K)
            os.environ["BLLM_FORCE_COMM"] = "0"
            out[kind] = {"losses": losses, **_compare(sd, ref_sd), **info}
        print(json.dumps(out), flush=True)
    finally:
        dist.destroy_process_group()


def _gloo_worker(rank, kinds, port, q):
    try:
        ops.load_ext(required=True)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2,
                                timeout=timedelta(minutes=3))
        batches = _batches(dev)
        out = {}
        if rank == 0:
            ref_losses, ref_sd, _ = train("local", dev, batches, 0, 1, 1)
            out["ref_losses"] = ref_losses
        dist.barrier()
        for kind in kinds:
            losses, sd, _ = train(kind, dev, batches, rank, 2, K)
            if rank == 0:
                out[kind] = {"losses": losses, **_compare(sd, ref_sd)}
            dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            q.put(json.dumps(out))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put("ERROR " + traceback.format_exc())
        raise


def gloo2(kinds):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, kinds, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = q.get(timeout=300)
    except Exception:
        res = "ERROR no result from the ranks"
    for p in procs:
        p.join(5 if res.startswith("ERROR") else 60)
    for p in procs:      # a rank whose peer failed would wait in a collective: leave nothing running
        if p.is_alive():
            p.terminate()
            p.join(10)
    print(res, flush=True)
    codes = [p.exitcode for p in procs]
    sys.exit(0 if not res.startswith("ERROR") and codes == [0, 0] else 1)


if __name__ == "__main__":
    {"rccl": rccl, "gloo2": gloo2}[sys.argv[1]](sys.argv[2].split(","))
