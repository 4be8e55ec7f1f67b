"""The per-step schedule and the trainer's state_dict / load_state_dict under data parallel (workers started as
tests/test_gpu_dp.py starts them; at most two processes).  Every rank attaches the same values and the counters advance
alike with no communication; state_dict() is a collective under the sharded update (every rank makes it); replicas stay
bitwise equal to each other and to the uninterrupted two-rank run.  One rank over RCCL: the schedule's launch sits inside
the graph that holds the collective.  ``-m gpu``."""
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
OPT = dict(lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0)
GLOBAL_BATCH = 32
RATES = [0.0125, 0.011, 0.0173, 0.0091, 0.0147, 0.0033, 0.0207, 0.0061]


def _batch(step):
    g = torch.Generator().manual_seed(777 + step)
    return torch.randn(GLOBAL_BATCH, 3, 32, 32, generator=g), torch.randint(0, 10, (GLOBAL_BATCH,), generator=g)


def _model(device, seed=0):
    if str(ROOT / "nnue-vision_amd") not in sys.path:
        sys.path.insert(0, str(ROOT / "nnue-vision_amd"))
    import nnue
    torch.manual_seed(seed)
    return nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(device)


def _trainer(model, per, schedule=True, **kw):
    from nnue_hip.trainer import NnueTrainer
    tr = NnueTrainer(model, per, (32, 32), input_slots=2, **OPT, **kw)
    if schedule:
        tr.set_lr_schedule(RATES)
    return tr


def _steps(tr, first, count, sl):
    losses = []
    for s in range(first, first + count):
        images, labels = _batch(s)
        losses.append(float(tr.step(images[sl].to(tr.dev), labels[sl].to(tr.dev), slot=s % 2)))
    return losses


def _momentum(sd):
    return torch.cat([sd["optimizer"]["state"][i]["momentum_buffer"].flatten().cpu() for i in sorted(sd["optimizer"]["state"])])


def _init(rank, port, world, backend, env):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _resume_worker(rank, port, out_dir, world, env):
    dist = _init(rank, port, world, "gloo", env)
    try:
        dev, per = torch.device("cuda", 0), GLOBAL_BATCH // world
        # the uninterrupted run: six steps
        straight = _trainer(_model(dev), per)
        assert straight.sharded_update == (env.get("NNUE_DP_SHARDED_UPDATE") == "1")
        sl = straight.dp.shard(GLOBAL_BATCH)
        want_losses = _steps(straight, 0, 6, sl)
        want_sd = straight.state_dict()  # (every rank: a collective under the sharded update)
        # three steps, the state out, new model and trainer, three more
        half_model = _model(dev)
        half = _trainer(half_model, per)
        losses = _steps(half, 0, 3, sl)
        sd = half.state_dict()
        params = {k: v.clone() for k, v in half_model.state_dict().items()}
        assert sd["steps_done"] == 3 and sd["lr_schedule"]["position"] == 3
        del half
        model = _model(dev, seed=50 + rank)  # (rank-dependent start: the constructor's broadcast and the load make them one)
        model.load_state_dict(params)
        new = _trainer(model, per)
        new.load_state_dict(sd)
        losses += _steps(new, 3, 3, sl)
        got_sd = new.state_dict()
        torch.cuda.synchronize()
        torch.save({"want_flat": straight.flat_params.cpu(), "got_flat": new.flat_params.cpu(), "want_losses": want_losses, "got_losses": losses,
                    "want_momentum": _momentum(want_sd), "got_momentum": _momentum(got_sd), "lr_pos": (int(straight.lr_pos), int(new.lr_pos)),
                    "lr_dev": (float(straight.lr_dev), float(new.lr_dev)), "steps": (got_sd["steps_done"], got_sd["lr_schedule"]["position"])},
                   Path(out_dir) / f"rank{rank}.pt")
    finally:
        dist.destroy_process_group()


def _spawn(worker, tmp_path, world, *args):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(worker, args=(port, str(tmp_path), world, *args), nprocs=world, join=True)
    return [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(world)]


@pytest.mark.parametrize("env", ({}, {"NNUE_DP_SHARDED_UPDATE": "1"}), ids=("allreduce", "sharded_update"))
def test_two_ranks_resume_with_a_schedule(tmp_path, env):
    ranks = _spawn(_resume_worker, tmp_path, 2, env)
    for r in ranks:
        assert torch.equal(r["got_flat"], r["want_flat"]), "the resumed run left the uninterrupted one"
        assert torch.equal(r["got_momentum"], r["want_momentum"])
        assert r["got_losses"] == r["want_losses"]
        assert r["lr_pos"] == (6, 6) and r["steps"] == (6, 6) and r["lr_dev"][0] == r["lr_dev"][1]
        assert r["lr_dev"][0] == float(torch.tensor(RATES[5], dtype=torch.float32))
    assert torch.equal(ranks[0]["got_flat"], ranks[1]["got_flat"]), "replicas diverged"
    assert torch.equal(ranks[0]["got_momentum"], ranks[1]["got_momentum"])


def _rccl_worker(rank, port, out_dir, world, env):
    dist = _init(rank, port, world, "nccl", env)
    try:
        dev = torch.device("cuda", 0)
        tr, twin = _trainer(_model(dev), GLOBAL_BATCH), _trainer(_model(dev), GLOBAL_BATCH, schedule=False)
        assert tr.dp.collectives and tr.capture_collectives and twin.capture_collectives
        for s in range(2):
            images, labels = _batch(s)
            for t in (tr, twin):
                t.inputs[s][0].copy_(images)
                t.inputs[s][1].copy_(labels)
        values = torch.tensor(RATES, dtype=torch.float32)
        got, want, n = [], [], 0

        def single(slot):
            nonlocal n
            twin.lr = float(values[min(n, len(RATES) - 1)])
            n += 1
            return float(twin.step(slot=slot))
        for slot in (0, 1):
            got.append(float(tr.step(slot=slot)))
            want.append(single(slot))
        assert (1, "full_dp") in tr._g_local, "the second step is the graph with the collective inside"
        for group in ((0, 1), (0, 1), (1, 0, 1)):
            torch.cuda.synchronize()
            got += [float(v) for v in tr.step_many(group)]
            want += [single(s) for s in group]
            assert (group, "many") in tr._g_local
        torch.cuda.synchronize()
        torch.save({"got": got, "want": want, "got_flat": tr.flat_params.cpu(), "want_flat": twin.flat_params.cpu(),
                    "got_momentum": tr.flat_momentum.cpu(), "want_momentum": twin.flat_momentum.cpu(),
                    "lr_pos": int(tr.lr_pos), "facts": (tr.steps_done, tr.lr_position), "capture": bool(tr.capture_collectives)},
                   Path(out_dir) / f"rank{rank}.pt")
    finally:
        dist.destroy_process_group()


def test_one_rank_over_rccl_with_the_schedule_inside_the_captured_collective_graph(tmp_path):
    (r,) = _spawn(_rccl_worker, tmp_path, 1, {"NNUE_DP_FORCE_COLLECTIVES": "1"})
    assert r["capture"] and r["got"] == r["want"], (r["got"], r["want"])
    assert torch.equal(r["got_flat"], r["want_flat"]) and torch.equal(r["got_momentum"], r["want_momentum"])
    assert r["lr_pos"] == 9 and r["facts"] == (9, 9)
