"""The weight average under data parallelism (include/nnue_hip.h, "weight average"): two gloo ranks on one GPU, tests/dp_modes.py's
per-rank driver pattern, one run each for the all-reduce update, the sharded update (every rank averages its own shard; the shards
meet on demand) and the factor exchange (the small update and the table update average their own parts), and one nccl rank with the collectives forced for the
rows of dp_modes.py whose step graphs hold the collective (capture_collectives): single graph steps and a step group.  The parameters are
identical on every rank, so the average needs no communication: after every step each rank's average is bitwise the stand-alone
pass applied in that process to the previous average and the plain run's parameters, and the ranks' averages are bitwise each
other's.  The one-rank forced-collectives form covers a step group under the factor exchange.  ``-m gpu``."""
import gc
import os
import socket
from pathlib import Path

import pytest
import torch

import ema_cases as ec
import trainer_modes as tm
import dp_modes
from dp_modes import FX, SHARD
from test_gpu_update_sequence import BACKWARD_DP, EXCHANGE, FORWARD, FRONT, _logged, _trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _collect_trainers():
    """A failed test's trainers live on in its traceback; their captured graphs must be destroyed here, between tests, and not by
    a garbage collection that happens to run inside the next test's graph capture (the runtime refuses that and aborts)."""
    yield
    gc.collect()


MODES = {"all_reduce": {}, "sharded": SHARD, "factor_exchange": FX}
CFG = dict(tm.A, batch=12)
WORLD = 2


def _worker(rank: int, port: int, out_dir: str):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        batches = ec.fresh_batches(3, CFG["batch"] * WORLD, CFG["image"], CFG["classes"])
        rows = slice(rank * CFG["batch"], (rank + 1) * CFG["batch"])
        for mode, env in MODES.items():
            for k in tm.KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            with tm.trainer_for(CFG, ema_decay=ec.DECAY) as (averaged, _), tm.trainer_for(CFG) as (plain, _):
                assert averaged.mode == plain.mode and averaged.dp.world == WORLD
                assert (averaged.sharded_update, averaged.factor_exchange) == (mode == "sharded", mode == "factor_exchange"), mode
                feed = [lambda tr, b=b: tr.step(b[0][rows].to("cuda"), b[1][rows].to("cuda")) for b in batches]
                ec.pair_steps(averaged, plain, feed, f"{mode} rank {rank}")
                if mode == "sharded":  # a further step leaves the other rank's shard behind until somebody asks
                    averaged.step(batches[0][0][rows].to("cuda"), batches[0][1][rows].to("cuda"))
                    torch.cuda.synchronize()
                    per = averaged.flat_ema.numel() // WORLD
                    own = averaged.flat_ema[rank * per:(rank + 1) * per].clone()
                    state = averaged.state_dict()  # (a collective: gathers momentum and average)
                    assert torch.equal(averaged.flat_ema[rank * per:(rank + 1) * per], own)
                    assert state["ema"]["decay"] == ec.DECAY
                torch.save(averaged.flat_ema.cpu(), Path(out_dir) / f"{mode}_{rank}.pt")
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_two_ranks_average_alike_in_every_exchange(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(port, str(tmp_path)), nprocs=WORLD, join=True)  # (a rank's failed assertion raises here)
    for mode in MODES:
        a, b = (torch.load(tmp_path / f"{mode}_{r}.pt", weights_only=True) for r in range(WORLD))
        assert torch.equal(a, b), f"{mode}: the ranks' averages differ in {int((a != b).sum())} elements"


def test_factor_exchange_group_launches_the_averaging_siblings(monkeypatch, tmp_path):
    """tests/test_gpu_update_sequence.py::test_factor_exchange_update_sequence with the option on: a gloo group of one rank with
    the collectives forced, so that a step_many group runs under the factor exchange; the group is bitwise three single steps."""
    import torch.distributed as dist
    monkeypatch.setenv("NNUE_DP_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("NNUE_DP_FACTOR_EXCHANGE", "1")
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        tr = _trainer(monkeypatch, "1", momentum=0.9, ema_decay=ec.DECAY)
        twin = _trainer(monkeypatch, "1", momentum=0.9, ema_decay=ec.DECAY)
        assert tr.factor_exchange and not tr.fuse_table_update
        single, group = _logged(monkeypatch, tr)  # two single steps, one eager step, one eager group of three
        losses = [twin.step(slot=s).clone() for s in (0, 1, 0, 0, 1, 2)]
        torch.cuda.synchronize()
        assert torch.equal(tr.loss_ring[:3], torch.stack(losses[3:]))
        for a, b in zip(ec.state_of(tr), ec.state_of(twin)):
            assert torch.equal(a, b)
        assert torch.equal(tr.flat_ema, twin.flat_ema) and not torch.equal(tr.flat_ema, tr.flat_params)
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    local = FRONT + FORWARD + BACKWARD_DP + EXCHANGE
    sgd, table, fused = "nnue_sgd_step_ema", "nnue_ftm_backward_weight_update_ema", "nnue_ftm_backward_weight_update_forward_ema"
    joint = [sgd, "nnue_ftm_conv_binarize", fused, "nnue_classifier_train_step"]
    assert single == local + [sgd, table]
    assert group == local + joint + BACKWARD_DP + EXCHANGE + joint + BACKWARD_DP + EXCHANGE + [sgd, table]


# ---------------------------------------------------------------------------------------------- one rank, the collectives captured
RCCL_ROWS = ("rccl_ar", "rccl_ar_adam", "rccl_shard", "rccl_fx", "rccl_fx_next_forward")


def _rccl_worker(rank: int, port: int, out_dir: str):
    """dp_modes._group_worker's process-group set-up; every row: three single steps held to plain + nnue_ema_update (the third
    replays the step graph with its collective inside), then a step_many group against three more single steps of a twin."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for name in RCCL_ROWS:
            row = dp_modes.BY_NAME[name]
            for k in tm.KNOBS:
                os.environ.pop(k, None)
            os.environ.update(row.env)
            cfg = row.config
            batches = [(i.to("cuda"), l.to("cuda")) for i, l in ec.fresh_batches(3, cfg["batch"], cfg["image"], cfg["classes"])]
            with tm.trainer_for(cfg, ema_decay=ec.DECAY, ema_warmup=True) as (averaged, _), tm.trainer_for(cfg) as (plain, _), \
                    tm.trainer_for(cfg, ema_decay=ec.DECAY, ema_warmup=True) as (twin, _):
                assert averaged.mode == plain.mode, name
                assert (averaged.sharded_update, averaged.factor_exchange) == ("shard" in name, "fx" in name), name
                assert averaged.fuse_next_forward == row.expect.get("fuse_next_forward", False), name
                assert averaged.dp.collectives and averaged.capture_collectives
                table = averaged.ema_table.cpu()
                ec.pair_steps(averaged, plain, [lambda tr, b=b: tr.step(*b) for b in batches], name, omd_of_step=lambda i: float(table[i]))
                assert averaged.capture_collectives and (0, "full_dp") in averaged._g_local, averaged._g_local.keys()
                for b in batches:
                    twin.step(*b)
                ring = averaged.step_many((0, 0, 0)).clone()
                losses = torch.stack([twin.step(slot=0).clone() for _ in range(3)])
                torch.cuda.synchronize()
                assert ((0, 0, 0), "many") in averaged._g_local, f"{name}: the group did not replay as one graph"
                assert torch.equal(ring, losses), (name, ring, losses)
                twin.ema_state()
                averaged.ema_state()
                assert torch.equal(averaged.flat_ema, twin.flat_ema) and torch.equal(averaged.flat_params, twin.flat_params), name
                assert torch.equal(averaged.ema_omd_dev, twin.ema_omd_dev) and int(averaged.ema_pos) == 6 == averaged.ema_position
                assert not torch.equal(averaged.flat_ema, averaged.flat_params)
            (Path(out_dir) / f"{name}.ok").write_text("ok")
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_one_rank_with_captured_collectives(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rccl_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    assert all((tmp_path / f"{name}.ok").exists() for name in RCCL_ROWS)
