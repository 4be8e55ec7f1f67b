"""The weight clip under data parallelism (include/nnue_hip.h, "weight clip"): two gloo ranks on one GPU, tests/dp_modes.py's
per-rank driver pattern, one run each for the all-reduce update, the sharded update (the clip's ranges translated into the
shard) and the factor exchange (the small update and the table update clamp their own parts).  After two steps every rank's
parameters are bitwise the other rank's, and bitwise the same run with the option off plus ``clamp_`` after each step; the
one-rank forced-collectives form covers a step group under the factor exchange.  ``-m gpu``."""
import gc
import os
import socket
from pathlib import Path

import pytest
import torch

import trainer_modes as tm
import weight_clip_cases as wc
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
        batches = wc.fresh_batches(2, CFG["batch"] * WORLD, CFG["image"], CFG["classes"])
        rows = slice(rank * CFG["batch"], (rank + 1) * CFG["batch"])
        for mode, env in MODES.items():
            for k in tm.KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            with tm.trainer_for(CFG, weight_clip=1.0) as (clipped, _), tm.trainer_for(CFG) as (plain, _):
                assert clipped.mode == plain.mode and clipped.dp.world == WORLD
                assert (clipped.sharded_update, clipped.factor_exchange) == (mode == "sharded", mode == "factor_exchange"), mode
                feed = [lambda tr, b=b: tr.step(b[0][rows].to("cuda"), b[1][rows].to("cuda")) for b in batches]
                # (respread: at 12 rows per rank the second layer's share was 0.098 at step 2)
                wc.pair_steps(clipped, plain, 1.0, feed, f"{mode} rank {rank}", respread=True)
                torch.save(clipped.flat_params.cpu(), Path(out_dir) / f"{mode}_{rank}.pt")
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_two_ranks_clamp_alike_in_every_exchange(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(port, str(tmp_path)), nprocs=WORLD, join=True)  # (a rank's failed assertion raises here)
    for mode in MODES:
        a, b = (torch.load(tmp_path / f"{mode}_{r}.pt", weights_only=True) for r in range(WORLD))
        assert torch.equal(a, b), f"{mode}: the ranks' parameters differ in {int((a != b).sum())} elements"


def test_factor_exchange_group_launches_the_clamped_siblings(monkeypatch, tmp_path):
    """tests/test_gpu_update_sequence.py::test_factor_exchange_update_sequence with the option on: a gloo group of one rank with
    the collectives forced, so that a step_many group runs under the factor exchange; the group is bitwise three single steps."""
    import torch.distributed as dist
    monkeypatch.setenv("NNUE_DP_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("NNUE_DP_FACTOR_EXCHANGE", "1")
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        tr = _trainer(monkeypatch, "1", momentum=0.9, weight_clip=1.0)
        twin = _trainer(monkeypatch, "1", momentum=0.9, weight_clip=1.0)
        assert tr.factor_exchange and not tr.fuse_table_update
        for t in (tr, twin):
            wc.rescale(t.p, 1.0)
            t.max_grad_norm = wc.GRAD_NORM
        single, group = _logged(monkeypatch, tr)  # two single steps, one eager step, one eager group of three
        losses = [twin.step(slot=s).clone() for s in (0, 1, 0, 0, 1, 2)]
        torch.cuda.synchronize()
        assert torch.equal(tr.loss_ring[:3], torch.stack(losses[3:]))
        for a, b in zip(wc.state_of(tr), wc.state_of(twin)):
            assert torch.equal(a, b)
        assert float(tr.p["input.weight"].abs().max()) <= 1.0
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    local = FRONT + FORWARD + BACKWARD_DP + EXCHANGE
    sgd, table, fused = "nnue_sgd_step_clip", "nnue_ftm_backward_weight_update_clip", "nnue_ftm_backward_weight_update_forward_clip"
    joint = [sgd, "nnue_ftm_conv_binarize", fused, "nnue_classifier_train_step"]
    assert single == local + [sgd, table]
    assert group == local + joint + BACKWARD_DP + EXCHANGE + joint + BACKWARD_DP + EXCHANGE + [sgd, table]
