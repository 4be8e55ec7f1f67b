"""The launch sequence of the trainer's update path (nnue_hip/trainer.py: _small_update, _table_update, _update,
_exchange_and_update, _run_many): the ordered C entry points of one eager ``step`` and one eager ``step_many`` at the smallest
shape with the fused table update (tests/test_gpu_adam_table_update.py::_bigtable_pair), held to lists logged once at the
commit before the update path was consolidated.  The results of these launches are held bitwise elsewhere
(tests/test_gpu_update_forward.py, test_gpu_adam_table_update.py, test_gpu_trainer.py, test_gpu_dp.py); this file holds
which launches there are and in which order, whichever way the trainer routes them (a recorded plan through
``lib.run_plan`` or a wrapper through ``lib._call``).  ``-m gpu``.
"""
import os

import pytest
import torch

import nnue

pytestmark = pytest.mark.gpu
DEV = "cuda"

OPTIMIZERS = {"sgd_momentum": dict(momentum=0.9), "sgd_plain": dict(momentum=0.0), "adam": dict(optimizer="adam")}

# ---- the local segments of a step at this shape (K = 1, no layer-1 fusion, the table's gradient never materialised)
FRONT = ["nnue_ftm_conv_binarize"]
FORWARD = ["nnue_ftm_forward", "nnue_classifier_train_step"]
BACKWARD = ["nnue_ftm_gram_sqnorm_tail", "nnue_classifier_train_step", "nnue_ftm_backward_values_ws", "nnue_ste_conv_backward"]
BACKWARD_DP = ["nnue_ftm_backward_tail_rows", "nnue_classifier_train_step", "nnue_ftm_backward_values_ws", "nnue_ste_conv_backward"]
EXCHANGE = ["nnue_dp_factor_pack", "nnue_dp_factor_unpack", "nnue_ftm_gram_sqnorm"]


def _step(small, table):
    return FRONT + FORWARD + BACKWARD + [small, table]


def _group(small, table, fused):
    """Three steps; fused: the first two updates also form the next map and its forward."""
    if not fused:
        return _step(small, table) * 3
    joint = [small, "nnue_ftm_conv_binarize", fused, "nnue_classifier_train_step"]
    return FRONT + FORWARD + BACKWARD + joint + BACKWARD + joint + BACKWARD + [small, table]


SGD = ("nnue_sgd_step", "nnue_ftm_backward_weight_update")
ADAM = ("nnue_adam_step_ext", "nnue_ftm_backward_weight_update_adam")
EXPECTED = {
    # (optimizer, NNUE_FUSE_NEXT_FORWARD): (step(slot=0), step_many((0, 1, 2)))
    ("sgd_momentum", "1"): (_step(*SGD), _group(*SGD, "nnue_ftm_backward_weight_update_forward")),
    ("sgd_momentum", "0"): (_step(*SGD), _group(*SGD, None)),
    ("sgd_plain", "1"): (_step(*SGD), _group(*SGD, "nnue_ftm_backward_weight_update_forward")),
    ("sgd_plain", "0"): (_step(*SGD), _group(*SGD, None)),
    ("adam", "1"): (_step(*ADAM), _group(*ADAM, "nnue_ftm_backward_weight_update_forward_adam")),
    ("adam", "0"): (_step(*ADAM), _group(*ADAM, None)),
}


def _trainer(monkeypatch, fuse_next, **opt):
    from nnue_hip.trainer import NnueTrainer
    if os.environ.get("NNUE_FT_PATH", "auto") not in ("auto", "mfma"):
        pytest.skip("another FeatureTransformer kernel family is forced (NNUE_FT_PATH)")
    monkeypatch.setenv("NNUE_FUSE_TABLE_UPDATE", "1")  # (auto: tables of 32 MB or more; this one has 8 MB)
    monkeypatch.setenv("NNUE_FUSE_NEXT_FORWARD", fuse_next)
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(16, 32), 256, 32, 16, num_classes=10, input_size=64).to(DEV)
    tr = NnueTrainer(model, 64, (64, 64), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, input_slots=3, use_graph=True, **opt)
    if fuse_next == "1" and not tr.fuse_next_forward and os.environ.get("NNUE_FTM_BF16") == "0":
        pytest.skip("a developer knob took the forward off the bf16-split 64-deep tiles the fused pass is built on")
    assert tr.fuse_next_forward == (fuse_next == "1") and not tr.grads_materialised
    gen = torch.Generator().manual_seed(5)
    for images, labels in tr.inputs:
        images.copy_(torch.randn(64, 3, 64, 64, generator=gen))
        labels.copy_(torch.randint(0, 10, (64,), generator=gen))
    return tr


def _logged(monkeypatch, tr):
    """(entry points of one eager step, of one eager group of three) after two single steps have recorded the plans."""
    from nnue_hip import lib
    tr.step(slot=0)
    tr.step(slot=1)
    assert tr.steps_done == 2 and tr._plan_local is not None
    log, call, run_plan = [], lib._call, lib.run_plan

    def log_call(name, *args):
        log.append(name)
        call(name, *args)

    def log_plan(plan, stream_ptr, timers=None):
        log.extend(c[0] for c in plan)
        run_plan(plan, stream_ptr, timers)

    monkeypatch.setattr(lib, "_call", log_call)
    monkeypatch.setattr(lib, "run_plan", log_plan)
    tr.step(slot=0, timers={})  # an empty timer dict: the eager form, no events
    single = list(log)
    del log[:]
    tr.step_many((0, 1, 2), timers={})
    torch.cuda.synchronize()
    assert tr.steps_done == 6
    print(f"step: {single}\nstep_many: {log}")
    return single, list(log)


@pytest.mark.parametrize("fuse_next", ("1", "0"))
@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
def test_single_rank_update_sequence(monkeypatch, optimizer, fuse_next):
    tr = _trainer(monkeypatch, fuse_next, **OPTIMIZERS[optimizer])
    assert tr.fuse_table_update
    single, group = _logged(monkeypatch, tr)
    want_single, want_group = EXPECTED[(optimizer, fuse_next)]
    assert single == want_single
    assert group == want_group


def test_factor_exchange_update_sequence(monkeypatch, tmp_path):
    """The factor-exchange branch with one rank: a gloo group of world size 1 with the collectives forced on (the all-gather
    of one chunk is the identity; the launches around it are the ones every rank of a larger world issues)."""
    import torch.distributed as dist
    monkeypatch.setenv("NNUE_DP_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("NNUE_DP_FACTOR_EXCHANGE", "1")
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        tr = _trainer(monkeypatch, "1", momentum=0.9)
        assert tr.factor_exchange and not tr.fuse_table_update and not tr.capture_collectives
        single, group = _logged(monkeypatch, tr)
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    local = FRONT + FORWARD + BACKWARD_DP + EXCHANGE
    joint = ["nnue_sgd_step", "nnue_ftm_conv_binarize", "nnue_ftm_backward_weight_update_forward", "nnue_classifier_train_step"]
    assert single == local + list(SGD)
    assert group == local + joint + BACKWARD_DP + EXCHANGE + joint + BACKWARD_DP + EXCHANGE + list(SGD)
