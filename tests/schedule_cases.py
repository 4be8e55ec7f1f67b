"""Shared builders of tests/test_gpu_lr_schedule.py, tests/test_gpu_resume.py and tests/test_gpu_dp_resume.py: the small shape
and the big-table pair (restated from tests/test_gpu_adam_table_update.py::_bigtable_pair), their fixed input slots, and the
twelve distinct float32 rates of the per-step schedule.  No test lives here."""
import os

import pytest
import torch

import nnue

DEV = "cuda"

# twelve distinct float32 rates, none a round number in binary, neither sorted nor periodic
RATES = torch.tensor([0.0125, 0.011, 0.0173, 0.0091, 0.0147, 0.0033, 0.0207, 0.0061, 0.0119, 0.0079, 0.0163, 0.0047], dtype=torch.float32)
assert len(set(RATES.tolist())) == 12

SMALL_SGD = dict(lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0)


def small_model(seed: int = 0):
    torch.manual_seed(seed)
    return nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(DEV)


def small_data(slots: int = 3, batch: int = 16, seed: int = 5):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (batch,), generator=gen).to(DEV))
            for _ in range(slots)]


def fill(trainer, data):
    for (im, lb), (ti, tl) in zip(data, trainer.inputs):
        ti.copy_(im)
        tl.copy_(lb)
    return trainer


def small_trainer(model, use_graph: bool = True, data=None, **over):
    from nnue_hip.trainer import NnueTrainer
    opt = dict(SMALL_SGD, input_slots=3, use_graph=use_graph)
    opt.update(over)
    return fill(NnueTrainer(model, 16, (32, 32), **opt), small_data() if data is None else data)


BIG_HW, BIG_L1 = 64, 256


def big_model(seed: int = 0):
    torch.manual_seed(seed)
    return nnue.NNUE(nnue.GridFeatureSet(16, 32), BIG_L1, 32, 16, num_classes=10, input_size=BIG_HW).to(DEV)


def big_data(seed: int = 5):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(64, 3, BIG_HW, BIG_HW, generator=gen).to(DEV), torch.randint(0, 10, (64,), generator=gen).to(DEV)) for _ in range(3)]


def big_trainer(monkeypatch, model, fuse_next: bool, data=None, **opt):
    """GridFeatureSet(16, 32), 256/32/16, 64x64, batch 64 with the table's update in the product's epilogue; fuse_next: groups
    also form the next step's forward in that pass (the trainer under test), else not (the twin)."""
    from nnue_hip.trainer import NnueTrainer
    monkeypatch.setenv("NNUE_FUSE_TABLE_UPDATE", "1")  # (auto: tables of 32 MB or more; this one has 8 MB)
    monkeypatch.setenv("NNUE_FUSE_NEXT_FORWARD", "1" if fuse_next else "0")
    tr = NnueTrainer(model, 64, (BIG_HW, BIG_HW), input_slots=3, use_graph=True, **opt)
    if fuse_next and not tr.fuse_next_forward and os.environ.get("NNUE_FTM_BF16") == "0":
        pytest.skip("a developer knob took the forward off the bf16-split 64-deep tiles the fused pass is built on")
    assert tr.fuse_table_update and tr.fuse_next_forward == fuse_next and not tr.grads_materialised
    return fill(tr, big_data() if data is None else data)


def big_pair(monkeypatch, **opt):
    model, twin = big_model(), big_model()
    twin.load_state_dict(model.state_dict())
    return big_trainer(monkeypatch, model, True, **opt), big_trainer(monkeypatch, twin, False, **opt)


BIG_OPTS = {"adam": dict(lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, optimizer="adam"),
            "sgd": dict(lr=0.01, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0)}


def optimizer_state(tr):
    """Every buffer the optimizer carries, cloned."""
    return [t.clone() for t in tr._optimizer_buffers()]


def same_state(a, b) -> bool:
    return torch.equal(a.flat_params, b.flat_params) and all(torch.equal(x, y) for x, y in zip(a._optimizer_buffers(), b._optimizer_buffers()))
