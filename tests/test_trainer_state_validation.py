"""NnueTrainer.load_state_dict's validation on a stub with no GPU: it refuses before anything is copied (the stub has no
buffers to copy into, so a refusal that came too late would fail differently).  CPU only."""
import copy

import pytest
import torch

from nnue_hip.trainer import FlatLayout, NnueTrainer


def _stub(optimizer="sgd", momentum=True):
    model = torch.nn.Sequential(torch.nn.Linear(3, 2))
    tr = NnueTrainer.__new__(NnueTrainer)
    tr.model, tr.optimizer = model, optimizer
    tr.layout = FlatLayout.of(model)
    tr.flat_momentum = object() if (momentum and optimizer == "sgd") else None
    return tr


def _state(optimizer="sgd", momentum=True, steps=4):
    entries = {}
    for i, shape in enumerate(((2, 3), (2,))):
        entries[i] = ({"step": torch.tensor(float(steps)), "exp_avg": torch.zeros(shape), "exp_avg_sq": torch.zeros(shape)}
                      if optimizer == "adam" else ({"momentum_buffer": torch.ones(shape)} if momentum else {}))
    return {"version": 1, "optimizer_type": optimizer, "optimizer": {"state": entries, "param_groups": []}, "steps_done": steps,
            "lr": 0.01, "lr_schedule": None}


def test_a_matching_state_passes_the_checks():
    for optimizer, momentum in (("sgd", True), ("sgd", False), ("adam", False)):
        got = _stub(optimizer, momentum)._checked_optimizer_state(_state(optimizer, momentum)["optimizer"], 4)
        want = {"adam": {"exp_avg", "exp_avg_sq"}, "sgd": {"momentum_buffer"} if momentum else set()}[optimizer]
        assert set(got) == want and all(set(v) == {"0.weight", "0.bias"} for v in got.values())
    assert _stub()._checked_optimizer_state({"state": {}, "param_groups": []}, 0) == {"momentum_buffer": {}}  # a state from before step 1


@pytest.mark.parametrize("what", ("type", "version", "shape", "momentum missing", "momentum unexpected", "entry missing", "foreign",
                                  "negative steps", "schedule position", "schedule shape", "not a dict"))
def test_mismatches_raise_value_error_before_any_copy(what):
    tr, sd = _stub(), _state()
    if what == "type":
        sd["optimizer_type"] = "adam"
    elif what == "version":
        sd["version"] = 2
    elif what == "shape":
        sd["optimizer"]["state"][1]["momentum_buffer"] = torch.ones(3)
    elif what == "momentum missing":
        sd = _state(momentum=False)
    elif what == "momentum unexpected":
        tr = _stub(momentum=False)
    elif what == "entry missing":
        del sd["optimizer"]["state"][0]
    elif what == "foreign":
        sd = dict(_state("adam"), optimizer_type="sgd")
    elif what == "negative steps":
        sd["steps_done"] = -1
    elif what == "schedule position":
        sd["lr_schedule"] = {"values": torch.ones(4), "position": -1}
    elif what == "schedule shape":
        sd["lr_schedule"] = {"values": torch.ones(2, 2), "position": 0}
    elif what == "not a dict":
        sd = [copy.deepcopy(sd)]
    with pytest.raises(ValueError):
        tr.load_state_dict(sd)
