"""nnue_hip.lr_schedule on the host: LrSchedule.lr is the reference's get_lr (training_utils.py:283-336) to the bit, on the
doubles tests/golden/make_golden_lr_schedule.py recorded from the reference itself; values() is their float32 rounding;
from_config stays off for every config that does not opt in.  CPU only."""
import json
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN
from nnue_hip.lr_schedule import LrSchedule

RECORD = json.loads((GOLDEN / "lr_schedule_cases.json").read_text())
CASES = {k: v for k, v in RECORD.items() if not k.startswith("_")}


def test_the_record_covers_the_cases_and_edges():
    assert len(CASES) >= 6
    for name, case in CASES.items():
        its = case["iterations"]
        assert set(range(8)) | {50, 99, 100, 101} <= set(its), name
        assert [float.fromhex(h) for h in case["hex"]] == [float(r) for r in case["repr"]], name
    assert CASES["long_29400"]["config"]["lr_decay_iters"] == 29400 and {29398, 29399, 29400} <= set(CASES["long_29400"]["iterations"])
    plain = dict(zip(CASES["plain_cosine_100"]["iterations"], (float.fromhex(h) for h in CASES["plain_cosine_100"]["hex"])))
    assert plain[0] == 0.01 and abs(plain[50] - 0.005) < 1e-15 and abs(plain[99] - 2.467e-06) < 1e-9 and plain[100] == 0.0 == plain[101]
    flat = dict(zip(CASES["no_decay"]["iterations"], (float.fromhex(h) for h in CASES["no_decay"]["hex"])))
    assert all(flat[it] == 0.01 for it in flat if it <= 100) and flat[101] == 0.0  # the reference's quirk, kept
    clamp = CASES["cyclical_period_8_clamped"]
    assert clamp["config"]["min_lr"] in (float.fromhex(h) for h in clamp["hex"])  # the final clamp is hit
    assert RECORD["_reference_at_warmup_eq_decay_iters"] == "ZeroDivisionError"


@pytest.mark.parametrize("name", sorted(CASES))
def test_lr_equals_the_reference_doubles(name):
    case = CASES[name]
    sched = LrSchedule(**case["config"])
    for it, h in zip(case["iterations"], case["hex"]):
        got = sched.lr(it)
        assert isinstance(got, float) and got == float.fromhex(h), (name, it, got.hex(), h)


@pytest.mark.parametrize("name", sorted(CASES))
def test_values_are_the_float32_rounding(name):
    case = CASES[name]
    sched = LrSchedule(**case["config"])
    n = max(case["iterations"]) + 1
    values = sched.values(n)
    assert values.dtype == torch.float32 and tuple(values.shape) == (n,)
    for it, h in zip(case["iterations"], case["hex"]):
        assert values[it].item() == torch.tensor(float.fromhex(h), dtype=torch.float64).to(torch.float32).item(), (name, it)
    with pytest.raises(ValueError):
        sched.values(0)


def test_the_reference_division_by_zero_is_refused_at_construction():
    with pytest.raises(ValueError, match="lr_decay_iters"):
        LrSchedule(learning_rate=0.01, warmup_iters=5, lr_decay_iters=5)
    with pytest.raises(ValueError, match="lr_decay_iters"):
        LrSchedule(learning_rate=0.01, warmup_iters=6, lr_decay_iters=5)
    LrSchedule(learning_rate=0.01, warmup_iters=5, lr_decay_iters=5, decay_lr=False)  # nothing divides there


def test_from_config_is_off_unless_the_config_opts_in():
    base = dict(learning_rate=0.02, max_epochs=3)
    assert LrSchedule.from_config(SimpleNamespace(**base), 7) is None
    # the reference's own keys do not switch it on (config/train_nnue.py:39-46 sets them and nothing reads them)
    ref_like = SimpleNamespace(**base, use_cosine_scheduler=True, decay_lr=True, use_cyclical_lr=True, warmup_iters=10, min_lr=1e-5)
    assert LrSchedule.from_config(ref_like, 7) is None
    assert LrSchedule.from_config(SimpleNamespace(**base, lr_schedule=False), 7) is None
    got = LrSchedule.from_config(SimpleNamespace(**base, lr_schedule=True, use_cosine_scheduler=True), 7)
    assert got == LrSchedule(learning_rate=0.02, min_lr=0.0, warmup_iters=0, lr_decay_iters=21, decay_lr=True)
    got = LrSchedule.from_config(SimpleNamespace(**base, lr_schedule=True), 7)
    assert got.decay_lr is False and got.lr_decay_iters == 21 and got.lr(21) == 0.02 and got.lr(22) == 0.0
    full = SimpleNamespace(**base, lr_schedule=True, warmup_iters=2, lr_decay_iters=50, min_lr=1e-4, decay_lr=True,
                           use_cosine_scheduler=False, use_cyclical_lr=True, cyclical_lr_period=8, cyclical_lr_amplitude=0.25)
    assert LrSchedule.from_config(full, 7) == LrSchedule(0.02, 1e-4, 2, 50, True, True, 8, 0.25)
