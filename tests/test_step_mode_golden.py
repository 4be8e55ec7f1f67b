"""nnue_hip.step_mode.resolve against tests/golden/trainer_modes_sweep.json: what the policy answered -- through the
restatement tests/trainer_modes.py held before the trainer's own resolver existed -- at every row's configuration and three
big tables, under no knob, the row's own knobs, and each of the two with every single knob setting on top
(tests/golden/make_golden_trainer_modes_sweep.py).  The table of tests/trainer_modes.py names 44 points; this holds the policy
still between them.  No GPU: the resolver is launch-free."""
import json
from pathlib import Path

import pytest

import trainer_modes as tm

SWEEP = json.loads((Path(__file__).parent / "golden" / "trainer_modes_sweep.json").read_text())


def test_the_sweep_covers_every_row_and_every_mode_key():
    assert SWEEP["keys"] == sorted(tm.A_MODES)
    assert SWEEP["configs"][:len(tm.ROWS)] == [row.config for row in tm.ROWS]
    seen = {(i, json.dumps(env, sort_keys=True)) for i, env, _ in SWEEP["records"]}
    assert len(seen) == len(SWEEP["records"]) > 1000
    for i, row in enumerate(tm.ROWS):
        assert (i, json.dumps(row.env, sort_keys=True)) in seen and (i, "{}") in seen, row.name


@pytest.mark.parametrize("index", range(len(SWEEP["configs"])))
def test_the_resolver_answers_as_recorded(index, monkeypatch):
    cfg, wrong = SWEEP["configs"][index], []
    for i, env, values in SWEEP["records"]:
        if i != index:
            continue
        tm.set_knobs(monkeypatch, tm.Row("sweep", env=env))
        got = tm.resolve(cfg)
        wrong += [f"{env}: {d}" for d in tm.differences(got, dict(zip(SWEEP["keys"], values)))]
        assert set(got) == set(SWEEP["keys"]) and got["phases"] in tm.PHASES
    assert not wrong, f"configuration {cfg}: " + "; ".join(wrong[:8])
