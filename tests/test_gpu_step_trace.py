"""The run form of every public call of the trainer -- which graph is replayed, which plan runs eagerly, where the collective
goes, what the graph cache and the counters hold afterwards -- held to tests/golden/step_trace.json, recorded at the commit
before ``step`` and ``step_many`` got one driver (tests/step_trace.py has the recorder and the scripted calls,
tests/golden/make_golden_step_trace.py wrote the fixture).  The launches' results are held bitwise elsewhere; this file holds
which launches, replays and collectives there are and in which order.  ``-m gpu``.
"""
import json
from pathlib import Path

import pytest

import step_trace

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "step_trace.json").read_text())


def test_the_fixture_has_the_scripted_scenarios():
    assert sorted(GOLDEN) == sorted(step_trace.SCENARIOS)


@pytest.mark.parametrize("name", sorted(step_trace.SCENARIOS))
def test_run_forms_follow_the_recorded_trace(name, tmp_path):
    why = step_trace.off_form(name)
    if why:
        pytest.skip(why)
    got, want = step_trace.run_scenario(name, tmp_path), GOLDEN[name]
    assert [(r["trainer"], r["call"]) for r in got] == [(r["trainer"], r["call"]) for r in want]
    for g, w in zip(got, want):
        where = f"{name}, trainer {g['trainer']}, {g['call']}"
        assert g["events"].split() == w["events"].split(), where
        assert g["state"] == w["state"], where
