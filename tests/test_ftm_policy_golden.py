"""The launch policy of csrc/ftm_kernels.hip against the table recorded before it was moved into one resolver
(tests/golden/ftm_policy.npz, written by tests/golden/make_golden_ftm_policy.py, which also holds the grid): every launch-free
shape query -- supported, scratch sizes, fused and planes-fed forward, rider, squared-norm count, STE ride, value planes, fused
update + forward, Gram scratch, nnue_ftm_uses_bf16(0..5) -- over 2028 shapes under six per-call knob settings.  CPU only."""
import json
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from nnue_hip import lib

sys.path.insert(0, str(GOLDEN))
import make_golden_ftm_policy as rec  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.PATH) as z:
        return {k: z[k] for k in z.files}


def test_fixture_is_the_recorders_grid_and_stays_small(golden):
    assert np.array_equal(golden["rows"], rec.rows()) and len(golden["rows"]) == 2028
    assert json.loads(str(golden["knobs"])) == list(rec.KNOBS) and len(rec.KNOBS) == 6
    assert set(golden) == {"rows", "knobs", *rec.QUERIES}
    assert rec.PATH.stat().st_size < 200 * 1024


def test_default_knobs_reach_every_branch(golden):
    counts = rec.branch_counts(golden)
    assert len(counts) == 7 and all(n > 0 for n in counts.values()), counts


def test_every_query_answers_as_recorded(golden):
    got = rec.record(lib.load())
    for q in rec.QUERIES:
        assert got[q].shape == golden[q].shape, q
        wrong = np.argwhere(got[q] != golden[q])
        assert len(wrong) == 0, (f"{q}: {len(wrong)} answers differ; first under {rec.KNOBS[wrong[0][0]]} at "
                                 f"(B, F, P, L1, H, W, stride) = {golden['rows'][wrong[0][1]].tolist()}: "
                                 f"{got[q][tuple(wrong[0])]} != {golden[q][tuple(wrong[0])]}")
