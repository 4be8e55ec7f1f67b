"""The host contract of the classifier block (csrc/classifier_kernels.hip) against what was recorded before its dispatch was
moved into one plan and one launcher per product (tests/golden/classifier_contract.npz, written by
tests/golden/make_golden_classifier_contract.py, which also holds the calls): every refused nnue_classifier_train_step call
-- all 128 phase values at six shapes, both blocks, one and four layer stacks, d_x given and NULL, with no scratch (the early
checks, down to the scratch check's total) and with ample scratch (the late checks) -- returns the recorded code with the
recorded text of nnue_hip_last_error(), and every launch-free query answers as recorded, the bytes of
nnue_classifier_train_rider included.  Nothing here is accepted by the library, so nothing launches.  CPU only; the header's
names of the phase bits are held to lib.CLS_* here as well."""
import json
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from nnue_hip import lib

sys.path.insert(0, str(GOLDEN))
import make_golden_classifier_contract as rec  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.PATH) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def replay():
    return rec.record(lib)


def test_fixture_is_the_recorders_grid_and_stays_small(golden):
    assert np.array_equal(golden["calls"], rec.call_rows(lib.load())) and len(golden["calls"]) > 6144
    assert np.array_equal(golden["queries"], rec.query_rows()) and len(golden["queries"]) == 72
    assert set(golden) == {"messages", "calls", "code", "message", "queries", "rider", *rec.QUERIES}
    assert set(golden["code"].tolist()) == set(rec.REFUSALS)
    messages = json.loads(str(golden["messages"]))
    assert len(set(messages)) == len(messages) and sorted(set(golden["message"].tolist())) == list(range(len(messages)))
    assert rec.PATH.stat().st_size < 64 * 1024


def test_every_refused_call_returns_the_recorded_code_and_text(golden, replay):
    codes, texts, _ = replay
    messages = json.loads(str(golden["messages"]))
    want = [messages[i] for i in golden["message"].tolist()]
    assert len(codes) == len(golden["code"])
    wrong = [i for i in range(len(codes)) if codes[i] != golden["code"][i] or texts[i] != want[i]]
    assert not wrong, (f"{len(wrong)} calls differ; first (section, B, L1, L2, L3, C, pairwise, K, phases, d_x, misaligned) = "
                       f"{golden['calls'][wrong[0]].tolist()}: {codes[wrong[0]]} {texts[wrong[0]]!r} != "
                       f"{golden['code'][wrong[0]]} {want[wrong[0]]!r}")


def test_every_query_answers_as_recorded(golden, replay):
    table = replay[2]
    for q in rec.QUERIES + ("rider",):
        assert table[q].shape == golden[q].shape and table[q].dtype == golden[q].dtype, q
        wrong = np.argwhere(table[q] != golden[q])
        assert len(wrong) == 0, (f"{q}: {len(wrong)} answers differ; first at (B, L1, L2, L3, C, K) = "
                                 f"{golden['queries'][wrong[0][0]].tolist()}: {table[q][tuple(wrong[0])]} != {golden[q][tuple(wrong[0])]}")


def test_header_names_the_phase_bits_as_lib_does():
    header = (ROOT / "include" / "nnue_hip.h").read_text()
    values = {name: int(v) for name, v in re.findall(r"#define NNUE_(CLS_[A-Z0-9_]+) (\d+)\b", header)}
    names = [n for n in dir(lib) if n.startswith("CLS_")]
    assert len(names) == 7 and values == {n: getattr(lib, n) for n in names}
    assert sorted(values.values()) == [1, 2, 4, 8, 16, 32, 64]
