"""oracle/nnue_engine_oracle.py (numpy restatement of the C++ engine's evaluate_logits) against outputs of the REAL
engine: tests/golden/engine_cases.npz was produced by oracle/_ref/nnue_inference, the reference's own sources
compiled here (recipe: tests/golden/make_golden_engine.py).  tests/golden/engine_shapes.npz holds what the same engine
gave, through oracle/engine_driver.cpp, at frames with W != H, on models with more than 64 channels per cell and at layer
stack indices 0..K of a K = 4 file, with its active feature ids (recipe: tests/golden/make_golden_engine_shapes.py).
CPU only."""
import json

import numpy as np
import pytest

import nnue_engine_oracle as eo
from conftest import GOLDEN


def cases():
    z = np.load(GOLDEN / "engine_cases.npz")
    return z, json.loads(str(z["index"]))


def test_oracle_reproduces_the_reference_engine_exactly():
    z, index = cases()
    assert sum(c["count"] for c in index) == 32
    for k, c in enumerate(index):
        m = eo.load_nnue(GOLDEN / c["model"])
        for i in range(c["count"]):
            logits, density = eo.evaluate_logits(m, z[f"case{k}/images"][i], c["h"], c["w"])
            # the engine prints with 10 decimals; its logits are multiples of 1/64, exactly representable
            assert np.array_equal(logits.astype(np.float64), z[f"case{k}/logits"][i]), (c, i)
            assert abs(float(density) - float(z[f"case{k}/density"][i])) < 5e-10, (c, i)


def shape_cases():
    """(index entry, images, logits [n, stacks, C], density [n], id arrays per image) of every engine_shapes.npz case."""
    z = np.load(GOLDEN / "engine_shapes.npz")
    for k, c in enumerate(json.loads(str(z["index"]))):
        off = z[f"case{k}/ids_offsets"]
        ids = [z[f"case{k}/ids"][off[i]:off[i + 1]] for i in range(c["count"])]
        yield c, z[f"case{k}/images"], z[f"case{k}/logits"], z[f"case{k}/density"], ids


def map_size(m, h, w):
    s = eo.conv_stride(h, m["grid"])
    return (h - 1) // s + 1, (w - 1) // s + 1


def test_oracle_reproduces_the_recorded_shapes_channels_and_stacks():
    """Logits equal, density within the ten-decimal print, ids equal -- at every recorded layer stack index.  Each of these
    edits of the oracle was seen to fail this test: row length g in place of OW in active_features (the produced map laid
    out row by row of the grid); the 64-channel mask dropped; `bucket` ignored."""
    models, seen = {}, set()
    for c, images, logits, density, ids in shape_cases():
        m = models.setdefault(c["model"], eo.load_nnue(GOLDEN / c["model"]))
        oh, ow = map_size(m, c["h"], c["w"])
        assert oh * ow * m["oc"] <= m["num_features"], c  # nothing recorded overruns the engine's buffer
        assert logits.shape == (c["count"], len(c["stacks"]), m["stacks"][0]["classes"]), c
        seen.add((c["model"], oh, ow))
        for i in range(c["count"]):
            conv, _ = eo.conv_forward(m, images[i], c["h"], c["w"])
            assert conv.shape == (oh, ow, m["oc"])
            assert np.array_equal(eo.active_features(m, conv), ids[i]), (c, i)
            for j, k in enumerate(c["stacks"]):
                got, dens = eo.evaluate_logits(m, images[i], c["h"], c["w"], bucket=k)
                assert np.array_equal(got.astype(np.float64), logits[i, j]), (c, i, k)
                assert abs(float(dens) - float(density[i])) < 5e-10, (c, i, k)
    # what the record is there for: maps narrower and wider than the grid, one column, the whole 4x4 grid at 96 and 70 channels
    assert {("nnue_c1arch.nnue", 8, 5), ("nnue_c1arch.nnue", 8, 10), ("nnue_c1arch.nnue", 8, 12), ("nnue_c1arch.nnue", 8, 1),
            ("nnue_c1arch.nnue", 10, 7), ("nnue_c1arch.nnue", 10, 8), ("nnue_c1arch.nnue", 9, 5), ("nnue_c1arch.nnue", 10, 6),
            ("nnue_c1arch.nnue", 10, 4), ("nnue_c1arch.nnue", 9, 10), ("nnue_tiny4x4.nnue", 3, 2), ("nnue_tiny4x4.nnue", 3, 4),
            ("nnue_wide96.nnue", 4, 4), ("nnue_wide96.nnue", 4, 3), ("nnue_wide96.nnue", 4, 2), ("nnue_wide96.nnue", 3, 5),
            ("nnue_wide96.nnue", 4, 1), ("nnue_wide70.nnue", 4, 4), ("nnue_wide70.nnue", 3, 2), ("nnue_k4.nnue", 6, 6),
            ("nnue_k4.nnue", 6, 4), ("nnue_k4.nnue", 6, 8)} == seen


def test_the_record_separates_the_readings_it_is_there_for():
    """The fixture's own data, without the oracle: the properties that make a shared misreading visible."""
    by_model = {}
    for c, images, logits, density, ids in shape_cases():
        by_model.setdefault(c["model"], []).append((c, logits, ids))
    for name, oc in (("nnue_wide96.nnue", 96), ("nnue_wide70.nnue", 70)):
        m = eo.load_nnue(GOLDEN / name)
        assert m["oc"] == oc and m["threshold"] < 0
        for c, _, ids in by_model[name]:
            oh, ow = map_size(m, c["h"], c["w"])
            for a in ids:
                assert int((a % oc).max()) == 63  # channels 64.. never turn on, in produced cells or in empty ones
                # every cell the conv did not produce is on in its 64 low channels (0 > threshold)
                empty = np.arange(oh * ow * oc, m["num_features"])
                assert np.array_equal(a[a >= oh * ow * oc], empty[empty % oc < 64]), c
    k4 = eo.load_nnue(GOLDEN / "nnue_k4.nnue")
    assert k4["buckets"] == 4
    counts = []
    for c, logits, ids in by_model["nnue_k4.nnue"]:
        assert c["stacks"] == [0, 1, 2, 3, 4]
        for i in range(c["count"]):
            assert np.array_equal(logits[i, 4], logits[i, 0])  # an index the file lacks is stack 0
            assert len({logits[i, j].tobytes() for j in range(4)}) == 4  # the four stacks are four networks
            counts.append(ids[i].size)
    # the stacks the training rule names for the recorded counts (min(K-1, n*K // (F+1))): the free choice meets several
    assert {min(3, n * 4 // 257) for n in counts} == {0, 1, 2, 3}, counts
    # consecutive frames of a chain through each model differ, so a stream's `changed` is not trivially zero
    for name, cases in by_model.items():
        sets = [a for _, _, ids in cases for a in ids]
        assert all(np.setxor1d(a, b).size > 0 for a, b in zip(sets, sets[1:])), name


def test_engine_stride_rule_differs_from_training():
    assert eo.conv_stride(32, 10) == 4 and (32 - 1) // (10 - 1) == 3  # ceil vs floor: 8x8 map inside a 10x10 grid
    assert eo.conv_stride(28, 10) == 3 and eo.conv_stride(96, 10) == 11 and eo.conv_stride(7, 1) == 7


def test_loader_rejections(tmp_path):
    good = (GOLDEN / "nnue_tiny4x4.nnue").read_bytes()
    for name, data, msg in (("magic", b"XNUE" + good[4:], "magic"), ("version", good[:4] + b"\x03\x00\x00\x00" + good[8:], "version"),
                            ("tail", good + b"\x00", "trailing")):
        p = tmp_path / f"{name}.nnue"
        p.write_bytes(data)
        with pytest.raises(ValueError, match=msg):
            eo.load_nnue(p)
    m = eo.load_nnue(GOLDEN / "nnue_c1arch.nnue")
    assert (m["num_features"], m["l1"], m["l2"], m["l3"], m["grid"], m["oc"], m["stacks"][0]["classes"]) == (800, 64, 32, 8, 10, 8, 10)
