"""Every way into the GPU integer engine against outputs RECORDED from the real C++ engine on models whose header values and
integers leave what serialize.py writes (tests/golden/engine_edges.npz, written through oracle/engine_driver.cpp --bits by
tests/golden/make_golden_engine_edges.py): scales that are no power of two and have a fractional part, quantized_one of 255,
20.9, 0 and -200, thresholds a conv byte equals or never passes, fractional conv scales under thresholds inside the byte
range, a table whose int16 sums wrap, int32 biases past 2^24, and a K = 3 file whose stacks differ in weights and in all three
scales.  tests/test_engine_edges_oracle.py proves on the CPU that the record reaches those edges and that the edges reach it.  Every comparison is bit-equal: logits and density as uint32, ids as recorded.  Reads
tests/golden/ only: neither the oracle nor the reference takes part.  ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import engine_edges_record
from nnue_hip import lib
from nnue_hip.engine import EngineModel, stack_of

pytestmark = pytest.mark.gpu

SINGLE = ("odd_scales", "small_scales", "q255", "q20_9", "q0", "qneg200", "thr5", "thr_neg127", "thr_neg200", "thr126_5",
          "conv50_5_thr5", "conv7_9_thr40", "conv2_7_thr5", "wrapping", "big_biases")
K3 = "k3"
F = 128
GIVEN = (0, 1, 2, 3, -1, 7)  # layer stack indices a caller may hand over; outside [0, 3) = stack 0, as the recorded index 3


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    """(model name -> path of its file, model name -> its recorded cases); loaded once, never modified."""
    paths, cases = engine_edges_record.load(tmp_path_factory.mktemp("edges"))
    by_model = {}
    for c in cases:
        c.device_images = torch.from_numpy(c.images).cuda()
        by_model.setdefault(c.model, []).append(c)
    assert set(by_model) == set(SINGLE) | {K3}
    return paths, by_model


@pytest.fixture(scope="module")
def engines(record):
    """(model name, bucket, planes) -> EngineModel, loaded once per module.  planes = 2 on a table that fits one plane packs
    the second plane anyway (the library takes either count for any table)."""
    paths, _ = record
    made = {}

    def get(name, bucket=0, planes=None):
        if (name, bucket, planes) not in made:
            engine = EngineModel.load(paths[name], bucket=bucket)
            if planes is not None:
                assert engine._planes is None and planes >= engine.table_planes
                engine.table_planes = planes
            made[name, bucket, planes] = engine
        return made[name, bucket, planes]

    return get


def plane_counts(engine):
    """The plane counts of the matrix form for this model: those the library accepts and the table fits."""
    ok = [p for p in (1, 2) if lib.load().nnue_engine_matrix_supported(ctypes.byref(engine._c), 1, p) and p >= engine.table_planes]
    assert ok and ok[-1] == 2
    return ok


def bits(t: torch.Tensor) -> np.ndarray:
    a = t.cpu().numpy()
    assert a.dtype == np.float32
    return a.view(np.uint32)


def same(got, want_logits, want_density) -> bool:
    """(logits, density, ...) of a call against recorded bit patterns."""
    return np.array_equal(bits(got[0]), want_logits) and np.array_equal(bits(got[1]), want_density)


def float_cases(cases):
    return [c for c in cases if c.layout is None]


def frames_of(cases):
    """Every recorded frame of a model, the uint8 cases' included: (id arrays, logits [N, stacks, C], density [N])."""
    return [a for c in cases for a in c.ids], np.concatenate([c.logits for c in cases]), np.concatenate([c.density for c in cases])


def maps_of(ids) -> torch.Tensor:
    maps = torch.zeros(len(ids), F, dtype=torch.bool)
    for i, a in enumerate(ids):
        maps[i, torch.from_numpy(a)] = True
    return maps.cuda()


def used_stack(k: int) -> int:
    return k if 0 <= k < 3 else 0


@pytest.mark.parametrize("name", SINGLE)
def test_gather_and_matrix(record, engines, name):
    cases = float_cases(record[1][name])
    assert [(c.h, c.w) for c in cases] == [(32, 32), (32, 20)]
    planes = plane_counts(engines(name))
    assert planes == ([2] if name in ("wrapping", "q255") else [1, 2])  # +-3000, and the table times 6, do not fit a byte
    for c in cases:
        assert same(engines(name).evaluate_logits(c.device_images, c.h, c.w, path="gather"), c.logits[:, 0], c.density), (c, "gather")
        for p in planes:
            engine = engines(name, 0, p)
            assert same(engine.evaluate_logits(c.device_images, c.h, c.w, path="matrix"), c.logits[:, 0], c.density), (c, p)
            assert engine.table_planes == p


@pytest.mark.parametrize("name", SINGLE)
def test_feature_maps_of_the_recorded_ids(record, engines, name):
    ids, logits, density = frames_of(record[1][name])
    maps = maps_of(ids)
    for p in plane_counts(engines(name)):
        assert same(engines(name, 0, p).evaluate_features(maps), logits[:, 0], density), p
    stream = engines(name).stream(len(ids))
    got = stream.step_features(maps)
    assert same(got, logits[:, 0], density) and [int(v) for v in got[2]] == [a.size for a in ids]


@pytest.mark.parametrize("name", SINGLE)
def test_stream_steps_through_the_images_in_both_orders(record, engines, name):
    """One stream per direction through every recorded float image, both sizes; `changed` = the features that differ from the
    stream's previous set, or all active ones on the first step (a refresh)."""
    frames = [(c, i) for c in float_cases(record[1][name]) for i in range(c.count)]
    for order in (frames, frames[::-1]):
        stream, prev = engines(name).stream(1), None
        for c, i in order:
            got = stream.step(c.device_images[i:i + 1], c.h, c.w)
            assert same(got, c.logits[i:i + 1, 0], c.density[i:i + 1]), (c, i)
            assert int(got[2][0]) == (c.ids[i].size if prev is None else np.setxor1d(prev, c.ids[i]).size), (c, i)
            prev = c.ids[i]


@pytest.mark.parametrize("name", SINGLE)
def test_refresh_and_update_between_recorded_sets(record, engines, name):
    """refresh to frame i's recorded set, then add / remove lists to frame j's: frame j's recorded bits.  Two streams walk the
    model's frames in opposite directions, so one call carries two different list pairs."""
    ids, logits, density = frames_of(record[1][name])
    n = len(ids)
    order = [list(range(n)), list(range(n - 1, -1, -1))]
    stream = engines(name).stream(2)
    first = [o[0] for o in order]
    got = stream.refresh([ids[i] for i in first])
    assert same(got, logits[first, 0], density[first]) and [int(v) for v in got[2]] == [ids[i].size for i in first]
    for t in range(1, n):
        i, j = [o[t - 1] for o in order], [o[t] for o in order]
        added = [np.setdiff1d(ids[b], ids[a]) for a, b in zip(i, j)]
        removed = [np.setdiff1d(ids[a], ids[b]) for a, b in zip(i, j)]
        got = stream.update(added, removed)
        assert same(got, logits[j, 0], density[j]), (name, t)
        assert [int(v) for v in got[2]] == [a.size + r.size for a, r in zip(added, removed)], (name, t)


def test_uint8_frames(record, engines):
    """conv_scale = 50.5: the u8 front's table (int32)(x * scale) over 768 (byte, channel) pairs truncates non-trivially;
    conv_scale = 2.7 under threshold 5: its division by (int)scale decides which bytes pass."""
    cases = [c for cs in record[1].values() for c in cs if c.layout]
    assert sorted((c.model, c.layout) for c in cases) == [("conv2_7_thr5", "chw"), ("conv2_7_thr5", "hwc"), ("odd_scales", "chw"),
                                                         ("odd_scales", "hwc")]
    for c in cases:
        store = torch.from_numpy(c.frames).cuda()
        engine = engines(c.model)
        assert same(engine.evaluate_logits_u8(store, layout=c.layout, path="gather"), c.logits[:, 0], c.density), c
        for p in plane_counts(engine):
            got = engines(c.model, 0, p).evaluate_logits_u8(store, layout=c.layout, path="matrix")
            assert same(got, c.logits[:, 0], c.density), (c, p)
        idx = torch.tensor([2, 0, 1, 2], device="cuda")
        pick = idx.cpu().numpy()
        assert same(engine.evaluate_logits_u8(store, idx, layout=c.layout, path="gather"), c.logits[pick, 0], c.density[pick]), c
        stream = engine.stream(c.count)
        got = stream.step_u8(store, layout=c.layout)
        assert same(got, c.logits[:, 0], c.density) and [int(v) for v in got[2]] == [a.size for a in c.ids], c
        back = torch.arange(c.count - 1, -1, -1, device="cuda")
        got = stream.step_u8(store, back, layout=c.layout)
        assert same(got, c.logits[::-1, 0], c.density[::-1]), c
        assert [int(v) for v in got[2]] == [np.setxor1d(a, b).size for a, b in zip(c.ids, c.ids[::-1])], c


def test_k3_every_single_stack_load(record, engines):
    """bucket=k keeps stack k with its own three scales (an index the file lacks keeps stack 0)."""
    cases = record[1][K3]
    ids, logits, density = frames_of(cases)
    for k in range(4):
        assert engines(K3, k).num_stacks == 1
        for c in cases:
            assert c.stacks == [0, 1, 2, 3]
            assert same(engines(K3, k).evaluate_logits(c.device_images, c.h, c.w, path="gather"), c.logits[:, k], c.density), (c, k)
            for p in plane_counts(engines(K3, k)):
                got = engines(K3, k, p).evaluate_logits(c.device_images, c.h, c.w, path="matrix")
                assert same(got, c.logits[:, k], c.density), (c, k, p)
        assert same(engines(K3, k).evaluate_features(maps_of(ids)), logits[:, k], density), k
        stream = engines(K3, k).stream(len(ids))
        assert same(stream.refresh(ids), logits[:, k], density), k


def test_k3_auto_with_given_stacks(record, engines):
    """bucket="auto" with stacks= from the caller: every image meets every index of GIVEN through the gather form, the matrix
    form at both plane counts, the feature maps, a stream over images and one over add / remove lists."""
    assert engines(K3, "auto").num_stacks == 3
    for c in record[1][K3]:
        B = c.count * len(GIVEN)
        pick = [b % c.count for b in range(B)]
        given = [GIVEN[b // c.count] for b in range(B)]
        used = [used_stack(k) for k in given]
        want = np.stack([c.logits[i, k] for i, k in zip(pick, used)])
        x, cur = c.device_images[pick], [c.ids[i] for i in pick]
        for dtype in (torch.int64, torch.int32):
            stacks = torch.tensor(given, dtype=dtype).cuda()
            calls = {"gather": lambda: engines(K3, "auto").evaluate_logits(x, c.h, c.w, stacks=stacks, return_stacks=True, path="gather")}
            for p in (1, 2):
                calls[f"matrix {p}"] = lambda p=p: engines(K3, "auto", p).evaluate_logits(x, c.h, c.w, stacks=stacks,
                                                                                          return_stacks=True, path="matrix")
                calls[f"maps {p}"] = lambda p=p: engines(K3, "auto", p).evaluate_features(maps_of(cur), stacks=stacks,
                                                                                        return_stacks=True)
            for what, call in calls.items():
                got = call()
                assert same(got, want, c.density[pick]) and [int(k) for k in got[2]] == used, (c, what)
            stream, lists = engines(K3, "auto").stream(B), engines(K3, "auto").stream(B)
            assert same(stream.step(x, c.h, c.w, stacks=stacks), want, c.density[pick]), c
            assert [int(k) for k in stream.stacks] == used, c
            other = [c.ids[(i + 1) % c.count] for i in pick]
            lists.refresh(other, stacks=stacks)
            got = lists.update([np.setdiff1d(a, b) for a, b in zip(cur, other)], [np.setdiff1d(b, a) for a, b in zip(cur, other)],
                               stacks=stacks)
            assert same(got, want, c.density[pick]) and [int(k) for k in lists.stacks] == used, c


def test_k3_auto_by_the_rule(record, engines):
    """The free choice lands on the record of the stack `stack_of` names for the RECORDED id count."""
    chosen = []
    for c in record[1][K3]:
        rule = [int(k) for k in stack_of(torch.tensor([a.size for a in c.ids]), 3, F)]
        want = np.stack([c.logits[i, k] for i, k in enumerate(rule)])
        calls = {"gather": lambda: engines(K3, "auto").evaluate_logits(c.device_images, c.h, c.w, return_stacks=True, path="gather")}
        for p in (1, 2):
            calls[f"matrix {p}"] = lambda p=p: engines(K3, "auto", p).evaluate_logits(c.device_images, c.h, c.w,
                                                                                      return_stacks=True, path="matrix")
            calls[f"maps {p}"] = lambda p=p: engines(K3, "auto", p).evaluate_features(maps_of(c.ids), return_stacks=True)
        for what, call in calls.items():
            got = call()
            assert [int(k) for k in got[2]] == rule and same(got, want, c.density), (c, what)
        stream = engines(K3, "auto").stream(c.count)
        assert same(stream.step(c.device_images, c.h, c.w), want, c.density) and [int(k) for k in stream.stacks] == rule, c
        assert same(stream.refresh(c.ids), want, c.density) and [int(k) for k in stream.stacks] == rule, c
        chosen += rule
    assert set(chosen) == {1, 2}  # 56 of the 128 features are on in every frame (cells the conv never writes): stack 0 is not named
