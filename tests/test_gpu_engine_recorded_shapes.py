"""Every way into the GPU integer engine against outputs RECORDED from the real C++ engine (tests/golden/engine_shapes.npz,
written through oracle/engine_driver.cpp by tests/golden/make_golden_engine_shapes.py) where engine_cases.npz has none: frames
with W != H -- the engine takes its stride from H alone, writes a dense [OH][OW][oc] map and reads it back flat against the
g x g grid, so cells shift by OW and a map may be wider than the grid -- models with 96 and 70 channels per cell (channels
>= 64 never turn on), and layer stack indices 0..4 of a K = 4 file (4 = stack 0).  Logits bit-equal to the recorded values,
density within the record's ten printed decimals (5e-10), `changed` from the recorded id sets.  Reads tests/golden/ only:
neither the oracle nor the reference takes part.  ``-m gpu``."""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from nnue_hip.engine import EngineModel, stack_of

pytestmark = pytest.mark.gpu

K4 = "nnue_k4.nnue"
FORCED = (0, 1, 2, 3, 4, 7, -1)  # layer stack indices a caller may hand over; outside [0, 4) = stack 0


class Case:
    def __init__(self, z, k, c):
        self.model, self.h, self.w, self.count, self.stacks = c["model"], c["h"], c["w"], c["count"], c["stacks"]
        self.images = torch.from_numpy(z[f"case{k}/images"]).cuda()
        self.logits = z[f"case{k}/logits"]  # float64 [count, len(stacks), C]
        self.density = z[f"case{k}/density"]
        off = z[f"case{k}/ids_offsets"]
        self.ids = [z[f"case{k}/ids"][off[i]:off[i + 1]].astype(np.int64) for i in range(self.count)]

    def __repr__(self):
        return f"{self.model} {self.h}x{self.w}"


@pytest.fixture(scope="module")
def record():
    """model name -> its recorded cases in the fixture's order; loaded once, never modified."""
    z = np.load(GOLDEN / "engine_shapes.npz")
    by_model = {}
    for k, c in enumerate(json.loads(str(z["index"]))):
        by_model.setdefault(c["model"], []).append(Case(z, k, c))
    assert set(by_model) == {"nnue_c1arch.nnue", "nnue_tiny4x4.nnue", "nnue_wide96.nnue", "nnue_wide70.nnue", K4}
    assert sum(c.count for cases in by_model.values() for c in cases) == 45
    return by_model


@pytest.fixture(scope="module")
def engines():
    """(model name, bucket) -> EngineModel, loaded once per module."""
    made = {}

    def get(name, bucket=0):
        if (name, bucket) not in made:
            made[name, bucket] = EngineModel.load(GOLDEN / name, bucket=bucket)
        return made[name, bucket]

    return get


def same_logits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().astype(np.float64), want)


def same_density(got: torch.Tensor, want) -> bool:
    return float(np.abs(got.cpu().numpy().astype(np.float64) - np.asarray(want, dtype=np.float64)).max()) < 5e-10


def used_stack(k: int) -> int:
    return k if 0 <= k < 4 else 0


def test_batched_gather_and_matrix(record, engines):
    ran_matrix = set()
    for name, cases in record.items():
        engine = engines(name)
        for c in cases:
            for path in ("gather", "matrix"):
                if path == "matrix" and not engine.matrix_supported(c.count):
                    continue
                logits, density = engine.evaluate_logits(c.images, c.h, c.w, path=path)
                assert same_logits(logits, c.logits[:, 0]), (c, path)
                assert same_density(density, c.density), (c, path)
                if path == "matrix":
                    ran_matrix.add((name, c.h, c.w))
    # the matrix form is left out only where the library refuses the model: it took part where the record matters most
    assert any(n == "nnue_c1arch.nnue" and h != w for n, h, w in ran_matrix)
    assert {("nnue_c1arch.nnue", 32, 45), ("nnue_wide96.nnue", 27, 40), ("nnue_wide96.nnue", 40, 40), (K4, 17, 22)} <= ran_matrix
    assert ran_matrix == {(n, c.h, c.w) for n, cases in record.items() for c in cases}  # no fixture model is refused


def test_four_dimensional_frames_are_the_same_buffers(record, engines):
    """[B,3,H,W] tensors are taken by their memory with H = shape[2], W = shape[3]: the recorded flat buffers, viewed so."""
    for name in ("nnue_c1arch.nnue", "nnue_wide96.nnue"):
        for c in record[name]:
            logits, density = engines(name).evaluate_logits(c.images.view(c.count, 3, c.h, c.w), path="gather")
            assert same_logits(logits, c.logits[:, 0]) and same_density(density, c.density), c


@pytest.mark.parametrize("name", ["nnue_c1arch.nnue", "nnue_tiny4x4.nnue", "nnue_wide96.nnue", "nnue_wide70.nnue", K4])
def test_stream_chains_through_every_recorded_size(record, engines, name):
    """One chain per model through all its sizes in the fixture's order (OW changes while OH stays, and back).  `changed` by
    the rule of test_gpu_engine_stream.py: the features that differ from the stream's previous set -- also across a change
    of H x W -- or all active ones on a refresh, which here is the first step only."""
    engine, cases = engines(name), record[name]
    # S = 1: every recorded image in turn
    stream, prev, sizes = engine.stream(1), None, []
    for c in cases:
        sizes.append((c.h, c.w))
        for i in range(c.count):
            logits, density, changed = stream.step(c.images[i:i + 1], c.h, c.w)
            assert same_logits(logits[0], c.logits[i, 0]), (c, i)
            assert same_density(density, c.density[i:i + 1]), (c, i)
            want = c.ids[i].size if prev is None else np.setxor1d(prev, c.ids[i]).size
            assert int(changed[0]) == want, (c, i, int(changed[0]), want)
            prev = c.ids[i]
    assert len(set(sizes)) == len(sizes) >= 2
    # S = the cases' image count: stream s walks image s of every size (of a case with fewer images: image s % count)
    S = max(c.count for c in cases)
    stream, prev = engine.stream(S), None
    for c in cases:
        pick = [s % c.count for s in range(S)]
        logits, density, changed = stream.step(c.images[pick], c.h, c.w)
        assert same_logits(logits, c.logits[pick, 0]), c
        assert same_density(density, c.density[pick]), c
        cur = [c.ids[i] for i in pick]
        want = [a.size for a in cur] if prev is None else [np.setxor1d(a, b).size for a, b in zip(prev, cur)]
        assert [int(v) for v in changed] == want, (c, changed, want)
        prev = cur
    # and back to the first size: same bits after the whole history
    c = cases[0]
    logits, _, changed = stream.step(c.images[[s % c.count for s in range(S)]], c.h, c.w)
    assert same_logits(logits, c.logits[[s % c.count for s in range(S)], 0])
    assert [int(v) for v in changed] == [np.setxor1d(a, c.ids[s % c.count]).size for s, a in enumerate(prev)]


def frames_of(cases):
    """Every recorded frame of a model: (id arrays, logits [N, stacks, C], density [N])."""
    ids = [a for c in cases for a in c.ids]
    return ids, np.concatenate([c.logits for c in cases]), np.concatenate([c.density for c in cases])


def maps_of(ids, F) -> torch.Tensor:
    maps = torch.zeros(len(ids), F, dtype=torch.bool)
    for i, a in enumerate(ids):
        maps[i, torch.from_numpy(a)] = True
    return maps.cuda()


@pytest.mark.parametrize("name", ["nnue_c1arch.nnue", "nnue_tiny4x4.nnue", "nnue_wide96.nnue", "nnue_wide70.nnue", K4])
def test_feature_maps_of_the_recorded_ids(record, engines, name):
    """The recorded ids are what the engine's accumulate step saw, so maps built from them give the recorded logits -- on the
    wide models too: the ids hold no channel >= 64, and the feature-map entries apply no mask of their own."""
    engine = engines(name)
    F = int(engine.header["num_features"])
    ids, logits, density = frames_of(record[name])
    maps = maps_of(ids, F)
    got, dens = engine.evaluate_features(maps)
    assert same_logits(got, logits[:, 0]) and same_density(dens, density)
    got, dens = engine.evaluate_features(maps.to(torch.uint8) * 7)
    assert same_logits(got, logits[:, 0]) and same_density(dens, density)
    stream = engine.stream(len(ids))
    got, dens, changed = stream.step_features(maps)
    assert same_logits(got, logits[:, 0]) and same_density(dens, density)
    assert [int(v) for v in changed] == [a.size for a in ids]


@pytest.mark.parametrize("name", ["nnue_c1arch.nnue", "nnue_tiny4x4.nnue", "nnue_wide96.nnue", "nnue_wide70.nnue", K4])
def test_refresh_and_update_between_recorded_sets(record, engines, name):
    """refresh to frame i's recorded set, then add / remove lists to frame j's: frame j's recorded logits.  Two streams walk
    the model's frames in opposite directions, so one call carries two different list pairs."""
    engine = engines(name)
    ids, logits, density = frames_of(record[name])
    n = len(ids)
    order = [list(range(n)), list(range(n - 1, -1, -1))]
    stream = engine.stream(2)
    got, dens, changed = stream.refresh([ids[o[0]] for o in order])
    first = [o[0] for o in order]
    assert same_logits(got, logits[first, 0]) and same_density(dens, density[first])
    assert [int(v) for v in changed] == [ids[i].size for i in first]
    for t in range(1, n):
        i, j = [o[t - 1] for o in order], [o[t] for o in order]
        added = [np.setdiff1d(ids[b], ids[a]) for a, b in zip(i, j)]
        removed = [np.setdiff1d(ids[a], ids[b]) for a, b in zip(i, j)]
        got, dens, changed = stream.update(added, removed)
        assert same_logits(got, logits[j, 0]), (name, t)
        assert same_density(dens, density[j]), (name, t)
        assert [int(v) for v in changed] == [a.size + r.size for a, r in zip(added, removed)], (name, t)


def test_k4_every_single_stack_load(record, engines):
    for k in range(5):  # an index the file lacks loads stack 0; the engine answered the same call with stack 0's logits
        engine = engines(K4, k)
        assert engine.num_stacks == 1
        for c in record[K4]:
            assert c.stacks == [0, 1, 2, 3, 4]
            for path in ("gather", "matrix"):
                logits, density = engine.evaluate_logits(c.images, c.h, c.w, path=path)
                assert same_logits(logits, c.logits[:, k]), (c, k, path)
                assert same_density(density, c.density), (c, k, path)
    ids, logits, _ = frames_of(record[K4])
    for k in range(4):
        assert same_logits(engines(K4, k).evaluate_features(maps_of(ids, 256))[0], logits[:, k]), k


def test_k4_auto_with_given_stacks(record, engines):
    """bucket="auto" with stacks= from the caller: every image of every size meets every index of FORCED, through the gather
    form, the matrix form, the feature maps, a stream over images and one over add / remove lists."""
    engine = engines(K4, "auto")
    assert engine.num_stacks == 4
    cases = record[K4]
    B = 2 * len(FORCED)
    pick = [b % 2 for b in range(B)]
    given = [FORCED[b // 2] for b in range(B)]
    used = [used_stack(k) for k in given]
    stream, lists = engine.stream(B), engine.stream(B)
    prev = None
    for dtype in (torch.int64, torch.int32):
        stacks = torch.tensor(given, dtype=dtype).cuda()
        for c in cases:
            want = np.stack([c.logits[i, k] for i, k in zip(pick, used)])
            x = c.images[pick]
            for path in ("gather", "matrix"):
                logits, density, stack = engine.evaluate_logits(x, c.h, c.w, stacks=stacks, return_stacks=True, path=path)
                assert same_logits(logits, want), (c, path)
                assert same_density(density, c.density[pick]), (c, path)
                assert [int(k) for k in stack] == used, (c, path)
            cur = [c.ids[i] for i in pick]
            logits, density, stack = engine.evaluate_features(maps_of(cur, 256), stacks=stacks, return_stacks=True)
            assert same_logits(logits, want) and same_density(density, c.density[pick]) and [int(k) for k in stack] == used, c
            logits, density, changed = stream.step(x, c.h, c.w, stacks=stacks)
            assert same_logits(logits, want) and same_density(density, c.density[pick]), c
            assert [int(k) for k in stream.stacks] == used, c
            assert [int(v) for v in changed] == [a.size if prev is None else np.setxor1d(p, a).size
                                                 for a, p in zip(cur, prev or cur)], c
            if prev is None:
                logits, _, _ = lists.refresh(cur, stacks=stacks)
            else:
                logits, _, _ = lists.update([np.setdiff1d(a, p) for a, p in zip(cur, prev)],
                                            [np.setdiff1d(p, a) for a, p in zip(cur, prev)], stacks=stacks)
            assert same_logits(logits, want) and [int(k) for k in lists.stacks] == used, c
            prev = cur


def test_k4_auto_by_the_rule(record, engines):
    """The free choice lands on the record of the stack `stack_of` names for the RECORDED id count."""
    engine = engines(K4, "auto")
    stream = engine.stream(2)
    chosen = []
    for c in record[K4]:
        rule = [int(k) for k in stack_of(torch.tensor([a.size for a in c.ids]), 4, 256)]
        want = np.stack([c.logits[i, k] for i, k in enumerate(rule)])
        for path in ("gather", "matrix"):
            logits, density, stack = engine.evaluate_logits(c.images, c.h, c.w, return_stacks=True, path=path)
            assert [int(k) for k in stack] == rule, (c, path)
            assert same_logits(logits, want) and same_density(density, c.density), (c, path)
        logits, _, stack = engine.evaluate_features(maps_of(c.ids, 256), return_stacks=True)
        assert [int(k) for k in stack] == rule and same_logits(logits, want), c
        logits, density, _ = stream.step(c.images, c.h, c.w)
        assert [int(k) for k in stream.stacks] == rule, c
        assert same_logits(logits, want) and same_density(density, c.density), c
        chosen += rule
    assert set(chosen) == {0, 1, 2, 3}  # the recorded counts spread over all four stacks
