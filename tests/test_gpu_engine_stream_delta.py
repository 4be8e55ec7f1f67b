"""Sparse add / remove lists on the engine's streams (EngineStream.update / refresh / snapshot / restore,
nnue_engine_stream_update): set semantics on dirty lists, bit-identical to the oracle's ft_forward + forward_multiclass on the
resulting sets -- hence to ``evaluate_features`` and the real C++ engine -- whatever the history.  ``-m gpu``.
"The real C++ engine" is reached through the oracle here; refresh / update between id sets RECORDED from that engine, with its
recorded logits as the answer, is test_gpu_engine_recorded_shapes.py (tests/golden/engine_shapes.npz)."""
import numpy as np
import pytest
import torch

import nnue
import nnue_engine_oracle as eo
import serialize
from nnue_hip.engine import EngineModel

pytestmark = pytest.mark.gpu

I32_MAX = 2 ** 31 - 1


def same_sign_columns(model):  # every row adds +-64 to these columns: a few hundred active rows leave the int16 range
    model.input.weight[:, :8] = 1.0
    model.input.weight[:, 64:72] = -1.0


def _build(arch, buckets=1, edit=None):
    g, fps, l1, l2, l3, classes, size = arch
    torch.manual_seed(g * 100 + l1)
    model = nnue.NNUE(nnue.GridFeatureSet(g, fps), l1, l2, l3, num_classes=classes, input_size=size, num_ls_buckets=buckets)
    with torch.no_grad():
        model.input.weight.mul_(3.0)  # spread the quantised table; int16 sums then wrap like the engine's
        model.input.bias.uniform_(-1, 1)
        model.visual_threshold.fill_(-0.5)
        if edit is not None:
            edit(model)
    return model


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """arch (+ stack count, + edit) -> (path of its .nnue file, the oracle's parse of it); written once, never modified."""
    made = {}

    def get(arch, buckets=1, edit=None):
        key = (arch, buckets, edit)
        if key not in made:
            path = tmp_path_factory.mktemp("delta") / "m.nnue"
            serialize.serialize_model(_build(arch, buckets, edit), path)
            made[key] = (path, eo.load_nnue(path))
        return made[key]

    return get


def _want(ref, ids, stack=0):
    ids = np.array(sorted(ids), dtype=np.int64)
    return eo.forward_multiclass(ref["stacks"][stack], eo.ft_forward(ref, ids), ref["l1"], ref["l2"], ref["l3"])


def _maps(sets, F):
    m = torch.zeros(len(sets), F, dtype=torch.bool)
    for i, s in enumerate(sets):
        if s:
            m[i, torch.tensor(sorted(s), dtype=torch.int64)] = True
    return m.cuda()


def _csr(lists, dtype=torch.int32):
    ids = [x for l in lists for x in l]
    off = np.concatenate(([0], np.cumsum([len(l) for l in lists])))
    return torch.tensor(ids, dtype=dtype).cuda(), torch.tensor(off, dtype=dtype).cuda()


def _model_step(sets, valid, added, removed, F):
    """The host model of one update: (new sets, changed) under the set semantics."""
    new, changed = [], []
    for i, old in enumerate(sets):
        old = old if valid[i] else set()
        a = {int(x) for x in added[i] if 0 <= int(x) < F}
        r = {int(x) for x in removed[i] if 0 <= int(x) < F} if valid[i] and removed is not None else set()
        cur = (old - r) | a
        new.append(cur)
        changed.append(len(cur ^ old) if valid[i] else len(cur))
    return new, changed


def _check(ref, out, sets, changed, F):
    logits, density, got_changed = (t.cpu() for t in out)
    for i, s in enumerate(sets):
        assert np.array_equal(logits[i].numpy(), _want(ref, s)), i
        assert float(density[i]) == float(np.float32(len(s)) / np.float32(F)), i
    assert [int(v) for v in got_changed] == changed
    return logits


def _pick(rng, pool, k):
    pool = sorted(pool)
    k = min(k, len(pool))
    return [int(x) for x in rng.choice(pool, size=k, replace=False)] if k else []


def _dirty(rng, cur, F, k_add, k_rem, junk):
    """Added and removed lists for one stream whose set is `cur`, with every kind of dirt the kernel must ignore or resolve."""
    off = set(range(F)) - cur
    a = _pick(rng, off, k_add) + _pick(rng, cur, 3)                       # real adds + ids that are already on
    r = _pick(rng, cur, k_rem) + _pick(rng, off - set(a), 3)              # real removes + ids that are off
    both = _pick(rng, cur - set(r), 2) + _pick(rng, off - set(a), 2)      # in both lists: previously on and previously off
    a += both + a[:2] + both[:1] + junk                                   # duplicates, ids outside [0, F)
    r += both + r[:2] + both[-1:] + junk[::-1]
    rng.shuffle(a)
    rng.shuffle(r)
    return a, r


# ---- 1. oracle parity on dirty lists ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", [(10, 8, 256, 32, 16, 10, 32), (4, 96, 64, 8, 8, 3, 40), (8, 4, 96, 16, 8, 1000, 17),
                                  (10, 8, 1024, 128, 32, 10, 32)])
def test_oracle_parity_on_dirty_lists(files, arch):
    path, ref = files(arch)
    engine = EngineModel.load(path)
    F, S = ref["num_features"], 5
    rng = np.random.default_rng(arch[0] * 1000 + arch[2])
    stream = engine.stream(S)
    sets, valid = [set() for _ in range(S)], [False] * S
    for t in range(8):
        junk = [-1, F, F + 63, I32_MAX] + ([2 ** 40, -2 ** 35] if t % 4 == 0 else [])  # beyond int32 only as int64 ids
        added, removed = [], []
        for i in range(S):
            a, r = _dirty(rng, sets[i], F, F * 3 // 10 if t == 0 else int(rng.integers(0, 12)), int(rng.integers(0, 12)), junk)
            if i == t % S:  # one stream with empty ranges
                a, r = [], []
            added.append(a)
            removed.append(r)
        if t == 5:  # everything empty, no removed list at all
            added, removed = [[] for _ in range(S)], None
            out = stream.update(added)
        elif t % 4 == 0:  # device CSR, int64
            out = stream.update(_csr(added, torch.int64), _csr(removed, torch.int64))
        elif t % 4 == 2:  # device CSR, int32
            out = stream.update(_csr(added), _csr(removed))
        else:  # per-stream sequences, lists and tensors mixed
            out = stream.update([torch.tensor(a, dtype=torch.int64) if i % 2 else a for i, a in enumerate(added)],
                                [np.array(r, dtype=np.int64) if i % 2 else r for i, r in enumerate(removed)])
        sets, changed = _model_step(sets, valid, added, removed, F)
        valid = [True] * S
        logits = _check(ref, out, sets, changed, F)
        # the stored bits are the host model's sets: a step on their maps changes nothing
        again, _, moved = stream.step_features(_maps(sets, F))
        assert int(moved.abs().max()) == 0 and torch.equal(again.cpu(), logits)
    assert all(0 < len(s) < F for s in sets)


# ---- 2. the int16 wrap -----------------------------------------------------------------------------------------------------
def test_int16_wrap_on_a_fresh_update(files):
    path, ref = files((8, 32, 128, 16, 8, 10, 32), edit=same_sign_columns)
    engine = EngineModel.load(path)
    F, S = ref["num_features"], 4
    rng = np.random.default_rng(3)
    sets = [set(_pick(rng, range(F), n)) for n in (600, 900, 1500, F)]
    lists = [list(s) for s in sets]
    for l in lists:
        rng.shuffle(l)
    stream = engine.stream(S)
    _check(ref, stream.update(lists), sets, [len(s) for s in sets], F)
    wrapped = False
    for s in sets:
        raw = ref["ft_b"].astype(np.int64) + ref["ft_w"][sorted(s)].astype(np.int64).sum(axis=0)
        wrapped |= bool((raw > 32767).any() or (raw < -32768).any())
    assert wrapped  # some column's int32 sum left the int16 range: the stored accumulator wrapped
    # and it keeps wrapping through a delta that takes half of every set away again
    removed = [l[:len(l) // 2] for l in lists]
    new, changed = _model_step(sets, [True] * S, [[] for _ in range(S)], removed, F)
    _check(ref, stream.update(None, removed), new, changed, F)


# ---- 3. mixing with step / step_features, and resets -----------------------------------------------------------------------
def test_mixing_and_resets(files):
    arch = (10, 8, 256, 32, 16, 10, 32)
    path, ref = files(arch)
    engine = EngineModel.load(path)
    F, S = ref["num_features"], 4
    rng = np.random.default_rng(21)
    gen = torch.Generator().manual_seed(21)
    stream = engine.stream(S)
    frames = torch.randn(S, 3, 32, 32, generator=gen) * 1.5
    stream.step(frames.cuda())
    sets = [set(int(x) for x in eo.active_features(ref, eo.conv_forward(ref, frames[i].numpy().reshape(-1), 32, 32)[0]))
            for i in range(S)]
    valid = [True] * S

    def dirty_update():
        nonlocal sets
        pairs = [_dirty(rng, sets[i], F, 9, 7, [-1, F]) for i in range(S)]
        added, removed = [p[0] for p in pairs], [p[1] for p in pairs]
        out = stream.update(added, removed)
        sets, changed = _model_step(sets, valid, added, removed, F)
        _check(ref, out, sets, changed, F)
        return added, removed

    dirty_update()  # step -> update
    on = torch.rand(S, F, generator=gen) < 0.3
    _, _, moved = stream.step_features(on.cuda())  # -> step_features sees the updated sets as the previous ones
    new = [set(int(x) for x in np.nonzero(on[i].numpy())[0]) for i in range(S)]
    assert [int(v) for v in moved.cpu()] == [len(new[i] ^ sets[i]) for i in range(S)]
    sets = new
    dirty_update()  # -> update
    # reset([i]): stream i takes its valid added ids as the whole set and ignores removed
    stream.reset([2])
    valid[2] = False
    added, removed = dirty_update()
    assert sets[2] == {x for x in added[2] if 0 <= x < F}
    valid[2] = True
    # refresh(features) = reset() + update(features)
    lists = [_pick(rng, range(F), n) for n in (0, 1, 64, 333)]
    out = stream.refresh(lists)
    sets = [set(l) for l in lists]
    _check(ref, out, sets, [len(s) for s in sets], F)
    dirty_update()
    _, _, moved = stream.step_features(_maps(sets, F))
    assert int(moved.abs().max()) == 0


# ---- 4. long lists at the 224x224 shape ------------------------------------------------------------------------------------
def test_long_lists_at_the_224_shape(files):
    path, ref = files((32, 64, 512, 32, 32, 10, 224))
    engine = EngineModel.load(path)
    F, S = ref["num_features"], 4
    assert F == 65536
    rng = np.random.default_rng(9)
    stream = engine.stream(S)

    def check(out, sets, changed):
        want_logits, want_density = engine.evaluate_features(_maps(sets, F))
        assert torch.equal(out[0], want_logits) and torch.equal(out[1], want_density)
        assert [int(v) for v in out[2].cpu()] == changed

    lists = [[int(x) for x in rng.permutation(F)[:n]] for n in (20000, 3, 0, 5000)]  # beyond any LDS work-list chunk
    sets = [set(l) for l in lists]
    check(stream.update(_csr(lists)), sets, [len(s) for s in sets])
    for t in range(2):  # deltas of 5 000 ids with duplicates, both directions
        added = [[int(x) for x in rng.integers(0, F, size=5000)] for _ in range(S)]
        removed = [[int(x) for x in rng.integers(0, F, size=5000)] for _ in range(S)]
        if t:
            removed[1], added[3] = [], []
        out = stream.update(_csr(added), _csr(removed))
        sets, changed = _model_step(sets, [True] * S, added, removed, F)
        check(out, sets, changed)


# ---- 5. offsets are clipped to the id buffer -------------------------------------------------------------------------------
def test_offsets_are_clipped_without_reading_outside_the_ids(files):
    path, ref = files((10, 8, 256, 32, 16, 10, 32))
    engine = EngineModel.load(path)
    F, S = ref["num_features"], 6
    rng = np.random.default_rng(5)
    n_a, n_r = 40, 24
    big_a = torch.tensor(rng.integers(0, F, size=4096), dtype=torch.int32).cuda()  # the lists are views of larger allocations:
    big_r = torch.tensor(rng.integers(0, F, size=4096), dtype=torch.int32).cuda()  # a wrong clip reads valid memory, wrong ids
    a_ids, r_ids = big_a[:n_a], big_r[:n_r]
    stream = engine.stream(S)
    base = [_pick(rng, range(F), 200) for _ in range(S)]
    stream.update(base)
    sets = [set(b) for b in base]
    # added:   [0, 10) | reversed | [4, 30) | straddles n: [30, 40) | beyond n then negative: empty | [-7, 2^31 - 1) = everything
    a_off = [0, 10, 4, 30, n_a + 60, -7, I32_MAX]
    # removed: reversed | [2, 20) | straddles n: [20, 24) | beyond n: empty | down to -2^31: empty | [0, 12)
    r_off = [5, 2, 20, n_r + 1, n_r + 9, -I32_MAX - 1, 12]

    def clip(ids, off, n):
        host = ids.cpu().tolist()
        out = []
        for b in range(S):
            lo, hi = (min(max(int(v), 0), n) for v in (off[b], off[b + 1]))
            out.append(host[lo:hi] if hi > lo else [])
        return out

    added, removed = clip(a_ids, a_off, n_a), clip(r_ids, r_off, n_r)
    assert sum(map(len, added)) > 0 and sum(map(len, removed)) > 0 and any(not l for l in added)
    out = stream.update((a_ids, torch.tensor(a_off, dtype=torch.int64).cuda()), (r_ids, torch.tensor(r_off, dtype=torch.int64).cuda()))
    sets, changed = _model_step(sets, [True] * S, added, removed, F)
    _check(ref, out, sets, changed, F)
    # int32 offsets take the same path without the host-side saturation
    a32 = [min(max(v, -I32_MAX - 1), I32_MAX) for v in a_off]
    out = stream.update((a_ids, torch.tensor(a32, dtype=torch.int32).cuda()), (r_ids, torch.tensor(r_off, dtype=torch.int32).cuda()))
    sets, changed = _model_step(sets, [True] * S, added, removed, F)
    _check(ref, out, sets, changed, F)


# ---- 6. layer stacks -------------------------------------------------------------------------------------------------------
def test_stacks_by_the_rule_and_given(files):
    arch = (10, 8, 256, 32, 16, 10, 32)
    path, ref = files(arch, buckets=4)
    engine = EngineModel.load(path, bucket="auto")
    F, S, K = ref["num_features"], 5, 4
    rng = np.random.default_rng(6)
    stream = engine.stream(S)
    lists = [_pick(rng, range(F), n) for n in (10, 250, 450, 700, 200)]
    sets = [set(l) for l in lists]
    out = stream.update(lists)
    want = engine.evaluate_features(_maps(sets, F), return_stacks=True)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]) and torch.equal(stream.stacks, want[2])
    assert stream.stacks.cpu().tolist() == [min(K - 1, len(s) * K // (F + 1)) for s in sets] == [0, 1, 2, 3, 0]
    for i, s in enumerate(sets):
        assert np.array_equal(out[0][i].cpu().numpy(), _want(ref, s, int(stream.stacks[i])))
    # a delta that moves stream 4 across a boundary: the stack follows the new count
    more = _pick(rng, set(range(F)) - sets[4], 10)
    out = stream.update([[], [], [], [], more])
    sets[4] |= set(more)
    want = engine.evaluate_features(_maps(sets, F), return_stacks=True)
    assert torch.equal(out[0], want[0]) and torch.equal(stream.stacks, want[2]) and int(stream.stacks[4]) == 1
    # stacks= overrides the rule (int64, an index outside [0, K) = stack 0)
    given = torch.tensor([3, 2, 1, 0, 17], dtype=torch.int64).cuda()
    out = stream.update([[] for _ in range(S)], stacks=given)
    want = engine.evaluate_features(_maps(sets, F), stacks=given, return_stacks=True)
    assert torch.equal(out[0], want[0]) and torch.equal(stream.stacks, want[2])
    assert stream.stacks.cpu().tolist() == [3, 2, 1, 0, 0] and int(out[2].abs().max()) == 0
    # a single-stack model takes no stacks=
    single = EngineModel.load(path, bucket=0).stream(S)
    with pytest.raises(ValueError):
        single.update(lists, stacks=given)
    _, _, changed = single.update(lists)
    assert changed.cpu().tolist() == [len(s) for s in (set(l) for l in lists)]  # the refused call changed nothing


# ---- 7. requantize ---------------------------------------------------------------------------------------------------------
def _shift(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        model.input.weight.add_((torch.rand(model.input.weight.shape, generator=gen) - 0.5).to(model.input.weight.device) * 0.5)
        model.input.bias.add_(0.25)


def test_update_rebuilds_after_a_requantize():
    arch = (10, 8, 256, 32, 16, 10, 32)
    model = _build(arch).cuda()
    engine = EngineModel.from_model(model)
    F, S = int(engine.header["num_features"]), 4
    rng = np.random.default_rng(7)
    stream = engine.stream(S)
    lists = [_pick(rng, range(F), n) for n in (300, 5, 0, 640)]
    stream.update(lists)
    sets = [set(l) for l in lists]
    added = [_pick(rng, set(range(F)) - s, 4) for s in sets]
    removed = [_pick(rng, s, 3) for s in sets]
    stream.update(added, removed)
    sets, _ = _model_step(sets, [True] * S, added, removed, F)
    snap = stream.snapshot()
    stale = engine.evaluate_features(_maps(sets, F))[0].clone()

    _shift(model, 1)
    engine.requantize(model)
    small_a = [_pick(rng, set(range(F)) - s, 2) for s in sets]
    small_r = [_pick(rng, s, 1) for s in sets]
    new, changed = _model_step(sets, [True] * S, small_a, small_r, F)
    want = engine.evaluate_features(_maps(new, F))
    assert not torch.equal(engine.evaluate_features(_maps(sets, F))[0], stale)  # the table did change
    out = stream.update(small_a, small_r)  # the sets were kept, the sums rebuilt over the new table
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]) and out[2].cpu().tolist() == changed
    out = stream.update([[] for _ in range(S)])  # once: the next update is incremental again, on the rebuilt sums
    assert torch.equal(out[0], want[0]) and int(out[2].abs().max()) == 0
    again, _, moved = stream.step_features(_maps(new, F))
    assert torch.equal(again, want[0]) and int(moved.abs().max()) == 0
    # through a snapshot taken before the requantize and restored after it
    stream.restore(snap)
    out = stream.update(small_a, small_r)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]) and out[2].cpu().tolist() == changed
    # ... and step_features after such a restore refreshes instead of trusting the old sums
    stream.restore(snap)
    out = stream.step_features(_maps(new, F))
    assert torch.equal(out[0], want[0]) and out[2].cpu().tolist() == [len(s) for s in new]


# ---- 8. snapshot and restore -----------------------------------------------------------------------------------------------
def test_snapshot_and_restore(files):
    path, ref = files((10, 8, 256, 32, 16, 10, 32))
    engine = EngineModel.load(path)
    F, S = ref["num_features"], 3
    rng = np.random.default_rng(8)
    base = [_pick(rng, range(F), n) for n in (100, 400, 7)]

    def delta(seed):
        r = np.random.default_rng(seed)
        return [_pick(r, range(F), 12) for _ in range(S)], [_pick(r, range(F), 12) for _ in range(S)]

    a, b = engine.stream(S), engine.stream(S)
    a.update(base)
    b.update(base)
    snap = a.snapshot()
    a.update(*delta(1))
    a.update(*delta(2))
    a.restore(snap)
    out_a, out_b = a.update(*delta(3)), b.update(*delta(3))
    for x, y in zip(out_a, out_b):
        assert torch.equal(x, y)
    sets, changed = _model_step([set(l) for l in base], [True] * S, *delta(3), F)
    _check(ref, out_a, sets, changed, F)
    assert torch.equal(a.state, b.state)
    # the snapshot is a copy: it still holds the base sets and can be restored again
    a.restore(snap)
    _, _, moved = a.step_features(_maps([set(l) for l in base], F))
    assert int(moved.abs().max()) == 0
    # foreign snapshots
    with pytest.raises(ValueError):
        engine.stream(S + 1).restore(snap)
    with pytest.raises(ValueError):
        EngineModel.load(path).stream(S).restore(snap)
    with pytest.raises(TypeError):
        a.restore(a.state)


# ---- 9. capture ------------------------------------------------------------------------------------------------------------
def test_captured_update_replays_with_new_lists(files):
    path, ref = files((10, 8, 256, 32, 16, 10, 32))
    engine = EngineModel.load(path)
    F, S, cap = ref["num_features"], 4, 256
    rng = np.random.default_rng(12)
    a_ids, r_ids = (torch.full((cap,), -1, dtype=torch.int32).cuda() for _ in range(2))
    a_off, r_off = (torch.zeros(S + 1, dtype=torch.int32).cuda() for _ in range(2))
    engine.stream(S).update((a_ids, a_off), (r_ids, r_off))  # every kernel has run once before the capture
    eager, graphed = engine.stream(S), engine.stream(S)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            out = graphed.update((a_ids, a_off), (r_ids, r_off))
    torch.cuda.current_stream().wait_stream(side)
    sets, valid = [set() for _ in range(S)], [False] * S
    for t, sizes in enumerate(((60, 0, 17, 90), (5, 30, 0, 2), (0, 9, 9, 1))):
        added = [_pick(rng, range(F), n) for n in sizes]
        removed = [_pick(rng, range(F), n) for n in sizes[::-1]]
        for buf, off, lists in ((a_ids, a_off, added), (r_ids, r_off, removed)):
            ids, offsets = _csr(lists)
            buf.fill_(-1)
            buf[:ids.numel()] = ids
            off.copy_(offsets)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = eager.update((a_ids, a_off), (r_ids, r_off))
        for x, y in zip(out, want):
            assert torch.equal(x, y), t
        sets, changed = _model_step(sets, valid, added, removed, F)
        valid = [True] * S
        _check(ref, out, sets, changed, F)
    assert torch.equal(eager.state, graphed.state)


# ---- 10. errors ------------------------------------------------------------------------------------------------------------
def test_update_errors_change_nothing(files):
    path, ref = files((10, 8, 256, 32, 16, 10, 32))
    engine = EngineModel.load(path)
    F, S = ref["num_features"], 3
    stream = engine.stream(S)
    ids, off = torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    with pytest.raises(ValueError):
        stream.update((ids, off))  # CPU tensors
    with pytest.raises(ValueError):
        stream.update((ids.cuda(), off))
    with pytest.raises(ValueError):
        stream.update((ids.cuda().float(), off.cuda()))  # float ids
    with pytest.raises(ValueError):
        stream.update((ids.cuda(), off.cuda().float()))
    with pytest.raises(ValueError):
        stream.update((ids.cuda(), off.cuda()[:3]))  # offsets of another stream count
    with pytest.raises(ValueError):
        stream.update((ids.cuda().view(3, 1), off.cuda()))
    with pytest.raises(ValueError):
        stream.update((ids.cuda(), off.cuda()), (ids.cuda(), off.cuda().view(1, 4)))
    with pytest.raises(ValueError):
        stream.update([[1], [2]])  # a sequence of the wrong length
    with pytest.raises(ValueError):
        stream.update([[1], [2], [3]], [[1], [2], [3], [4]])
    with pytest.raises(ValueError):
        stream.update([[1.5], [2], [3]])
    with pytest.raises(ValueError):
        stream.refresh([[1], [2]])
    with pytest.raises(ValueError):
        stream.update([[1], [2], [3]], stacks=torch.zeros(S, dtype=torch.int32).cuda())  # a single-stack model
    # a refused call changed nothing: the next real call still sees fresh streams and ignores `removed`
    out = stream.update([[1, 5], [2], []], [[5], [2], [9]])
    _check(ref, out, [{1, 5}, {2}, set()], [2, 1, 0], F)
