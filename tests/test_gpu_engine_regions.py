"""The stream step from the dirty rectangles of uint8 frames (EngineStream.step_u8_regions, nnue_engine_stream_step_u8_regions)
against two witnesses, bitwise on logits, density, `changed` and the stacks:

1. the CPU oracle (oracle/nnue_engine_oracle.py) on ``floats_of(frames, "hwc")`` -- where the caller's promise holds that is the
   whole frame's evaluation; where it is broken on purpose, the DEFINITION is restated here on the oracle's feature sets: the
   old set with the features of every cell whose 3 x 3 window meets a clipped rectangle replaced from the new frame;
2. a twin stream fed ``step_u8(layout="hwc")`` on the whole frames.
``-m gpu``."""
import numpy as np
import pytest
import torch

import nnue_engine_oracle as orc
from nnue_hip.engine import EngineModel
from test_gpu_engine_u8 import floats_of, make_store, models, oracle_rows, same_bits  # noqa: F401  (models is a fixture)

pytestmark = pytest.mark.gpu

C1, TINY, WIDE70, K4, BIG = "nnue_c1arch.nnue", "nnue_tiny4x4.nnue", "nnue_wide70.nnue", "nnue_k4.nnue", "big224"
# (model, H, W): stride 4 with a map smaller than F (a zero-filled rest) | stride 1 | stride 6 | 70 channels, the c < 64 mask |
# bucket="auto" | stride 8, 64 channels, more flips and more bit words than one round
CHAINS = [(C1, 32, 32), (C1, 32, 20), (C1, 10, 4), (TINY, 17, 11), (WIDE70, 27, 14), (K4, 17, 17), (K4, 17, 22), (BIG, 224, 224),
          (BIG, 224, 200)]
IDS = [f"{m.replace('nnue_', '').replace('.nnue', '')}-{h}x{w}" for m, h, w in CHAINS]
K4_RANGES = [(0, 40), (0, 256), (200, 256)]  # the brightness classes of make_store: a redrawn patch can move the stack


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def csr(lists):
    """Per-stream rectangle lists as the device pair (rects int32 [R, 4], offsets int32 [S + 1])."""
    flat = [r for l in lists for r in l]
    off = np.concatenate(([0], np.cumsum([len(l) for l in lists])))
    return dev(np.asarray(flat, dtype=np.int32).reshape(-1, 4)), dev(off.astype(np.int32))


def redraw(frames, rng, name, most=3):
    """Every frame with one to `most` random rectangles of bytes redrawn; returns (new frames, per-stream rectangle lists)."""
    out = frames.copy()
    _, h, w, _ = out.shape
    lists = []
    for f in out:
        rects = []
        for _ in range(rng.randint(1, most + 1)):
            lo, hi = K4_RANGES[rng.randint(3)] if name == K4 else (0, 256)
            span = (h, w) if name == K4 else (max(2, h // 3), max(2, w // 3))
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            y1, x1 = min(h, y0 + rng.randint(1, span[0] + 1)), min(w, x0 + rng.randint(1, span[1] + 1))
            f[y0:y1, x0:x1] = rng.randint(lo, hi, size=(y1 - y0, x1 - x0, 3))
            rects.append((y0, x0, y1, x1))
        lists.append(rects)
    return out, lists


def feature_sets(m, frames):
    """The oracle's active sets of whole frames under layout hwc: bool [n, F]."""
    n, h, w, _ = frames.shape
    on = np.zeros((n, m["num_features"]), dtype=bool)
    for i, row in enumerate(floats_of(frames, "hwc")):
        conv, _ = orc.conv_forward(m, row, h, w)
        on[i, orc.active_features(m, conv)] = True
    return on


def touched_cells(m, h, w, rects):
    """The definition: bool [OH, OW], cell (oh, ow) reads rows oh*stride-1 .. +1 and columns ow*stride-1 .. +1; it is touched
    when that window shares a pixel with a rectangle clipped to the frame.  Brute force over pixels, on purpose."""
    s = orc.conv_stride(h, m["grid"])
    oh_n, ow_n = (h - 1) // s + 1, (w - 1) // s + 1
    dirty = np.zeros((h, w), dtype=bool)
    for y0, x0, y1, x1 in rects:
        y0, x0, y1, x1 = max(0, y0), max(0, x0), min(h, y1), min(w, x1)
        if y0 < y1 and x0 < x1:
            dirty[y0:y1, x0:x1] = True
    padded = np.zeros((h + 2, w + 2), dtype=bool)
    padded[1:-1, 1:-1] = dirty
    cells = np.zeros((oh_n, ow_n), dtype=bool)
    for oh in range(oh_n):
        for ow in range(ow_n):
            cells[oh, ow] = padded[oh * s:oh * s + 3, ow * s:ow * s + 3].any()
    return cells


def defined_step(m, h, w, old, full, rects):
    """new set = old with the features of the touched cells taken from `full` (the whole new frame's set)."""
    cells = touched_cells(m, h, w, rects)
    oc = m["oc"]
    mask = np.zeros(m["num_features"], dtype=bool)
    mask[:cells.size * oc] = np.repeat(cells.reshape(-1), oc)
    return np.where(mask, full, old)


def want_of(m, on, stack=0):
    """(logits float32, density float32) of a feature set by the oracle's FeatureTransformer and layer stack."""
    ids = np.nonzero(on)[0].astype(np.int64)
    logits = orc.forward_multiclass(m["stacks"][stack], orc.ft_forward(m, ids), m["l1"], m["l2"], m["l3"])
    return logits.astype(np.float32), np.float32(ids.size) / np.float32(m["num_features"])


def check_sets(m, out, new, old, valid=True):
    """One step's outputs against the oracle on the sets `new` [S, F]; changed = |new xor old| (|new| where not valid)."""
    logits, density, changed = (t.cpu().numpy() for t in out)
    for i in range(len(new)):
        lg, dn = want_of(m, new[i])
        assert np.array_equal(logits[i].view(np.int32), lg.view(np.int32)), i
        assert density[i] == dn, i
        assert int(changed[i]) == int((new[i] ^ old[i]).sum() if valid else new[i].sum()), i


def equal_outputs(got, want):
    return all(torch.equal(a, b) for a, b in zip(got, want))


# ---- 1. chains -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h,w", CHAINS, ids=IDS)
def test_chain(models, name, h, w):
    """Five frames; frame t+1 is frame t with bytes redrawn inside one to three rectangles per stream, the rectangles handed over
    (per-stream lists and the device CSR pair in turn).  The first step finds the streams not valid."""
    engine, m = models(name)
    auto = name == K4
    S = 2 if name == BIG else 3
    rng = np.random.RandomState(1000 + 31 * h + w)
    a, b = engine.stream(S), engine.stream(S)
    frames = make_store(name, h, w, seed=41)[:S]
    rects = [[(0, 0, 1, 1)]] * S
    old = np.zeros((S, m["num_features"]), dtype=bool)
    stacks_seen, moved = set(), 0
    for t in range(5):
        if t:
            frames, rects = redraw(frames, rng, name)
        store = dev(frames)
        got = a.step_u8_regions(store, rects if t % 2 else csr(rects))
        twin = b.step_u8(store, layout="hwc")
        assert equal_outputs(got, twin), t
        want_logits, want_density, want_stacks = oracle_rows(m, floats_of(frames, "hwc"), h, w, auto)
        assert same_bits(got[0], want_logits) and same_bits(got[1], want_density), t
        new = feature_sets(m, frames)
        assert [int(c) for c in got[2]] == [int(v) for v in ((new ^ old).sum(axis=1) if t else new.sum(axis=1))], t
        moved += int(got[2].sum()) if t else 0
        if auto:
            assert [int(k) for k in a.stacks] == want_stacks and torch.equal(a.stacks, b.stacks), t
            stacks_seen |= set(want_stacks)
        old = new
    assert moved > 0  # the redrawn bytes moved features (at stride 9 many a small rectangle lies between the cells' windows)
    if auto:
        assert len(stacks_seen) >= 2  # the chain re-selected a stack
    if name == C1 and (h, w) == (32, 20):
        assert orc.conv_forward(m, floats_of(frames, "hwc")[0], h, w)[0].size < m["num_features"]  # the zero-filled rest exists


# ---- 2. every pixel --------------------------------------------------------------------------------------------------------------
def _every_pixel(models, name, h, w, pixels):
    """Stream 0 takes the pixels in the given order, stream 1 in reverse: the pixel's three bytes become 255 - v and the step gets
    the 1 x 1 rectangle at it, as an int32 [S, 4] tensor.  Any cell the kernel's range misses keeps a stale bit somewhere."""
    engine, m = models(name)
    a, b = engine.stream(2), engine.stream(2)
    frames = make_store(name, h, w, seed=43)[:2].copy()
    store = dev(frames)
    assert equal_outputs(a.step_u8_regions(store, [[], []]), b.step_u8(store, layout="hwc"))
    old = feature_sets(m, frames)
    moved = 0
    for p, q in zip(pixels, pixels[::-1]):
        for f, (y, x) in zip(frames, (p, q)):
            f[y, x] = 255 - f[y, x]
        store = dev(frames)
        rects = dev(np.array([[p[0], p[1], p[0] + 1, p[1] + 1], [q[0], q[1], q[0] + 1, q[1] + 1]], dtype=np.int32))
        got = a.step_u8_regions(store, rects)
        assert equal_outputs(got, b.step_u8(store, layout="hwc")), (p, q)
        new = feature_sets(m, frames)
        check_sets(m, got, new, old)
        moved += int(got[2].sum())
        old = new
    assert moved > 0


@pytest.mark.parametrize("name,h,w", [(TINY, 17, 11), (C1, 10, 4)], ids=["stride6", "stride1"])
def test_every_pixel(models, name, h, w):
    _every_pixel(models, name, h, w, [(y, x) for y in range(h) for x in range(w)])


def test_every_border_pixel_at_stride_4(models):
    h, w = 32, 20
    rows, cols = list(range(10)) + list(range(h - 5, h)), list(range(10)) + list(range(w - 5, w))
    _every_pixel(models, C1, h, w, [(y, x) for y in rows for x in cols])


# ---- 3. set semantics ------------------------------------------------------------------------------------------------------------
def test_set_semantics(models):
    """Overlapping and repeated rectangles, rectangles reaching beyond the frame, inverted and empty ones, offsets outside [0, R]
    and a stream without rectangles, each against the definition on the oracle's sets."""
    engine, m = models(C1)
    h, w, S = 32, 20, 4
    rng = np.random.RandomState(3)
    a = engine.stream(S)
    frames = make_store(C1, h, w, seed=47)[:S].copy()
    first = a.step_u8_regions(dev(frames), [[]] * S)
    old = feature_sets(m, frames)
    check_sets(m, first, old, old, valid=False)

    # stream 0: overlaps and duplicates; 1: beyond the frame on every side; 2: inverted, empty, wholly outside -- over an unchanged
    # frame; 3: no rectangle, unchanged frame
    frames[0, 4:20, 2:12] = rng.randint(0, 256, size=(16, 10, 3))
    frames[1, :6, :5] = rng.randint(0, 256, size=(6, 5, 3))
    frames[1, 25:, 13:] = rng.randint(0, 256, size=(7, 7, 3))
    lists = [[(4, 2, 14, 12), (10, 2, 20, 12), (4, 2, 14, 12), (8, 4, 12, 8), (4, 2, 14, 12)],
             [(-7, -3, 6, 5), (25, 13, 1000, 2 ** 31 - 1), (-2 ** 31, -2 ** 31, 0, 0)],
             [(9, 9, 3, 3), (5, 5, 5, 9), (5, 9, 9, 9), (h, 0, h + 4, w), (0, w, h, w + 9), (-9, -9, 0, 0), (12, 3, 2, 18)],
             []]
    got = a.step_u8_regions(dev(frames), lists)
    full = feature_sets(m, frames)
    new = np.stack([defined_step(m, h, w, old[i], full[i], lists[i]) for i in range(S)])
    assert np.array_equal(new, full)  # the promise holds here: the definition gives the whole frame's sets
    check_sets(m, got, new, old)
    assert int(got[2][0]) > 0 and int(got[2][1]) > 0
    assert [int(c) for c in got[2][2:]] == [0, 0]
    assert torch.equal(got[0][2:], first[0][2:]) and torch.equal(got[1][2:], first[1][2:])
    twin = engine.stream(S)
    assert equal_outputs(got[:2], twin.step_u8(dev(frames), layout="hwc")[:2])
    old = new

    # offsets outside [0, R]: clipped as update_range clips them -- stream 0 owns [0, 2), 1 nothing ([2, 2)), 2 [2, R), 3 nothing
    # ([R, R) after the clip; its range is reversed before it).  Every stream's frame changes everywhere: only owners see it.
    frames = make_store(C1, h, w, seed=53)[:S].copy()
    boxes = [(0, 0, 8, 8), (20, 10, 32, 20), (0, 0, h, w), (3, 3, 9, 9), (16, 0, 24, 20)]
    R = len(boxes)
    offsets = np.array([-5, 2, 2, R + 100, R + 7], dtype=np.int64)
    got = a.step_u8_regions(dev(frames), (dev(np.asarray(boxes, dtype=np.int32)), dev(offsets)))
    owned = [boxes[0:2], [], boxes[2:R], []]
    full = feature_sets(m, frames)
    new = np.stack([defined_step(m, h, w, old[i], full[i], owned[i]) for i in range(S)])
    check_sets(m, got, new, old)
    assert np.array_equal(new[2], full[2]) and not np.array_equal(new[0], full[0])
    assert [int(c) for c in got[2][[1, 3]]] == [0, 0] and int(got[2][0]) > 0


# ---- 4. the definition when the promise is broken ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h,w", [(C1, 32, 20), (TINY, 17, 11), (WIDE70, 27, 14), (C1, 10, 4)],
                         ids=["stride4", "stride6", "wide70", "stride1"])
def test_bytes_change_outside_the_rectangles(models, name, h, w):
    engine, m = models(name)
    S = 3
    rng = np.random.RandomState(5 + h)
    a = engine.stream(S)
    frames = make_store(name, h, w, seed=59)[:S]
    a.step_u8_regions(dev(frames), [[]] * S)
    old = feature_sets(m, frames)
    for t in range(3):
        frames = rng.randint(0, 256, size=frames.shape).astype(np.uint8)  # every byte redrawn
        lists = []
        for _ in range(S):
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            lists.append([(y0, x0, min(h, y0 + rng.randint(1, 6)), min(w, x0 + rng.randint(1, 6)))] * (1 + t % 2))
        got = a.step_u8_regions(dev(frames), lists)
        full = feature_sets(m, frames)
        new = np.stack([defined_step(m, h, w, old[i], full[i], lists[i]) for i in range(S)])
        assert not np.array_equal(new, full), t  # the rest of the frame did move, and is not looked at
        check_sets(m, got, new, old)
        old = new
    # the stored sets are what the definition says: a whole-frame step now reports exactly the difference to them
    _, _, changed = a.step_u8(dev(frames), layout="hwc")
    assert [int(c) for c in changed] == [int(v) for v in (full ^ old).sum(axis=1)]


# ---- 5. streams that are not valid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h,w", [(C1, 32, 20), (K4, 17, 22), (WIDE70, 27, 14)], ids=["c1arch", "k4", "wide70"])
def test_streams_that_are_not_valid(models, name, h, w):
    engine, m = models(name)
    S = 3
    frames = make_store(name, h, w, seed=61)
    store = dev(frames)
    idx = torch.tensor([4, 0, 7], device="cuda")
    small = dev(np.array([[1, 1, 2, 2]] * S, dtype=np.int32))
    a = engine.stream(S)
    want = engine.evaluate_logits_u8(store, idx, layout="hwc", return_stacks=True)
    logits, density, changed = a.step_u8_regions(store, small, indices=idx)  # fresh
    assert torch.equal(logits, want[0]) and torch.equal(density, want[1])
    sets = feature_sets(m, frames[[4, 0, 7]])
    assert [int(c) for c in changed] == [int(v) for v in sets.sum(axis=1)]
    if name == K4:
        assert torch.equal(a.stacks, want[2])
    # reset of one stream: that one takes its whole new frame, the others only their rectangle (which holds no change)
    idx2 = torch.tensor([4, 8, 7], device="cuda")
    a.reset([1])
    logits, density, changed = a.step_u8_regions(store, small, indices=idx2)
    want = engine.evaluate_logits_u8(store, idx2, layout="hwc")
    assert torch.equal(logits, want[0]) and torch.equal(density, want[1])
    assert [int(c) for c in changed] == [0, int(feature_sets(m, frames[[8]]).sum()), 0]
    a.reset()
    logits, _, _ = a.step_u8_regions(store[:S], [[]] * S)  # no rectangle at all: still the whole frame
    assert torch.equal(logits, engine.evaluate_logits_u8(store[:S], layout="hwc")[0])


# ---- 6. more flips than one work-list round ------------------------------------------------------------------------------------------
def test_more_flips_than_one_round(models):
    engine, m = models(BIG)
    h = w = 224
    S = 2
    a, b = engine.stream(S), engine.stream(S)
    zero = torch.zeros((S, h, w, 3), dtype=torch.uint8, device="cuda")
    assert equal_outputs(a.step_u8_regions(zero, [[]] * S), b.step_u8(zero, layout="hwc"))
    frames = np.random.RandomState(67).randint(0, 256, size=(S, h, w, 3)).astype(np.uint8)
    store = dev(frames)
    got = a.step_u8_regions(store, dev(np.array([[0, 0, h, w]] * S, dtype=np.int32)))
    assert equal_outputs(got, b.step_u8(store, layout="hwc"))
    want_logits, want_density, _ = oracle_rows(m, floats_of(frames, "hwc"), h, w, False)
    assert same_bits(got[0], want_logits) and same_bits(got[1], want_density)
    assert int(got[2].min()) > 1024  # kUpdateChunk: the work list was filled and walked more than once


# ---- 7. order with the other calls -------------------------------------------------------------------------------------------------
def test_interleaved_with_the_other_stream_calls(models):
    """a takes region steps, b whole-frame steps; update, step_features, snapshot and restore go to both.  After an update the
    rectangle also covers the cells of the updated ids, after step_features the whole frame: then the promise holds again."""
    engine, m = models(C1)
    h, w, S = 32, 32, 3
    F, oc = m["num_features"], m["oc"]
    rng = np.random.RandomState(71)
    a, b = engine.stream(S), engine.stream(S)
    frames = make_store(C1, h, w, seed=73)[:S]
    whole = [[(0, 0, h, w)]] * S

    def both(rects):
        store = dev(frames)
        got = a.step_u8_regions(store, rects)
        assert equal_outputs(got, b.step_u8(store, layout="hwc"))
        want_logits, want_density, _ = oracle_rows(m, floats_of(frames, "hwc"), h, w, False)
        assert same_bits(got[0], want_logits) and same_bits(got[1], want_density)
        return got

    both([[]] * S)
    frames, rects = redraw(frames, rng, C1)
    both(rects)
    # update: features of cell (0, 0) and (0, 1) flip by hand; the next rectangles also cover pixel (0, 0) .. (1, 5)
    added = (dev(np.array([0, 1, oc, 0, 2, 3], dtype=np.int32)), dev(np.array([0, 2, 4, 6], dtype=np.int32)))
    removed = (dev(np.array([4, 5, 6], dtype=np.int32)), dev(np.arange(S + 1, dtype=np.int32)))
    assert equal_outputs(a.update(added, removed), b.update(added, removed))
    frames, rects = redraw(frames, rng, C1)
    both([r + [(0, 0, 2, 6)] for r in rects])
    # step_features: an arbitrary map replaces every set -- arbitrary over the conv map's ids; the ids behind it belong to no cell,
    # so a region step keeps them as they are, and the map leaves them off as the whole-frame step does (threshold > 0)
    assert m["threshold"] > 0
    maps = rng.randint(0, 2, size=(S, F)).astype(np.uint8)
    maps[:, 8 * 8 * oc:] = 0
    maps = dev(maps)
    assert equal_outputs(a.step_features(maps), b.step_features(maps))
    frames, _ = redraw(frames, rng, C1)
    both(whole)
    # snapshot / restore around two region steps: the same step from the same point gives the same bits
    snap_a, snap_b = a.snapshot(), b.snapshot()
    frames, rects = next_frames, next_rects = redraw(frames, rng, C1)
    first = both(rects)
    frames, rects = redraw(frames, rng, C1)
    both(rects)
    a.restore(snap_a)
    b.restore(snap_b)
    frames = next_frames
    again = both(next_rects)
    assert equal_outputs(again, first) and int(again[2].max()) > 0
    # a whole-frame step after a region step finds nothing left to change
    logits, density, changed = a.step_u8(dev(frames), layout="hwc")
    assert [int(c) for c in changed] == [0] * S
    assert torch.equal(logits, again[0]) and torch.equal(density, again[1])


def test_after_requantize(models):
    """One region step with the full-frame rectangle after requantize: the new tensors' whole-frame evaluation."""
    import nnue
    torch.manual_seed(5)
    live = nnue.NNUE(nnue.GridFeatureSet(10, 8), 32, 8, 8, num_classes=5, input_size=32).cuda()
    with torch.no_grad():
        live.visual_threshold.fill_(-0.5)
    engine = EngineModel.from_model(live)
    h, w, S = 32, 32, 3
    rng = np.random.RandomState(79)
    a, b = engine.stream(S), engine.stream(S)
    frames = make_store(C1, h, w, seed=83)[:S]
    assert equal_outputs(a.step_u8_regions(dev(frames), [[]] * S), b.step_u8(dev(frames), layout="hwc"))
    frames, rects = redraw(frames, rng, C1)
    before = a.step_u8_regions(dev(frames), rects)
    assert equal_outputs(before, b.step_u8(dev(frames), layout="hwc"))
    with torch.no_grad():
        live.input.weight.mul_(1.5)
        live.conv.weight.mul_(-0.7)
    engine.requantize(live)
    got = a.step_u8_regions(dev(frames), [[(0, 0, h, w)]] * S)
    want = engine.evaluate_logits_u8(dev(frames), layout="hwc")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert equal_outputs(got, b.step_u8(dev(frames), layout="hwc"))
    assert not torch.equal(got[0], before[0])
    frames, rects = redraw(frames, rng, C1)  # and the chain goes on from the new sets
    assert equal_outputs(a.step_u8_regions(dev(frames), rects), b.step_u8(dev(frames), layout="hwc"))


# ---- 8. capture --------------------------------------------------------------------------------------------------------------------
def test_capture(models):
    """step_u8_regions under torch.cuda.graph; frames and rects rewritten in place, replayed, against the eager call."""
    engine, _ = models(C1)
    h, w, S = 32, 20, 3
    rng = np.random.RandomState(89)
    a, eager, b = engine.stream(S), engine.stream(S), engine.stream(S)
    frames = make_store(C1, h, w, seed=97)[:S]
    store = dev(frames)
    rects = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
    for s in (a, eager):
        s.step_u8_regions(store, rects)  # the streams become valid; buffers and the unit offsets exist before the capture
    b.step_u8(store, layout="hwc")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a.step_u8_regions(store, rects)
    seen = []
    for _ in range(3):
        frames, lists = redraw(frames, rng, C1, most=1)
        store.copy_(dev(frames))
        rects.copy_(dev(np.asarray([l[0] for l in lists], dtype=np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        want = eager.step_u8_regions(store, rects)
        assert equal_outputs(out, want)
        assert equal_outputs(out, b.step_u8(store, layout="hwc"))
        assert int(out[2].max()) > 0
        seen.append(out[0].clone())
    assert not torch.equal(seen[0], seen[1]) or not torch.equal(seen[1], seen[2])


# ---- 9. Python errors --------------------------------------------------------------------------------------------------------------
def test_python_errors(models):
    engine, _ = models(C1)
    h, w, S = 32, 20, 3
    store = dev(make_store(C1, h, w)[:S])
    one = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
    stream = engine.stream(S)
    with pytest.raises(ValueError, match="hwc"):
        stream.step_u8_regions(store, one, layout="chw")
    for bad in (one.long(), one.float(), one[:, :3], one[:2], one.cpu(), one.reshape(-1), (one, one), (one, torch.zeros(S, dtype=torch.int32, device="cuda")),
                (one, torch.zeros(S + 1, device="cuda")), (one, torch.zeros(S + 1, dtype=torch.int32)), (one.long(), torch.zeros(S + 1, dtype=torch.int32, device="cuda")),
                [[(0, 0, 1, 1)]] * (S + 1), [[(0, 0, 1)]] * S, [[(0.5, 0, 1, 1)]] * S, None, 7):
        with pytest.raises(ValueError):
            stream.step_u8_regions(store, bad)
    with pytest.raises(TypeError):
        stream.step_u8_regions(store.float(), one)
    with pytest.raises(ValueError):
        stream.step_u8_regions(store[:2], one)
    assert int(stream._valid.sum()) == 0  # no refused call launched
    stream.step_u8_regions(store, one)
    other = dev(make_store(C1, 32, 32)[:S])
    with pytest.raises(ValueError, match="32x32"):
        stream.step_u8_regions(other, one)
    stream.step_u8(other, layout="hwc")  # a whole-frame step moves the stream to the new size
    stream.step_u8_regions(other, one)
    with pytest.raises(ValueError, match="32x20"):
        stream.step_u8_regions(store, one)
    stream.reset()
    stream.step_u8_regions(store, one)
