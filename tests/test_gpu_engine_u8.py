"""The engine's uint8 input form (EngineModel.evaluate_logits_u8, EngineStream.step_u8) at the smallest shapes where its conv
front can go wrong, against three independent witnesses:

1. the CPU oracle (oracle/nnue_engine_oracle.py) on numpy float32 buffers built from the DEFINITION of the two layouts,
       chw  x[i] = norm(u[(i mod HW)*3 + i div HW], i div HW)      hwc  x[i] = norm(u[i], i mod 3)
       norm(v, c) = ((float32)v - mean255[c]) * inv_std255[c]
   -- logits equal as float32 bits, density equal, on the gather and the matrix form;
2. the float call on lib.load_batch of the same indices (layout chw, default constants): bit for bit;
3. outputs RECORDED from the real C++ engine (tests/golden/engine_u8.npz, written by tests/golden/make_golden_engine_u8.py).
Frame sizes of 1683, 561, 1134, 288, 120 ... bytes put every frame after the first at a base that is no multiple of 4 or 16;
H = 32, 10 and 17 put a CHW plane boundary inside a flat row, H = 33 does not.  Every index handed over lies inside the store.
``-m gpu``."""
import json

import numpy as np
import pytest
import torch

import nnue_engine_oracle as orc
from conftest import GOLDEN
from nnue_hip import lib
from nnue_hip.engine import EngineModel, stack_of, u8_constants

pytestmark = pytest.mark.gpu

K4 = "nnue_k4.nnue"
BIG = "big224"
# (model, H, W)
CASES = [("nnue_c1arch.nnue", 32, 32), ("nnue_c1arch.nnue", 32, 20), ("nnue_c1arch.nnue", 33, 17), ("nnue_c1arch.nnue", 10, 4),
         ("nnue_c1arch.nnue", 96, 100), ("nnue_c1arch.nnue", 32, 3), ("nnue_tiny4x4.nnue", 17, 11), ("nnue_grid8.nnue", 32, 32),
         ("nnue_saturated.nnue", 32, 32), ("nnue_wide96.nnue", 40, 40), ("nnue_wide96.nnue", 40, 1), ("nnue_wide70.nnue", 27, 14),
         (K4, 17, 17), (K4, 17, 22), (BIG, 224, 224), (BIG, 224, 200)]
IDS = [f"{m.replace('nnue_', '').replace('.nnue', '')}-{h}x{w}" for m, h, w in CASES]
PICK = [6, 0, 3, 3, 1]  # repeats, unordered
LAYOUTS = ("chw", "hwc")
PATHS = ("gather", "matrix")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """name -> (EngineModel, the oracle's parse of the same file), loaded once.  nnue_k4 with bucket="auto"; the large-grid
    model (stride 8, 64 channels, bands that do not divide OH, OW < g) is built here and serialised for the oracle."""
    import nnue
    made = {}

    def get(name):
        if name not in made:
            if name == BIG:
                torch.manual_seed(224)
                model = nnue.NNUE(nnue.GridFeatureSet(32, 64), 32, 8, 8, num_classes=3, input_size=224).cuda()
                path = tmp_path_factory.mktemp("u8") / "big224.nnue"
                import serialize
                serialize.serialize_model(model, path)
                engine = EngineModel.from_model(model)
            else:
                path = GOLDEN / name
                engine = EngineModel.load(path, bucket="auto" if name == K4 else 0)
            made[name] = (engine, orc.load_nnue(path))
        return made[name]

    return get


def make_store(name, h, w, seed=7):
    """[9, H, W, 3] uint8: seven frames of uniform bytes (for nnue_k4: three brightness classes), one all 0, one all 255."""
    rng = np.random.RandomState(seed + 131 * h + w)
    if name == K4:
        ranges = [(0, 40), (0, 256), (200, 256), (0, 40), (0, 256), (200, 256), (0, 256)]
    else:
        ranges = [(0, 256)] * 7
    frames = [rng.randint(lo, hi, size=(h, w, 3)).astype(np.uint8) for lo, hi in ranges]
    frames += [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)]
    return np.stack(frames)


def floats_of(frames: np.ndarray, layout: str, mean=None, std=None) -> np.ndarray:
    """[n, H, W, 3] uint8 -> [n, 3*H*W] float32 by the definition; the constants formed as the host forms them."""
    n, h, w, _ = frames.shape
    hw = h * w
    u = frames.reshape(n, 3 * hw)
    i = np.arange(3 * hw)
    mean255, inv_std255 = u8_constants(mean, std)
    assert mean255.dtype == np.float32 and inv_std255.dtype == np.float32
    src, ch = ((i % hw) * 3 + i // hw, i // hw) if layout == "chw" else (i, i % 3)
    return ((u[:, src].astype(np.float32) - mean255[ch][None, :]) * inv_std255[ch][None, :]).astype(np.float32)


def oracle_rows(m, x, h, w, auto):
    """(logits [n, C] float32, density [n] float32, stacks [n]) of the oracle, the stack by `stack_of` on its own counts."""
    logits, density, stacks = [], [], []
    for row in x:
        conv, _ = orc.conv_forward(m, row, h, w)
        count = int(orc.active_features(m, conv).size)
        k = int(stack_of(torch.tensor([count]), m["buckets"], m["num_features"])[0]) if auto else 0
        lg, dn = orc.evaluate_logits(m, row, h, w, k)
        logits.append(lg)
        density.append(dn)
        stacks.append(k)
    return np.stack(logits).astype(np.float32), np.asarray(density, dtype=np.float32), stacks


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    g = got.cpu().numpy()
    return g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("name,h,w", CASES, ids=IDS)
def test_against_the_oracle_and_the_float_call(models, name, h, w):
    engine, m = models(name)
    auto = name == K4
    frames = make_store(name, h, w)
    if name == BIG:
        frames = frames[[0, 8]]  # batch 2: a uniform frame and the all-255 frame
    n = len(frames)
    store = torch.from_numpy(frames).cuda()
    labels = torch.zeros(n, dtype=torch.int64, device="cuda")
    pick = [1, 0] if name == BIG else PICK
    idx = torch.tensor(pick, device="cuda")
    assert engine.matrix_supported(n)
    ref = {layout: oracle_rows(m, floats_of(frames, layout), h, w, auto) for layout in LAYOUTS}
    if name != BIG:  # the witness can tell the layouts apart on every uniform frame's density or logits taken together
        assert not np.array_equal(ref["chw"][0][:7], ref["hwc"][0][:7])
    for layout in LAYOUTS:
        want_logits, want_density, want_stacks = ref[layout]
        for path in PATHS:
            # 1. the oracle: all frames in order, picked frames, and the store as a view one frame into its storage
            logits, density, used = engine.evaluate_logits_u8(store, layout=layout, path=path, return_stacks=True)
            assert same_bits(logits, want_logits) and same_bits(density, want_density), (layout, path)
            assert [int(k) for k in used] == want_stacks, (layout, path)
            logits, density = engine.evaluate_logits_u8(store, idx, layout=layout, path=path)
            assert same_bits(logits, want_logits[pick]) and same_bits(density, want_density[pick]), (layout, path, "indices")
            logits, density = engine.evaluate_logits_u8(store[1:], layout=layout, path=path)
            assert same_bits(logits, want_logits[1:]) and same_bits(density, want_density[1:]), (layout, path, "view")
            if name != BIG:
                logits, density = engine.evaluate_logits_u8(store[1:], idx - 1 + (idx == 0), layout=layout, path=path)
                shifted = [p if p else 1 for p in pick]
                assert same_bits(logits, want_logits[shifted]) and same_bits(density, want_density[shifted]), (layout, path)
    # 2. the parent's path: layout chw with the defaults is the float call on load_batch of the same indices
    for ix in (idx, torch.arange(n, device="cuda")):
        x, _ = lib.load_batch(store, labels, ix, False, 0, 0)
        for path in PATHS:
            want = engine.evaluate_logits(x, path=path, return_stacks=True)
            got = engine.evaluate_logits_u8(store, ix, path=path, return_stacks=True)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), path
            if auto:
                given = torch.tensor([(3 * i) % 5 - 1 for i in range(ix.numel())], device="cuda")  # -1 and 4 mean stack 0
                want = engine.evaluate_logits(x, path=path, stacks=given, return_stacks=True)
                got = engine.evaluate_logits_u8(store, ix, path=path, stacks=given, return_stacks=True)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), (path, "stacks=")


def test_k4_brightness_classes_name_three_stacks(models):
    """Over the model's two sizes together the three brightness classes name at least three of the four stacks by the oracle's
    rule (dark frames land on stack 1 at 17 x 17 and on stack 0 at 17 x 22), and the engine uses exactly those."""
    engine, m = models(K4)
    for layout in LAYOUTS:
        named = set()
        for h, w in ((17, 17), (17, 22)):
            frames = make_store(K4, h, w)
            _, _, want = oracle_rows(m, floats_of(frames, layout), h, w, True)
            _, _, used = engine.evaluate_logits_u8(torch.from_numpy(frames).cuda(), layout=layout, return_stacks=True)
            assert [int(k) for k in used] == want
            named |= set(want)
        assert len(named) >= 3, (layout, named)


@pytest.mark.parametrize("name,h,w", [("nnue_c1arch.nnue", 32, 20), ("nnue_wide70.nnue", 27, 14), (K4, 17, 17)])
def test_custom_constants(models, name, h, w):
    """mean = std = 0.5 on every channel, formed in float32 the way the host forms them."""
    engine, m = models(name)
    frames = make_store(name, h, w)
    store = torch.from_numpy(frames).cuda()
    half = (0.5, 0.5, 0.5)
    for layout in LAYOUTS:
        want_logits, want_density, want_stacks = oracle_rows(m, floats_of(frames, layout, half, half), h, w, name == K4)
        for path in PATHS:
            logits, density, used = engine.evaluate_logits_u8(store, layout=layout, mean=half, std=half, path=path, return_stacks=True)
            assert same_bits(logits, want_logits) and same_bits(density, want_density), (layout, path)
            assert [int(k) for k in used] == want_stacks
    assert not torch.equal(engine.evaluate_logits_u8(store)[0], engine.evaluate_logits_u8(store, mean=half, std=half)[0])


@pytest.fixture(scope="module")
def record():
    z = np.load(GOLDEN / "engine_u8.npz")
    cases = json.loads(str(z["index"]))
    assert len(cases) == 11 and sum(c["count"] for c in cases) == 34
    return z, cases


def test_against_the_recorded_engine(record, models):
    """Logits bit-equal to the values the C++ engine printed, density within the record's ten decimals (5e-10), as
    tests/test_gpu_engine_recorded_shapes.py compares engine_shapes.npz; the stack of nnue_k4 by the rule on the RECORDED ids."""
    z, cases = record
    for k, c in enumerate(cases):
        engine, _ = models(c["model"])
        store = torch.from_numpy(z[f"case{k}/frames"]).cuda()
        assert tuple(store.shape) == (c["count"], c["h"], c["w"], 3)
        for layout in LAYOUTS:
            want, dens = z[f"case{k}/{layout}/logits"], z[f"case{k}/{layout}/density"]
            off = z[f"case{k}/{layout}/ids_offsets"]
            counts = torch.from_numpy(np.diff(off))
            rule = [int(s) for s in stack_of(counts, len(c["stacks"]), int(engine.header["num_features"]))] \
                if len(c["stacks"]) > 1 else [0] * c["count"]
            want = np.stack([want[i, s] for i, s in enumerate(rule)])
            for path in PATHS:
                logits, density, used = engine.evaluate_logits_u8(store, layout=layout, path=path, return_stacks=True)
                assert np.array_equal(logits.cpu().numpy().astype(np.float64), want), (c, layout, path)
                assert float(np.abs(density.cpu().numpy().astype(np.float64) - dens).max()) < 5e-10, (c, layout, path)
                assert [int(s) for s in used] == rule, (c, layout, path)
            if len(c["stacks"]) > 1:  # and every recorded stack, handed over by the caller
                for s in c["stacks"]:
                    given = torch.full((c["count"],), s, device="cuda")
                    logits, _ = engine.evaluate_logits_u8(store, layout=layout, stacks=given, path="gather")
                    assert np.array_equal(logits.cpu().numpy().astype(np.float64), z[f"case{k}/{layout}/logits"][:, s]), (c, layout, s)
    chosen = set()
    for k, c in enumerate(cases):
        if c["model"] == K4:
            chosen |= {int(s) for s in stack_of(torch.from_numpy(np.diff(z[f"case{k}/chw/ids_offsets"])), 4, 256)}
    assert len(chosen) >= 3


def patched(frames: np.ndarray, rng) -> np.ndarray:
    """Every frame with a random 4 x 4 patch of bytes redrawn."""
    out = frames.copy()
    _, h, w, _ = out.shape
    for f in out:
        y, x = rng.randint(0, h - 3), rng.randint(0, w - 3)
        f[y:y + 4, x:x + 4] = rng.randint(0, 256, size=(4, 4, 3))
    return out


@pytest.mark.parametrize("name", ["nnue_c1arch.nnue", K4])
@pytest.mark.parametrize("requantized", [False, True], ids=["loaded", "requantized"])
def test_stream(models, name, requantized):
    """S = 3; four step_u8 calls with, in the middle, one step through `step` on the float frames and one `update`; frame t+1
    is frame t with a random 4 x 4 patch redrawn, and at the fourth frame the size changes.  Every step_u8 is bitwise
    evaluate_logits_u8 on the same frames and its `changed` that of a second stream fed the float frames (and the same
    update).  requantized: the engine comes from a live model of the same architecture and is requantised mid-chain."""
    import nnue
    rng = np.random.RandomState(11)
    auto = name == K4
    live = None
    if requantized:
        torch.manual_seed(5)
        g, fps, size, k = (8, 4, 17, 4) if auto else (10, 8, 32, 1)
        live = nnue.NNUE(nnue.GridFeatureSet(g, fps), 32, 8, 8, num_classes=5, input_size=size, num_ls_buckets=k).cuda()
        with torch.no_grad():
            live.visual_threshold.fill_(-0.5)
        engine = EngineModel.from_model(live)
    else:
        engine, _ = models(name)
    sizes = [(17, 17)] * 3 + [(17, 22)] * 2 if auto else [(32, 32)] * 3 + [(32, 20)] * 2
    S = 3
    a, b = engine.stream(S), engine.stream(S)  # a: the chain under test; b: fed the float frames throughout
    labels = torch.zeros(S, dtype=torch.int64, device="cuda")
    order = torch.arange(S, device="cuda")
    # the update in the middle: stream s turns features 5 and 6 + s on and feature 0 off, on both streams alike
    added = (torch.tensor([5, 6, 5, 7, 5, 8], dtype=torch.int32, device="cuda"), torch.tensor([0, 2, 4, 6], dtype=torch.int32, device="cuda"))
    removed = (torch.zeros(S, dtype=torch.int32, device="cuda"), torch.arange(S + 1, dtype=torch.int32, device="cuda"))
    frames, u8_steps = None, 0
    for t, (h, w) in enumerate(sizes):
        if frames is None or frames.shape[1:3] != (h, w):
            frames = make_store(name, h, w, seed=23)[:S]
        else:
            frames = patched(frames, rng)
        store = torch.from_numpy(frames).cuda()
        x, _ = lib.load_batch(store, labels, order, False, 0, 0)
        if t == 2:
            if requantized:
                with torch.no_grad():
                    live.input.weight.mul_(1.5)
                engine.requantize(live)
            got, ref = a.update(added, removed), b.update(added, removed)
            assert all(torch.equal(p, q) for p, q in zip(got, ref))
        want = engine.evaluate_logits_u8(store, return_stacks=True)
        ref_logits, ref_density, ref_changed = b.step(x)
        if t == 1:  # through the float frames
            logits, density, changed = a.step(x)
        else:
            logits, density, changed = a.step_u8(store)
            u8_steps += 1
        assert torch.equal(logits, want[0]) and torch.equal(density, want[1]), t
        assert torch.equal(logits, ref_logits) and torch.equal(density, ref_density) and torch.equal(changed, ref_changed), t
        if t > 0:
            assert int(changed.max()) > 0  # the patch, the update or the new size moved something
        if engine.num_stacks > 1:
            assert torch.equal(a.stacks, want[2]) and torch.equal(a.stacks, b.stacks), t
    assert u8_steps == 4
    # with indices and the other layout: stream s takes frame indices[s] of a larger store
    h, w = sizes[-1]
    big = torch.from_numpy(make_store(name, h, w, seed=29)).cuda()
    idx = torch.tensor([8, 2, 2], device="cuda")
    logits, density, _ = a.step_u8(big, idx, layout="hwc")
    want = engine.evaluate_logits_u8(big, idx, layout="hwc")
    assert torch.equal(logits, want[0]) and torch.equal(density, want[1])


@pytest.mark.parametrize("path", PATHS)
def test_capture(models, path):
    """evaluate_logits_u8(store, idx) under torch.cuda.graph; store and idx rewritten in place, replayed, against the eager call."""
    engine, _ = models("nnue_c1arch.nnue")
    h, w = 32, 20
    store = torch.from_numpy(make_store("nnue_c1arch.nnue", h, w)).cuda()
    idx = torch.tensor(PICK, device="cuda")
    engine.prepare_matrix()
    engine.evaluate_logits_u8(store, idx, path=path)  # buffers sized before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits, density = engine.evaluate_logits_u8(store, idx, path=path)
    graph.replay()
    torch.cuda.synchronize()
    want = engine.evaluate_logits_u8(store, idx, path=path)
    assert torch.equal(logits, want[0]) and torch.equal(density, want[1])
    store.copy_(torch.from_numpy(make_store("nnue_c1arch.nnue", h, w, seed=99)).cuda())
    idx.copy_(torch.tensor([0, 8, 7, 2, 2], device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    fresh = engine.evaluate_logits_u8(store, idx, path=path)
    assert torch.equal(logits, fresh[0]) and torch.equal(density, fresh[1])
    assert not torch.equal(fresh[0], want[0])


def test_python_errors(models):
    engine, _ = models("nnue_c1arch.nnue")
    store = torch.from_numpy(make_store("nnue_c1arch.nnue", 32, 20)).cuda()
    stream = engine.stream(9)
    for call in (engine.evaluate_logits_u8, stream.step_u8):
        with pytest.raises(TypeError):
            call(store.float())
        with pytest.raises(TypeError):
            call(store.cpu().numpy())
        with pytest.raises(ValueError):
            call(store.cpu())
        with pytest.raises(ValueError):
            call(store.permute(0, 3, 1, 2).contiguous())  # [N,3,H,W]
        with pytest.raises(ValueError):
            call(store[:, :, ::2])  # not contiguous
        with pytest.raises(ValueError):
            call(store.permute(0, 2, 1, 3))
        with pytest.raises(ValueError):
            call(store, layout="nchw")
        with pytest.raises(ValueError):
            call(store, std=(0.2, 0.0, 0.2))
        with pytest.raises(ValueError):
            call(store, mean=(0.2, 0.2))
        with pytest.raises(TypeError):
            call(store, torch.arange(9, device="cuda", dtype=torch.int32))
        with pytest.raises(ValueError):
            call(store, torch.arange(9))  # indices on the CPU
    with pytest.raises(ValueError):
        stream.step_u8(store[:4])  # four frames for nine streams
    with pytest.raises(ValueError):
        stream.step_u8(store, torch.tensor([0, 1], device="cuda"))
    with pytest.raises(ValueError):
        engine.evaluate_logits_u8(store, path="fast")
    with pytest.raises(ValueError):
        engine.evaluate_logits_u8(store, stacks=torch.zeros(9, dtype=torch.int32, device="cuda"))  # a single-stack model
    with pytest.raises(lib.NnueHipError):  # constants that leave int32 under the model's conv_scale are refused by the library
        engine.evaluate_logits_u8(store, std=(1e-12, 1.0, 1.0))
