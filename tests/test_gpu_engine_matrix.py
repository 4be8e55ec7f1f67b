"""The engine's integer inference with its accumulate step on the int8 matrix unit (EngineModel.evaluate_logits(path="matrix"),
EngineModel.evaluate_features, nnue_engine_pack_table, nnue_engine_evaluate_logits_matrix): bit-identical to the real C++ engine's
recorded outputs, to its numpy restatement and to the gather kernels.  Every comparison is exact.  ``-m gpu``."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

import nnue
import nnue_engine_oracle as eo
import serialize
from conftest import GOLDEN
from nnue_hip import lib
from nnue_hip.engine import EngineModel

pytestmark = pytest.mark.gpu

ARCHS = [(10, 8, 1024, 128, 32, 10, 32), (10, 8, 256, 32, 16, 100, 32), (4, 64, 64, 8, 8, 3, 40), (8, 4, 96, 16, 8, 1000, 17),
         (32, 64, 512, 32, 32, 10, 224)]


# ---- models ---------------------------------------------------------------------------------------------------------
def _fresh(tmp_path, arch, threshold=None, buckets=1, nonneg_conv=False, patch_table=None):
    """A model file as test_gpu_engine builds it (table x3 so the int16 sums wrap); patch_table: int16 [F][L1] written over the
    file's table bytes (the serialiser itself clamps to +-127)."""
    g, fps, l1, l2, l3, classes, size = arch
    torch.manual_seed(g * 100 + l1)
    model = nnue.NNUE(nnue.GridFeatureSet(g, fps), l1, l2, l3, num_classes=classes, input_size=size, num_ls_buckets=buckets)
    with torch.no_grad():
        model.input.weight.mul_(3.0)
        model.input.bias.uniform_(-1, 1)
        if threshold is not None:
            model.visual_threshold.fill_(threshold)
        if nonneg_conv:
            model.conv.weight.abs_()
    path = tmp_path / "m.nnue"
    serialize.serialize_model(model, path)
    if patch_table is not None:
        data = bytearray(path.read_bytes())
        oc = struct.unpack_from("<I", data, 4 + 4 + 20 + 12 + 4 + 4)[0]
        off = 4 + 4 + 20 + 12 + 4 + 4 + 16 + oc * 27 + 4 + oc * 4 + 4
        f, cols = struct.unpack_from("<2I", data, off)
        assert (f, cols) == patch_table.shape
        raw = np.ascontiguousarray(patch_table, dtype="<i2").tobytes()
        data[off + 8:off + 8 + len(raw)] = raw
        path.write_bytes(bytes(data))
    return eo.load_nnue(path), path


def _direct(g, oc, l1, l2=8, l3=8, classes=3, seed=0, threshold=0.0, table=None, wmax=20, as_torch=False):
    """An oracle-form model of random integers and the EngineModel constructed straight from its tensors (no file)."""
    rng = np.random.default_rng(seed)
    F = g * g * oc
    ints = lambda lo, hi, shape, dt: rng.integers(lo, hi + 1, size=shape).astype(dt)
    ft_w = ints(-wmax, wmax, (F, l1), np.int16) if table is None else np.ascontiguousarray(table, dtype=np.int16)
    stack = {"l1_scale": 64.0, "l2_scale": 64.0, "out_scale": 16.0, "classes": classes,
             "l1_w": ints(-127, 127, (l2 + 1, l1), np.int8), "l1_b": ints(-500, 500, (l2 + 1,), np.int32),
             "l2_w": ints(-127, 127, (l3, 2 * l2), np.int8), "l2_b": ints(-500, 500, (l3,), np.int32),
             "out_w": ints(-127, 127, (classes, l3), np.int8), "out_b": ints(-500, 500, (classes,), np.int32)}
    ref = {"num_features": F, "l1": l1, "l2": l2, "l3": l3, "buckets": 1, "oc": oc, "grid": g, "threshold": threshold,
           "conv_scale": 64.0, "quantized_one": 127.0, "conv_w": ints(-127, 127, (oc * 27,), np.int8),
           "conv_b": np.zeros((oc,), np.int32), "ft_w": ft_w, "ft_b": ints(-64, 64, (l1,), np.int32), "stacks": [stack]}
    header = {k: ref[k] for k in ("num_features", "l1", "l2", "l3", "grid", "oc", "conv_scale", "threshold", "quantized_one")}
    header.update(classes=classes, buckets=1, l1_scale=64.0, l2_scale=64.0, out_scale=16.0)
    tensors = {"conv_w": ref["conv_w"], "conv_b": ref["conv_b"], "ft_w": ft_w.reshape(-1), "ft_b": ref["ft_b"]}
    tensors.update({k: stack[k].reshape(-1) for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b")})
    if as_torch:
        tensors = {k: torch.from_numpy(v) for k, v in tensors.items()}
    return ref, EngineModel(header, tensors, "cuda")


def _want_features(ref, on_row: np.ndarray):
    ids = np.nonzero(on_row)[0]
    logits = eo.forward_multiclass(ref["stacks"][0], eo.ft_forward(ref, ids), ref["l1"], ref["l2"], ref["l3"])
    return logits, np.float32(ids.size) / np.float32(ref["num_features"])


def _maps(B, F, seed, full_rows=True):
    """bool [B][F]: row 0 all off and row 1 all on (when there are that many), then densities 0.01 and 0.5 in turn."""
    gen = torch.Generator().manual_seed(seed)
    on = torch.zeros(B, F, dtype=torch.bool)
    for b in range(B):
        if b == 0 and B > 1 and full_rows:
            continue
        if b == 1 and full_rows:
            on[b] = True
            continue
        on[b] = torch.rand(F, generator=gen) < (0.01 if b % 2 else 0.5)
    return on


def _as_bytes(on: torch.Tensor, seed) -> torch.Tensor:
    """The map as uint8 with arbitrary non-zero bytes where it is on."""
    gen = torch.Generator().manual_seed(seed)
    return on.to(torch.uint8) * torch.randint(1, 256, tuple(on.shape), generator=gen, dtype=torch.int32).to(torch.uint8)


def _check_features(ref, engine, on: torch.Tensor, active: torch.Tensor, what):
    logits, density = engine.evaluate_features(active.cuda())
    logits, density = logits.cpu().numpy(), density.cpu().numpy()
    for b in range(on.shape[0]):
        want_logits, want_density = _want_features(ref, on[b].numpy())
        assert np.array_equal(logits[b], want_logits), (what, b)
        assert density[b] == want_density, (what, b)
    return logits, density


# ---- 0. the operand maps of the int8 MFMA, seen through a transparent stack ---------------------------------------------
def test_operand_lane_maps_with_asymmetric_integers():
    """Exact asymmetric data through a stack that shows the accumulator itself: with l1/l2/out scales of 1 and identity weights,
    logits[b][o] = clip(acc[b][o], 0, 127) for the first half of the columns; the table rolled by half a row shows the rest.
    Every (row, column, feature) has its own weight pattern, so a transposed or permuted operand map cannot pass."""
    g, oc, l1 = 10, 8, 256
    F, half, B = g * g * oc, l1 // 2, 130
    f, n = np.meshgrid(np.arange(F), np.arange(l1), indexing="ij")
    table = ((f * 5 + n * 3 + (f // 16) * (n // 32)) % 4).astype(np.int16) - ((f * n) % 7 == 0)  # -1 .. 3, no symmetry
    gen = torch.Generator().manual_seed(3)
    on = torch.rand(B, F, generator=gen) < 0.04
    on[0] = False
    seen_inside = 0
    for roll in (0, half):
        tab = np.roll(table, -roll, axis=1)
        ref, _ = _direct(g, oc, l1, l2=half, l3=half, classes=half, table=tab)
        st = ref["stacks"][0]
        st["l1_scale"] = st["l2_scale"] = st["out_scale"] = 1.0
        st["l1_w"] = np.zeros((half + 1, l1), np.int8)
        st["l1_w"][np.arange(half), half + np.arange(half)] = 1  # pair[half + o] = clip(ft[o], 0, 127)
        st["l2_w"] = np.concatenate([np.eye(half, dtype=np.int8), np.zeros((half, half), np.int8)], axis=1)
        st["out_w"] = np.eye(half, dtype=np.int8)
        for k in ("l1_b", "l2_b", "out_b"):
            st[k] = np.zeros_like(st[k])
        ref["ft_b"] = np.zeros((l1,), np.int32)
        header = {k: ref[k] for k in ("num_features", "l1", "l2", "l3", "grid", "oc", "conv_scale", "threshold", "quantized_one")}
        header.update(classes=half, buckets=1, l1_scale=1.0, l2_scale=1.0, out_scale=1.0)
        tensors = {"conv_w": ref["conv_w"], "conv_b": ref["conv_b"], "ft_w": tab.reshape(-1), "ft_b": ref["ft_b"]}
        tensors.update({k: st[k].reshape(-1) for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b")})
        engine = EngineModel(header, tensors, "cuda")
        assert engine.table_planes == 1
        logits, _ = engine.evaluate_features(on.cuda())
        acc = on.numpy().astype(np.int64) @ tab.astype(np.int64)
        want = np.clip(acc[:, :half], 0, 127).astype(np.float32)
        assert np.array_equal(logits.cpu().numpy(), want), roll
        seen_inside += int(((acc[:, :half] > 0) & (acc[:, :half] < 127)).sum())
    assert seen_inside > 0.9 * (B - 1) * l1  # the sums themselves were visible, not their clipped ends


# ---- 1. the reference engine's recorded outputs ------------------------------------------------------------------------
def test_golden_outputs_of_the_reference_engine():
    z = np.load(GOLDEN / "engine_cases.npz")
    index = json.loads(str(z["index"]))
    for k, c in enumerate(index):
        engine = EngineModel.load(GOLDEN / c["model"])
        images = torch.from_numpy(z[f"case{k}/images"]).cuda()
        logits, density = engine.evaluate_logits(images, c["h"], c["w"], path="matrix")
        assert engine._planes is not None
        assert np.array_equal(logits.cpu().numpy().astype(np.float64), z[f"case{k}/logits"]), c
        gather = engine.evaluate_logits(images, c["h"], c["w"], path="gather")
        assert torch.equal(density, gather[1]) and torch.equal(logits, gather[0]), c


# ---- 2. the oracle and the gather path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("threshold", (None, -0.5, 1.0))
def test_fresh_models_against_the_oracle_and_the_gather_path(tmp_path, arch, threshold):
    ref, path = _fresh(tmp_path, arch, threshold)
    size = arch[-1]
    engine = EngineModel.load(path)
    assert engine.table_planes == 1
    gen = torch.Generator().manual_seed(7)
    images = torch.randn(6, 3, size, size, generator=gen) * 1.5
    x = images.cuda()
    logits, density, used = engine.evaluate_logits(x, return_stacks=True, path="matrix")
    for i in range(images.shape[0]):
        want_logits, want_density = eo.evaluate_logits(ref, images[i].numpy().reshape(-1), size, size)
        assert np.array_equal(logits[i].cpu().numpy(), want_logits), (arch, threshold, i)
        assert float(density[i]) == float(want_density), (arch, threshold, i)
    g_logits, g_density, g_used = engine.evaluate_logits(x, return_stacks=True, path="gather")
    assert torch.equal(logits, g_logits) and torch.equal(density, g_density) and torch.equal(used, g_used)


# ---- 3. the edges of the tiling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_oc", [(3, 5), (10, 8), (4, 96)])
@pytest.mark.parametrize("l1", (2, 96, 200, 2048))
def test_tile_edges_through_evaluate_features(grid_oc, l1):
    g, oc = grid_oc
    F = g * g * oc
    assert F in (45, 800, 1536)
    ref, engine = _direct(g, oc, l1, seed=F + l1)
    for B in (1, 5, 33, 130):
        on = _maps(B, F, seed=B)
        active = _as_bytes(on, B) if B % 2 else on
        _check_features(ref, engine, on, active, (F, l1, B))
        if B >= 5:
            assert not on[0].any() and on[1].all()
        if oc > 64:  # ids of channels >= 64 count here: the feature-map rule applies no per-cell mask
            assert (np.nonzero(on.numpy())[1] % oc >= 64).any()


def test_channel_mask_applies_to_images_only():
    """oc = 96: channels >= 64 of a cell are masked on the image path (the engine bit-packs 64 per cell) and count on the
    feature-map path; both occur in these inputs."""
    g, oc, size = 4, 96, 40
    ref, engine = _direct(g, oc, 64, threshold=-0.5, seed=11)
    F = g * g * oc
    gen = torch.Generator().manual_seed(2)
    images = torch.randn(5, 3, size, size, generator=gen) * 1.5
    logits, density = engine.evaluate_logits(images.cuda(), path="matrix")
    masked = 0
    for i in range(images.shape[0]):
        flat_img = images[i].numpy().reshape(-1)
        want_logits, want_density = eo.evaluate_logits(ref, flat_img, size, size)
        assert np.array_equal(logits[i].cpu().numpy(), want_logits), i
        assert float(density[i]) == float(want_density), i
        conv, _ = eo.conv_forward(ref, flat_img, size, size)
        flat = np.zeros(F, np.int8)
        flat[:conv.size] = conv.reshape(-1)
        masked += int((flat.astype(np.float32) > np.float32(-0.5)).reshape(g * g, oc)[:, 64:].sum())
    assert masked > 0
    g_logits, g_density = engine.evaluate_logits(images.cuda(), path="gather")
    assert torch.equal(logits, g_logits) and torch.equal(density, g_density)
    # the same bytes as a feature map: the high channels count
    on = torch.zeros(2, F, dtype=torch.bool)
    on[0, 64:96] = True  # only masked-on-images channels
    on[1] = torch.rand(F, generator=gen) < 0.5
    _, dens = _check_features(ref, engine, on, on, "oc96")
    assert dens[0] == np.float32(32) / np.float32(F)


# ---- 4. wide tables --------------------------------------------------------------------------------------------------------
SPECIAL = (32767, -32768, -129, 128, 255, -256)


def _wide_table(F, l1, seed=5):
    rng = np.random.default_rng(seed)
    table = rng.integers(-32768, 32768, size=(F, l1)).astype(np.int16)
    for j, v in enumerate(SPECIAL):
        table[j, j] = v
    return table


def _assert_wraps_both_ways(ref, on_rows, special=True):
    over = under = 0
    for row in on_rows:
        ids = np.nonzero(row)[0]
        if special:  # the special entries sit in rows that are on
            assert set(range(len(SPECIAL))) <= set(ids.tolist())
        s = ref["ft_b"].astype(np.int64) + ref["ft_w"][ids].astype(np.int64).sum(axis=0)
        over += int((s > 32767).sum())
        under += int((s < -32768).sum())
    assert over > 0 and under > 0


def test_wide_table_two_planes():
    g, oc, l1 = 10, 8, 448
    F = g * g * oc
    table = _wide_table(F, l1)
    ref, engine = _direct(g, oc, l1, table=table)
    assert engine.table_planes == 2
    on = _maps(9, F, seed=4, full_rows=False)
    on[:, :len(SPECIAL)] = True
    _assert_wraps_both_ways(ref, on.numpy())
    _check_features(ref, engine, on, on, "wide")
    # a one-plane pack of this table reports every element that does not fit a byte
    L = lib.load()
    nbytes = int(L.nnue_engine_table_planes_bytes(ctypes.byref(engine._c), 1))
    planes = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    misfit = torch.zeros((1,), dtype=torch.int32, device="cuda")
    lib._call("nnue_engine_pack_table", ctypes.addressof(engine._c), 1, planes.data_ptr(), nbytes, misfit.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    assert int(misfit.item()) == int(((table < -128) | (table > 127)).sum()) > 0
    # a table the host has not seen (device tensors): the preparation finds the second plane out by itself
    _, blind = _direct(g, oc, l1, table=table, as_torch=True)
    assert blind.table_planes is None
    blind.prepare_matrix()
    assert blind.table_planes == 2
    assert torch.equal(blind.evaluate_features(on.cuda())[0], engine.evaluate_features(on.cuda())[0])
    # and one that fits a byte stays at one plane
    _, narrow = _direct(g, oc, l1, as_torch=True)
    narrow.prepare_matrix()
    assert narrow.table_planes == 1


def test_wide_table_through_load(tmp_path):
    arch = (10, 8, 448, 32, 16, 10, 32)
    F, l1 = 800, 448
    table = _wide_table(F, l1)
    ref, path = _fresh(tmp_path, arch, -0.5, patch_table=table)
    assert np.array_equal(ref["ft_w"], table)
    engine = EngineModel.load(path)
    assert engine.table_planes == 2  # decided from the file's table on the host
    gen = torch.Generator().manual_seed(7)
    images = torch.randn(6, 3, 32, 32, generator=gen) * 1.5
    rows = []
    for i in range(6):
        conv, _ = eo.conv_forward(ref, images[i].numpy().reshape(-1), 32, 32)
        row = np.zeros(F, bool)
        row[eo.active_features(ref, conv)] = True
        rows.append(row)
    _assert_wraps_both_ways(ref, rows, special=False)  # which rows an image turns on is the conv's business
    outs = {p: engine.evaluate_logits(images.cuda(), path=p) for p in ("matrix", "auto", "gather")}
    for i in range(6):
        want_logits, want_density = eo.evaluate_logits(ref, images[i].numpy().reshape(-1), 32, 32)
        for p, (logits, density) in outs.items():
            assert np.array_equal(logits[i].cpu().numpy(), want_logits), (p, i)
            assert float(density[i]) == float(want_density), (p, i)


# ---- 5. split-K ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_oc", [(3, 5), (10, 8), (4, 96)])
def test_split_k_gives_the_same_tensor(monkeypatch, grid_oc):
    g, oc = grid_oc
    F = g * g * oc
    ref, engine = _direct(g, oc, 200, seed=F, wmax=127)
    on = _maps(7, F, seed=1)
    on[2] = False
    on[2, :min(F, 30)] = True      # later slabs hold no active feature of this row
    on[3] = False
    on[3, F - 1] = True            # only the ragged last slab does
    monkeypatch.delenv("NNUE_ENGINE_MATRIX_KSPLIT", raising=False)
    base = _check_features(ref, engine, on, on, ("policy", F))
    for ks in (1, 2, 3, 5):
        monkeypatch.setenv("NNUE_ENGINE_MATRIX_KSPLIT", str(ks))
        logits, density = engine.evaluate_features(on.cuda())
        assert np.array_equal(logits.cpu().numpy(), base[0]) and np.array_equal(density.cpu().numpy(), base[1]), (F, ks)


def test_split_k_with_two_planes_and_images(monkeypatch, tmp_path):
    table = _wide_table(800, 448, seed=9)
    ref, path = _fresh(tmp_path, (10, 8, 448, 32, 16, 10, 32), -0.5, patch_table=table)
    engine = EngineModel.load(path)
    images = (torch.randn(5, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 1.5).cuda()
    want = engine.evaluate_logits(images, path="gather")
    for ks in (1, 2, 3, 5):
        monkeypatch.setenv("NNUE_ENGINE_MATRIX_KSPLIT", str(ks))
        got = engine.evaluate_logits(images, path="matrix")
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ks


# ---- 6. layer stacks --------------------------------------------------------------------------------------------------------
def test_layer_stack_selection(tmp_path):
    arch, K, B = (10, 8, 256, 32, 16, 10, 32), 8, 24
    ref, path = _fresh(tmp_path, arch, buckets=K, nonneg_conv=True)
    engine = EngineModel.load(path, bucket="auto")
    assert engine.num_stacks == K
    gen = torch.Generator().manual_seed(7)
    n = 3 * 32 * 32
    rows = []
    for b in range(B):  # dark noise with a bright prefix: the counts spread over the stacks
        flat = torch.randn(n, generator=gen) * 0.3 - 1.5
        flat[:n * b // (B - 1)] += 3.0
        rows.append(flat)
    x = torch.stack(rows).view(B, 3, 32, 32).cuda()
    want = engine.evaluate_logits(x, return_stacks=True, path="gather")
    got = engine.evaluate_logits(x, return_stacks=True, path="matrix")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert len(set(want[2].tolist())) >= 4  # several stacks were really chosen
    for i in (0, B // 2, B - 1):  # and the oracle agrees with the stack used
        want_logits, _ = eo.evaluate_logits(ref, x[i].cpu().numpy().reshape(-1), 32, 32, int(got[2][i]))
        assert np.array_equal(got[0][i].cpu().numpy(), want_logits)
    for dtype in (torch.int32, torch.int64):
        stacks = (torch.arange(B) % (K + 3) - 1).to(dtype)  # -1 and K .. K+1 are out of range: stack 0
        if dtype == torch.int64:
            stacks[3] = 2 ** 32 + 1
        want = engine.evaluate_logits(x, stacks=stacks.cuda(), return_stacks=True, path="gather")
        got = engine.evaluate_logits(x, stacks=stacks.cuda(), return_stacks=True, path="matrix")
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        inside = (stacks >= 0) & (stacks < K)
        assert torch.equal(got[2].cpu().long(), torch.where(inside, stacks.long(), torch.zeros_like(stacks.long())))
    # feature maps: the per-stream kernels apply the same rule to the same maps
    F = ref["num_features"]
    on = _maps(B, F, seed=8)
    on[2:] = torch.rand(B - 2, F, generator=gen) < torch.linspace(0.02, 0.98, B - 2)[:, None]
    stream = engine.stream(B)
    s_logits, s_density, _ = stream.step_features(on.cuda())
    logits, density, used = engine.evaluate_features(on.cuda(), return_stacks=True)
    assert torch.equal(logits, s_logits) and torch.equal(density, s_density) and torch.equal(used, stream.stacks)
    assert len(set(used.tolist())) == K
    stacks = (torch.arange(B) % (K + 2)).to(torch.int32).cuda()
    s_logits, _, _ = stream.step_features(on.cuda(), stacks=stacks)
    logits, _, used = engine.evaluate_features(on.cuda(), stacks=stacks, return_stacks=True)
    assert torch.equal(logits, s_logits) and torch.equal(used, stream.stacks)


# ---- 7. requantize ---------------------------------------------------------------------------------------------------------
def _shift(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        model.input.weight.add_((torch.rand(model.input.weight.shape, generator=gen) - 0.5).to(model.input.weight.device) * 0.5)
        model.input.bias.add_(0.25)


@pytest.mark.parametrize("buckets", (1, 8))
def test_requantize_repacks_the_planes(monkeypatch, buckets):
    torch.manual_seed(3)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10, num_ls_buckets=buckets).cuda()
    with torch.no_grad():
        model.input.weight.mul_(3.0)
    x = (torch.randn(40, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 1.5).cuda()
    engine = EngineModel.from_model(model)
    assert engine.table_planes == 1
    before = engine.evaluate_logits(x, path="matrix")[0].clone()
    planes_ptr = engine._planes.data_ptr()
    _shift(model, 1)
    engine.requantize(model)
    assert engine._planes.data_ptr() == planes_ptr
    after = engine.evaluate_logits(x, path="matrix")
    fresh = EngineModel.from_model(model).evaluate_logits(x, path="gather")
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
    assert not torch.equal(after[0], before)  # stale planes could not have passed

    # a captured matrix call (a linear chain on one stream) stays valid across requantize
    static = x.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            out = engine.evaluate_logits(static, path="matrix")
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], after[0])
    _shift(model, 2)
    engine.requantize(model)
    graph.replay()
    torch.cuda.synchronize()
    fresh = EngineModel.from_model(model).evaluate_logits(x, path="gather")
    assert torch.equal(out[0], fresh[0]) and torch.equal(out[1], fresh[1])
    assert not torch.equal(out[0], after[0])
    # auto inside a capture takes the matrix form only with the planes ready; an engine without them stays on gather
    import nnue_hip.engine as engine_module
    monkeypatch.setattr(engine_module, "_MATRIX_MIN_MAP_BYTES", 1)  # auto would take the matrix form here if it could
    cold = EngineModel.from_model(model)
    with torch.cuda.stream(side):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side, capture_error_mode="thread_local"):
            cold.evaluate_logits(static, path="auto")
    torch.cuda.current_stream().wait_stream(side)
    assert cold._planes is None
    cold.evaluate_logits(static, path="auto")
    assert cold._planes is not None


# ---- 8. errors and the path choice -----------------------------------------------------------------------------------------
def test_errors_and_path_choice(monkeypatch):
    ref, engine = _direct(4, 8, 64)
    F = 128
    on = torch.zeros(3, F, dtype=torch.bool).cuda()
    with pytest.raises(ValueError, match="gather"):
        engine.evaluate_features(on, path="gather")
    with pytest.raises(ValueError, match="path"):
        engine.evaluate_features(on, path="mfma")
    with pytest.raises(ValueError, match="path"):
        engine.evaluate_logits(torch.zeros(1, 3, 32, 32).cuda(), path="dense")
    with pytest.raises(ValueError, match="shape"):
        engine.evaluate_features(torch.zeros(3, F + 1, dtype=torch.bool).cuda())
    with pytest.raises(ValueError, match="shape"):
        engine.evaluate_features(torch.zeros(F, dtype=torch.bool).cuda())
    with pytest.raises(ValueError, match="dtype"):
        engine.evaluate_features(torch.zeros(3, F, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match="CPU"):
        engine.evaluate_features(torch.zeros(3, F, dtype=torch.bool))
    with pytest.raises(TypeError):
        engine.evaluate_features(np.zeros((3, F), bool))
    with pytest.raises(ValueError, match="stacks"):
        engine.evaluate_features(on, stacks=torch.zeros(3, dtype=torch.int32).cuda())  # a single-stack model
    # a model the matrix form cannot run: the tail's LDS (the gather call refuses it as well, with the same code)
    _, fat = _direct(4, 8, 2048, l2=13000, l3=8)
    assert not fat.matrix_supported(3)
    with pytest.raises(lib.NnueHipError, match="matrix"):
        fat.evaluate_logits(torch.zeros(3, 3, 32, 32).cuda(), path="matrix")
    with pytest.raises(lib.NnueHipError, match="matrix"):
        fat.evaluate_features(on)
    with pytest.raises(lib.NnueHipError, match="matrix"):
        fat.prepare_matrix()
    # the environment variable chooses when path is None
    x = torch.randn(3, 3, 32, 32).cuda()
    monkeypatch.setenv("NNUE_ENGINE_PATH", "gather")
    _, cold = _direct(4, 8, 64)
    a = cold.evaluate_logits(x)
    assert cold._planes is None
    monkeypatch.setenv("NNUE_ENGINE_PATH", "matrix")
    b = cold.evaluate_logits(x)
    assert cold._planes is not None
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    monkeypatch.setenv("NNUE_ENGINE_PATH", "simd")
    with pytest.raises(ValueError, match="path"):
        cold.evaluate_logits(x)


def test_224_shape(tmp_path):
    arch = (32, 64, 512, 32, 32, 10, 224)
    _, path = _fresh(tmp_path, arch)
    engine = EngineModel.load(path)
    images = (torch.randn(16, 3, 224, 224, generator=torch.Generator().manual_seed(9)) * 1.5).cuda()
    got = engine.evaluate_logits(images, path="matrix")
    want = engine.evaluate_logits(images, path="gather")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert float(want[1].min()) > 0.05  # thousands of active rows per image
