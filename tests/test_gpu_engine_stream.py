"""Incremental per-stream evaluation of the engine (EngineModel.stream, nnue_engine_stream_step): every step's logits and
density are bit-identical to evaluate_logits on the same frames -- hence to the real C++ engine -- whatever the stream's
history, and `changed` counts the features that differ from the stream's previous set.  ``-m gpu``."""
import json

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


def _fresh(tmp_path, arch, threshold=None, wscale=3.0, seed=None, edit=None):
    g, fps, l1, l2, l3, classes, size = arch
    torch.manual_seed(g * 100 + l1 if seed is None else seed)
    model = nnue.NNUE(nnue.GridFeatureSet(g, fps), l1, l2, l3, num_classes=classes, input_size=size)
    with torch.no_grad():
        model.input.weight.mul_(wscale)  # spread the quantised table; int16 sums then wrap like the engine's
        model.input.bias.uniform_(-1, 1)
        if threshold is not None:
            model.visual_threshold.fill_(threshold)
        if edit is not None:
            edit(model)
    path = tmp_path / "m.nnue"
    serialize.serialize_model(model, path)
    return eo.load_nnue(path), EngineModel.load(path)


def _ids(ref, frame: torch.Tensor, h: int, w: int) -> np.ndarray:
    conv, _ = eo.conv_forward(ref, frame.numpy().reshape(-1), h, w)
    return eo.active_features(ref, conv)


def _patch(frames: torch.Tensor, gen: torch.Generator, p: int) -> torch.Tensor:
    """A copy of frames with one p x p patch per frame re-randomised (at a different place per frame)."""
    out = frames.clone()
    h, w = frames.shape[2], frames.shape[3]
    for i in range(frames.shape[0]):
        y = int(torch.randint(0, h - p + 1, (1,), generator=gen))
        x = int(torch.randint(0, w - p + 1, (1,), generator=gen))
        out[i, :, y:y + p, x:x + p] = torch.randn(3, p, p, generator=gen) * 1.5
    return out


def _step_and_check(ref, engine, stream, frames: torch.Tensor, prev, refreshed=()):
    """One step on the device; logits and density bitwise against evaluate_logits; changed against the oracle's sets.
    Returns (logits, density, changed) on the host and the new sets."""
    h, w = frames.shape[2], frames.shape[3]
    logits, density, changed = stream.step(frames.cuda())
    want_logits, want_density = engine.evaluate_logits(frames.cuda())
    assert torch.equal(logits.cpu(), want_logits.cpu())
    assert torch.equal(density.cpu(), want_density.cpu())
    ids = [_ids(ref, frames[i], h, w) for i in range(frames.shape[0])]
    for i, cur in enumerate(ids):
        want = cur.size if prev is None or i in refreshed else np.setxor1d(prev[i], cur).size
        assert int(changed[i]) == want, (i, int(changed[i]), want)
    return (logits.cpu(), density.cpu(), changed.cpu()), ids


def test_golden_sequence_of_the_reference_engine():
    z = np.load(GOLDEN / "engine_cases.npz")
    index = json.loads(str(z["index"]))
    by_model = {}
    for k, c in enumerate(index):
        by_model.setdefault(c["model"], []).append((k, c))
    for model, cases in by_model.items():
        engine = EngineModel.load(GOLDEN / model)
        stream = engine.stream(1)
        sizes = set()
        for k, c in cases:
            images = torch.from_numpy(z[f"case{k}/images"]).cuda()
            sizes.add((c["h"], c["w"]))
            for i in range(images.shape[0]):
                logits, density, _ = stream.step(images[i:i + 1], c["h"], c["w"])
                assert np.array_equal(logits[0].cpu().numpy().astype(np.float64), z[f"case{k}/logits"][i]), (model, k, i)
                assert abs(float(density[0]) - float(z[f"case{k}/density"][i])) < 5e-10, (model, k, i)
        if model == "nnue_c1arch.nnue":
            assert len(sizes) == 3  # the chain crosses H x W changes


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("threshold", (None, -0.5, 1.0))
def test_equivalence_to_the_batched_engine(tmp_path, arch, threshold):
    size = arch[-1]
    ref, engine = _fresh(tmp_path, arch, threshold)
    gen = torch.Generator().manual_seed(11)
    S, p = 5, max(2, size // 8)
    other = max(8, size * 3 // 4)
    stream = engine.stream(S)
    frames = torch.randn(S, 3, size, size, generator=gen) * 1.5
    (logits, _, _), prev = _step_and_check(ref, engine, stream, frames, None)
    for t in range(1, 12):
        if t == 4:  # identical repeat
            last = logits
            (logits, _, changed), prev = _step_and_check(ref, engine, stream, frames, prev)
            assert torch.equal(logits, last) and int(changed.cpu().abs().max()) == 0
            continue
        if t == 5:  # full jump
            frames = torch.randn(S, 3, size, size, generator=gen) * 1.5
        elif t == 7:  # another H x W mid-sequence
            frames = torch.randn(S, 3, other, other, generator=gen) * 1.5
        elif t == 9:
            frames = torch.randn(S, 3, size, size, generator=gen) * 1.5
        else:
            frames = _patch(frames, gen, p)
        (logits, _, _), prev = _step_and_check(ref, engine, stream, frames, prev)


def test_int16_wrap_is_exercised(tmp_path):
    def same_sign_columns(model):  # every row adds +-64 to these columns: ~1000 active rows leave the int16 range
        model.input.weight[:, :8] = 1.0
        model.input.weight[:, 64:72] = -1.0

    arch = (8, 32, 128, 16, 8, 10, 32)
    ref, engine = _fresh(tmp_path, arch, -0.5, edit=same_sign_columns)
    gen = torch.Generator().manual_seed(3)
    S = 4
    stream = engine.stream(S)
    frames = torch.randn(S, 3, 32, 32, generator=gen) * 1.5
    wrapped, prev = False, None
    for _ in range(6):
        (logits, _, _), ids = _step_and_check(ref, engine, stream, frames, prev)
        for i in range(S):
            raw = ref["ft_b"].astype(np.int64) + ref["ft_w"][ids[i]].astype(np.int64).sum(axis=0)
            wrapped |= bool((raw > 32767).any() or (raw < -32768).any())
            want, _ = eo.evaluate_logits(ref, frames[i].numpy().reshape(-1), 32, 32)
            assert np.array_equal(logits[i].numpy(), want)
        prev = ids
        frames = _patch(frames, gen, 6)
    assert wrapped  # some column's int32 sum left the int16 range: the stored accumulator wrapped


def test_reset_independence_and_repeats(tmp_path):
    arch = (10, 8, 256, 32, 16, 100, 32)
    ref, engine = _fresh(tmp_path, arch, -0.5)
    gen = torch.Generator().manual_seed(21)
    S = 4
    seq = [torch.randn(S, 3, 32, 32, generator=gen) * 1.5]
    for _ in range(5):
        seq.append(_patch(seq[-1], gen, 4))
    perm = [2, 0, 3, 1]
    a, b = engine.stream(S), engine.stream(S)
    prev = None
    for t, frames in enumerate(seq):
        refreshed = ()
        if t == 3:  # stream 2 of a, and the same sequence's place in b
            a.reset([2])
            b.reset([perm.index(2)])
            refreshed = (2,)
        out_a, prev = _step_and_check(ref, engine, a, frames, prev, refreshed)
        if t == 3:
            assert int(out_a[2][2]) == prev[2].size
        out_b = [x.cpu() for x in b.step(frames[perm].cuda())]
        for xa, xb in zip(out_a, out_b):  # permuting the streams permutes every output
            assert torch.equal(xb, xa[perm]), t
    last = out_a[0]
    # a repeated frame: nothing changed, same logits
    logits, _, changed = a.step(seq[-1].cuda())
    assert torch.equal(logits.cpu(), last) and int(changed.cpu().abs().max()) == 0
    # reset of every stream: the next step refreshes all of them, with the same bits
    a.reset()
    logits, _, changed = a.step(seq[-1].cuda())
    assert torch.equal(logits.cpu(), last)
    assert [int(v) for v in changed.cpu()] == [ids.size for ids in prev]


@pytest.mark.parametrize("arch", [(10, 8, 256, 32, 16, 10, 32), (4, 96, 64, 8, 8, 3, 40)])
def test_step_features_against_the_oracle(tmp_path, arch):
    ref, engine = _fresh(tmp_path, arch, -0.5)
    F = ref["num_features"]
    stack = ref["stacks"][0]
    gen = torch.Generator().manual_seed(5)
    S = 3
    stream = engine.stream(S)
    prev = None
    for t, p in enumerate((0.0, 0.01, 0.5, 1.0, 0.5, 0.01, 0.5)):
        on = torch.rand(S, F, generator=gen) < p
        if t % 2:  # uint8 map, any non-zero byte is on
            active = (on.to(torch.uint8) * torch.randint(1, 256, (S, F), generator=gen, dtype=torch.int32).to(torch.uint8))
        else:
            active = on
        logits, density, changed = stream.step_features(active.cuda())
        ids = [np.nonzero(on[i].numpy())[0] for i in range(S)]
        for i in range(S):
            want = eo.forward_multiclass(stack, eo.ft_forward(ref, ids[i]), ref["l1"], ref["l2"], ref["l3"])
            assert np.array_equal(logits[i].cpu().numpy(), want), (arch, p, i)
            assert float(density[i]) == float(np.float32(ids[i].size) / np.float32(F))
            assert int(changed[i]) == (ids[i].size if prev is None else np.setxor1d(prev[i], ids[i]).size)
        prev = ids
    if arch[1] > 64:  # channels >= 64 of a cell count here: the feature-map entry applies no per-cell mask
        assert any(((ids[i] % arch[1]) >= 64).any() for i in range(S))
    # mixed with image steps on the same streams
    frames = torch.randn(S, 3, arch[-1], arch[-1], generator=gen) * 1.5
    logits, density, changed = stream.step(frames.cuda())
    want_logits, want_density = engine.evaluate_logits(frames.cuda())
    assert torch.equal(logits.cpu(), want_logits.cpu()) and torch.equal(density.cpu(), want_density.cpu())
    img_ids = [_ids(ref, frames[i], arch[-1], arch[-1]) for i in range(S)]
    assert [int(v) for v in changed.cpu()] == [np.setxor1d(prev[i], img_ids[i]).size for i in range(S)]
    on = torch.rand(S, F, generator=gen) < 0.3
    logits, _, changed = stream.step_features(on.cuda())
    for i in range(S):
        ids = np.nonzero(on[i].numpy())[0]
        want = eo.forward_multiclass(stack, eo.ft_forward(ref, ids), ref["l1"], ref["l2"], ref["l3"])
        assert np.array_equal(logits[i].cpu().numpy(), want)
        assert int(changed[i]) == np.setxor1d(img_ids[i], ids).size


def test_224_shape(tmp_path):
    arch = (32, 64, 512, 32, 32, 10, 224)
    ref, engine = _fresh(tmp_path, arch)
    gen = torch.Generator().manual_seed(9)
    S = 16
    stream = engine.stream(S)
    frames = torch.randn(S, 3, 224, 224, generator=gen) * 1.5
    for t in range(4):
        logits, density, changed = stream.step(frames.cuda())
        want_logits, want_density = engine.evaluate_logits(frames.cuda())
        assert torch.equal(logits.cpu(), want_logits.cpu()) and torch.equal(density.cpu(), want_density.cpu()), t
        frames = _patch(frames, gen, 16) if t < 2 else torch.randn(S, 3, 224, 224, generator=gen) * 1.5


def test_stream_errors():
    engine = EngineModel.load(GOLDEN / "nnue_tiny4x4.nnue")
    F = int(engine.header["num_features"])
    stream = engine.stream(3)
    with pytest.raises(ValueError):
        engine.stream(0)
    with pytest.raises(ValueError):
        stream.step(torch.zeros(4, 3, 32, 32).cuda())  # wrong S
    with pytest.raises(ValueError):
        stream.step_features(torch.zeros(2, F, dtype=torch.bool).cuda())  # wrong S
    with pytest.raises(ValueError):
        stream.step_features(torch.zeros(3, F + 1, dtype=torch.bool).cuda())  # wrong F
    with pytest.raises(ValueError):
        stream.step(torch.zeros(3, 3, 32, 32, dtype=torch.float64).cuda())  # wrong dtype
    with pytest.raises(ValueError):
        stream.step_features(torch.zeros(3, F, dtype=torch.int32).cuda())  # wrong dtype
    with pytest.raises(ValueError):
        stream.step(torch.zeros(3, 3, 32, 32))  # CPU tensor
    with pytest.raises(ValueError):
        stream.step_features(torch.zeros(3, F, dtype=torch.bool))  # CPU tensor
    with pytest.raises(ValueError):
        stream.reset([3])
    with pytest.raises(lib.NnueHipError, match="overruns"):
        stream.step(torch.zeros(3, 3, 8, 40).cuda())
    # a rejected call changed nothing: the first real step is still a refresh of every stream
    _, _, changed = stream.step(torch.zeros(3, 3, 32, 32).cuda())
    want = eo.active_features(eo.load_nnue(GOLDEN / "nnue_tiny4x4.nnue"),
                              eo.conv_forward(eo.load_nnue(GOLDEN / "nnue_tiny4x4.nnue"), np.zeros(3 * 32 * 32, np.float32), 32, 32)[0])
    assert [int(v) for v in changed.cpu()] == [want.size] * 3
