"""Per-image layer-stack selection in the engine's integer inference (EngineModel.load(bucket="auto"),
nnue_engine_evaluate_logits_stacks, nnue_engine_stream_step_stacks): bit-identical to the engine oracle with the stack the
rule -- or the caller -- picks, for whole batches and for the incremental per-stream form.  ``-m gpu``.
The oracle's own `bucket` argument is held to the real C++ engine at indices 0..4 of a K = 4 file by
tests/golden/engine_shapes.npz (tests/test_engine_oracle.py), and test_gpu_engine_recorded_shapes.py holds the same entry points
to that record directly; what rests on the oracle alone here are the other stack counts (K = 2, 3, 8, 64) and shapes.

Models are built as test_gpu_engine.test_fresh_models_against_the_oracle builds them (table x3 so the int16 sums wrap, uniform
bias) with K layer stacks and a non-negative conv, so that a bright region turns every channel on and a dark one every channel
off; image b of B is dark noise with its first 3*H*W*b // (B-1) floats bright, which spreads the active-feature counts from
none to all the engine's map can reach."""
import numpy as np
import pytest
import torch

import nnue
import nnue_engine_oracle as eo
import serialize
from nnue_hip.engine import EngineFormatError, EngineModel, stack_of

pytestmark = pytest.mark.gpu

# (g, fps, l1, l2, l3, classes, size), K, B, stacks the oracle's counts select at least
CASES = {
    "10x10x8": ((10, 8, 256, 32, 16, 10, 32), 8, 24, {0, 1, 2, 3, 4, 5}),  # the 8x8 map fills at most 512 of 800 ids
    "4x4x64": ((4, 64, 64, 8, 8, 3, 40), 4, 12, {0, 1, 2, 3}),
    "8x8x4": ((8, 4, 96, 16, 8, 100, 17), 3, 12, {0, 1}),
}


def make_model(arch, K):
    g, fps, l1, l2, l3, classes, size = arch
    torch.manual_seed(g * 100 + l1)
    model = nnue.NNUE(nnue.GridFeatureSet(g, fps), l1, l2, l3, num_classes=classes, input_size=size, num_ls_buckets=K)
    with torch.no_grad():
        model.input.weight.mul_(3.0)
        model.input.bias.uniform_(-1, 1)
        model.conv.weight.abs_()
    return model


def make_images(B, size, seed=7):
    gen = torch.Generator().manual_seed(seed)
    n = 3 * size * size
    rows = []
    for b in range(B):
        flat = torch.randn(n, generator=gen) * 0.3 - 1.5
        flat[:n * b // max(1, B - 1)] += 3.0
        rows.append(flat)
    return torch.stack(rows).view(B, 3, size, size)


def rule(n, K, F):
    return min(K - 1, int(n) * K // (F + 1))


class Case:
    """One model file, its oracle form, its images and the oracle's answers (computed once, never modified)."""

    def __init__(self, tmp, arch, K, B):
        self.arch, self.K, self.B, self.size = arch, K, B, arch[-1]
        self.model = make_model(arch, K)
        self.path = tmp / "m.nnue"
        serialize.serialize_model(self.model, self.path)
        self.ref = eo.load_nnue(self.path)
        assert self.ref["buckets"] == K
        self.F = self.ref["num_features"]
        self.images = make_images(B, self.size)
        self._memo = {}
        self.counts = [eo.active_features(self.ref, eo.conv_forward(self.ref, self.flat(i), self.size, self.size)[0]).size
                       for i in range(B)]
        self.stacks = [rule(n, K, self.F) for n in self.counts]

    def flat(self, i):
        return self.images[i].numpy().reshape(-1)

    def oracle(self, i, bucket):
        if (i, bucket) not in self._memo:
            self._memo[i, bucket] = eo.evaluate_logits(self.ref, self.flat(i), self.size, self.size, bucket)
        return self._memo[i, bucket]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            arch, K, B, _ = CASES[name]
            made[name] = Case(tmp_path_factory.mktemp(name), arch, K, B)
        return made[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_batched_by_the_rule(cases, name):
    c = cases(name)
    engine = EngineModel.load(c.path, bucket="auto")
    assert engine.num_stacks == c.K
    logits, density, stack = engine.evaluate_logits(c.images.cuda(), return_stacks=True)
    assert stack.dtype == torch.int32 and tuple(stack.shape) == (c.B,)
    two = engine.evaluate_logits(c.images.cuda())
    assert len(two) == 2 and torch.equal(two[0], logits) and torch.equal(two[1], density)
    plain, _ = EngineModel.load(c.path).evaluate_logits(c.images.cuda())
    logits, density, stack, plain = logits.cpu().numpy(), density.cpu().numpy(), stack.cpu().numpy(), plain.cpu().numpy()
    for i in range(c.B):
        k = int(stack[i])
        assert k == rule(round(float(density[i]) * c.F), c.K, c.F) == c.stacks[i], (name, i, k, c.counts[i])
        want_logits, want_density = c.oracle(i, k)
        assert np.array_equal(logits[i], want_logits), (name, i, k)
        assert float(density[i]) == float(want_density), (name, i)
        if k != 0:  # the image went through another network than the single-stack call's
            assert not np.array_equal(want_logits, c.oracle(i, 0)[0]), (name, i)
            assert not np.array_equal(logits[i], plain[i]), (name, i)
        else:
            assert np.array_equal(logits[i], plain[i]), (name, i)
    assert set(int(k) for k in stack) >= CASES[name][3], (name, sorted(set(int(k) for k in stack)), c.counts)
    assert torch.equal(stack_of(torch.tensor(c.counts), c.K, c.F), torch.from_numpy(stack).long())


def test_boundary_counts_of_the_4x4x64_images(cases):
    c = cases("4x4x64")  # stack 1 ends at 512 of 1024 active ids, stack 2 begins at 513
    assert min(c.counts) == 0 and max(c.counts) == 1024 and {511, 512, 514} <= set(c.counts), c.counts


@pytest.mark.parametrize("name", list(CASES))
def test_batched_given_stacks(cases, name):
    c = cases(name)
    engine = EngineModel.load(c.path, bucket="auto")
    gen = torch.Generator().manual_seed(13)
    given = torch.randint(-2, c.K + 2, (c.B,), generator=gen)
    given[:4] = torch.tensor([-2, -1, c.K, c.K + 1])  # both sides out of range are always present
    x = c.images.cuda()
    for dtype in (torch.int64, torch.int32):
        logits, density, stack = engine.evaluate_logits(x, stacks=given.to(dtype).cuda(), return_stacks=True)
        for i in range(c.B):
            k = int(given[i]) if 0 <= int(given[i]) < c.K else 0  # the oracle maps >= K itself; a negative index would wrap
            assert int(stack[i]) == k, (name, i)
            assert np.array_equal(logits[i].cpu().numpy(), c.oracle(i, k)[0]), (name, i, k)
            assert float(density[i]) == float(c.oracle(i, k)[1])
    for k in range(c.K):
        forced, _, stack = engine.evaluate_logits(x, stacks=torch.full((c.B,), k, dtype=torch.int64).cuda(), return_stacks=True)
        single, _ = EngineModel.load(c.path, bucket=k).evaluate_logits(x)
        assert torch.equal(forced, single) and int(stack.min()) == int(stack.max()) == k, (name, k)
    huge = torch.full((c.B,), 2 ** 32 + 1, dtype=torch.int64).cuda()  # does not wrap into the range
    assert torch.equal(engine.evaluate_logits(x, stacks=huge)[0], EngineModel.load(c.path).evaluate_logits(x)[0])
    with pytest.raises(ValueError):
        EngineModel.load(c.path).evaluate_logits(x, stacks=given.cuda())  # a single-stack model
    with pytest.raises(ValueError):
        engine.evaluate_logits(x, stacks=given[:-1].cuda())
    with pytest.raises(ValueError):
        engine.evaluate_logits(x, stacks=given.float().cuda())
    with pytest.raises(ValueError):
        engine.evaluate_logits(x, stacks=given)  # host tensor
    with pytest.raises(ValueError):
        EngineModel.load(c.path, bucket="all")


def test_one_stack_one_image_and_64_stacks(tmp_path, cases):
    arch = CASES["10x10x8"][0]
    one = Case(tmp_path, arch, 1, 6)
    auto, plain = EngineModel.load(one.path, bucket="auto"), EngineModel.load(one.path)
    assert auto.num_stacks == 1 and plain.num_stacks == 1
    x = one.images.cuda()
    logits, density, stack = auto.evaluate_logits(x, return_stacks=True)
    want_logits, want_density, zeros = plain.evaluate_logits(x, return_stacks=True)
    assert torch.equal(logits, want_logits) and torch.equal(density, want_density)
    assert int(stack.abs().max()) == 0 and int(zeros.abs().max()) == 0 and zeros.dtype == torch.int32
    # B = 1, on every image of the K = 4 case in turn
    c = cases("4x4x64")
    engine = EngineModel.load(c.path, bucket="auto")
    for i in (0, 5, c.B - 1):
        logits, density, stack = engine.evaluate_logits(c.images[i:i + 1].cuda(), return_stacks=True)
        assert int(stack[0]) == c.stacks[i]
        assert np.array_equal(logits[0].cpu().numpy(), c.oracle(i, c.stacks[i])[0])
    # K = 64
    (tmp_path / "k64").mkdir()
    big = Case(tmp_path / "k64", CASES["4x4x64"][0], 64, 12)
    engine = EngineModel.load(big.path, bucket="auto")
    assert engine.num_stacks == 64
    logits, density, stack = engine.evaluate_logits(big.images.cuda(), return_stacks=True)
    assert [int(k) for k in stack] == big.stacks and {0, 63} <= set(big.stacks) and len(set(big.stacks)) >= 6
    for i in range(big.B):
        assert np.array_equal(logits[i].cpu().numpy(), big.oracle(i, big.stacks[i])[0]), i
    given = torch.tensor([63, 64, 62, -1, 31, 0, 1, 2, 3, 40, 50, 60])
    logits, _, stack = engine.evaluate_logits(big.images.cuda(), stacks=given.cuda(), return_stacks=True)
    for i in range(big.B):
        k = int(given[i]) if 0 <= int(given[i]) < 64 else 0
        assert int(stack[i]) == k and np.array_equal(logits[i].cpu().numpy(), big.oracle(i, k)[0]), i


def test_auto_load_refuses_stacks_that_disagree(tmp_path, cases):
    c = cases("8x8x4")
    data = bytearray(c.path.read_bytes())
    classes, l3 = c.arch[5], c.arch[4]
    # the last stack's output layer ends the file: [u32 out][u32 in][out*in i8][u32 count][count i32]
    tail = 8 + classes * l3 + 4 + 4 * classes
    cut = bytes(data[:len(data) - tail]) + np.array([classes - 1, l3], np.uint32).tobytes() + bytes((classes - 1) * l3) \
        + np.array([classes - 1], np.uint32).tobytes() + bytes(4 * (classes - 1))
    (tmp_path / "bad.nnue").write_bytes(cut)
    with pytest.raises(EngineFormatError, match="classes"):
        EngineModel.load(tmp_path / "bad.nnue", bucket="auto")
    assert EngineModel.load(tmp_path / "bad.nnue").num_classes == classes  # an integer bucket loads as before
    longer = bytes(data[:len(data) - 4 - 4 * classes]) + np.array([classes + 1], np.uint32).tobytes() + bytes(4 * (classes + 1))
    (tmp_path / "bias.nnue").write_bytes(longer)
    with pytest.raises(EngineFormatError, match="bias"):
        EngineModel.load(tmp_path / "bias.nnue", bucket="auto")


def _exact_maps(F, counts, gen):
    maps = torch.zeros(len(counts), F, dtype=torch.bool)
    for s, n in enumerate(counts):
        maps[s, torch.randperm(F, generator=gen)[:n]] = True
    return maps


def _check_features(c, maps, logits, density, stacks, given=None):
    """step_features' outputs against the oracle, formed as test_gpu_engine_stream forms them, with the rule's stack."""
    for s in range(maps.shape[0]):
        ids = np.nonzero(maps[s].numpy())[0]
        k = rule(ids.size, c.K, c.F) if given is None else (int(given[s]) if 0 <= int(given[s]) < c.K else 0)
        assert int(stacks[s]) == k, (s, ids.size, int(stacks[s]), k)
        want = eo.forward_multiclass(c.ref["stacks"][k], eo.ft_forward(c.ref, ids), c.ref["l1"], c.ref["l2"], c.ref["l3"])
        assert np.array_equal(logits[s].cpu().numpy(), want), (s, ids.size, k)
        assert float(density[s]) == float(np.float32(ids.size) / np.float32(c.F))


@pytest.mark.parametrize("name", ["10x10x8", "4x4x64"])
def test_streams_at_exact_counts(cases, name):
    c = cases(name)
    engine = EngineModel.load(c.path, bucket="auto")
    F, K = c.F, c.K
    counts = [0, F]
    for k in range(1, K):  # the two sides of every boundary
        lo = -(-k * (F + 1) // K)
        counts += [lo - 1, lo]
        assert rule(lo - 1, K, F) == k - 1 and rule(lo, K, F) == k
    gen = torch.Generator().manual_seed(17)
    maps = _exact_maps(F, counts, gen)
    stream = engine.stream(len(counts))
    assert stream.stacks.dtype == torch.int32 and tuple(stream.stacks.shape) == (len(counts),)
    logits, density, changed = stream.step_features(maps.cuda())
    _check_features(c, maps, logits, density, stream.stacks)
    assert set(int(k) for k in stream.stacks) == set(range(K))
    assert [int(v) for v in changed] == counts
    # the same streams, every count moved to another place of the list: incremental or refresh per stream, same answers
    maps2 = maps.roll(3, 0)
    logits, density, _ = stream.step_features(maps2.to(torch.uint8).cuda())
    _check_features(c, maps2, logits, density, stream.stacks)
    # given stacks on a stream
    given = torch.randint(-2, K + 2, (len(counts),), generator=gen)
    logits, density, changed = stream.step_features(maps2.cuda(), stacks=given.cuda())
    assert int(changed.abs().max()) == 0
    _check_features(c, maps2, logits, density, stream.stacks, given)
    with pytest.raises(ValueError):
        EngineModel.load(c.path).stream(2).step_features(maps[:2].cuda(), stacks=given[:2].cuda())
    with pytest.raises(ValueError):
        stream.step_features(maps2.cuda(), stacks=given[:-1].cuda())


def test_stream_crosses_a_boundary_incrementally(cases):
    """One stream whose consecutive sets differ by a few ids and cross 512 | 513 (stack 1 | 2 of 4) both ways: the steps take
    the incremental path (changed is small and below the set's size).  The batched call takes images, not feature sets, so
    every step is checked against the oracle and against a second stream that is reset before each step (the from-scratch
    form); the same crossing through images is test_stream_steps_on_images."""
    c = cases("4x4x64")
    engine = EngineModel.load(c.path, bucket="auto")
    F, K = c.F, c.K
    gen = torch.Generator().manual_seed(19)
    order = torch.randperm(F, generator=gen)
    sizes = [509, 511, 512, 513, 516, 513, 512, 510, 513]
    stream, fresh = engine.stream(1), engine.stream(1)
    seen, prev = [], None
    for t, n in enumerate(sizes):
        maps = torch.zeros(1, F, dtype=torch.bool)
        maps[0, order[:n]] = True
        if t % 3 == 2:  # and swap two ids, so that a step both adds and removes rows
            maps[0, order[n - 1]] = False
            maps[0, order[F - 1 - t]] = True
        logits, density, changed = stream.step_features(maps.cuda())
        _check_features(c, maps, logits, density, stream.stacks)
        fresh.reset()
        want_logits, _, fresh_changed = fresh.step_features(maps.cuda())
        assert torch.equal(logits, want_logits) and torch.equal(stream.stacks, fresh.stacks)
        assert int(fresh_changed[0]) == n
        if prev is not None:
            assert int(changed[0]) == int((maps ^ prev).sum()) and 0 < int(changed[0]) <= 6
        seen.append(int(stream.stacks[0]))
        prev = maps
    assert seen == [rule(n, K, F) for n in sizes] and set(seen) == {1, 2}


def _growing_prefix_frames(size, lengths, seed=23):
    """One dark noise image with a bright prefix of the given lengths: neighbouring frames differ in a few pixels."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.randn(3 * size * size, generator=gen) * 0.3 - 1.5
    frames = base.repeat(len(lengths), 1)
    for t, n in enumerate(lengths):
        frames[t, :n] += 3.0
    return frames.view(len(lengths), 1, 3, size, size)


def test_stream_steps_on_images(cases):
    c = cases("4x4x64")
    engine = EngineModel.load(c.path, bucket="auto")
    size = c.size
    # S = B streams over three frames each: the case's images, rolled, and back
    x = c.images.cuda()
    stream = engine.stream(c.B)
    for frames in (x, x.roll(1, 0), x):
        logits, density, _ = stream.step(frames)
        want_logits, want_density, want_stack = engine.evaluate_logits(frames, return_stacks=True)
        assert torch.equal(logits, want_logits) and torch.equal(density, want_density) and torch.equal(stream.stacks, want_stack)
    assert set(int(k) for k in stream.stacks) == {0, 1, 2, 3}
    # one stream, a bright prefix growing and shrinking float by float across a conv patch: few features change per frame
    lengths = PREFIX_LENGTHS
    seq = _growing_prefix_frames(size, lengths).cuda()
    one = engine.stream(1)
    seen, small = [], 0
    for t in range(len(lengths)):
        logits, density, changed = one.step(seq[t])
        want_logits, want_density, want_stack = engine.evaluate_logits(seq[t], return_stacks=True)
        assert torch.equal(logits, want_logits) and torch.equal(density, want_density) and torch.equal(one.stacks, want_stack), t
        n = round(float(density[0]) * c.F)
        assert int(one.stacks[0]) == rule(n, c.K, c.F)
        small += t > 0 and 0 < int(changed[0]) < n // 2  # an incremental step, not a refresh
        seen.append(int(one.stacks[0]))
    assert len(set(seen)) >= 2 and small >= 4, (seen, small)
    # mixed with step_features, a reset in between, and given stacks
    gen = torch.Generator().manual_seed(29)
    maps = _exact_maps(c.F, [300], gen)
    logits, density, changed = one.step_features(maps.cuda())
    _check_features(c, maps, logits, density, one.stacks)
    logits, _, changed = one.step(seq[0])
    assert torch.equal(logits, engine.evaluate_logits(seq[0])[0])
    one.reset()
    logits, density, changed = one.step(seq[3])
    want_logits, want_density, want_stack = engine.evaluate_logits(seq[3], return_stacks=True)
    assert torch.equal(logits, want_logits) and torch.equal(one.stacks, want_stack)
    assert int(changed[0]) == round(float(density[0]) * c.F)  # the refresh counts every active feature
    given = torch.tensor([3]).cuda()
    logits, _, changed = one.step(seq[3], stacks=given)
    assert int(changed[0]) == 0 and int(one.stacks[0]) == 3
    assert torch.equal(logits, engine.evaluate_logits(seq[3], stacks=given)[0])
    assert not torch.equal(logits, want_logits) or int(want_stack[0]) == 3
    # a state buffer passes between the plain and the stack-selecting step
    single = EngineModel.load(c.path, bucket=0)
    plain_stream = single.stream(1)
    plain_stream.state = one.state
    logits, _, changed = plain_stream.step(seq[8])
    assert torch.equal(logits, single.evaluate_logits(seq[8])[0])
    assert int(changed[0]) == int((_ids(c, seq[8]) ^ _ids(c, seq[3])).sum()) > 0
    logits, _, changed = one.step(seq[2])
    assert torch.equal(logits, engine.evaluate_logits(seq[2])[0])
    assert int(changed[0]) == int((_ids(c, seq[2]) ^ _ids(c, seq[8])).sum()) > 0


def _ids(c, frame):
    conv, _ = eo.conv_forward(c.ref, frame.cpu().numpy().reshape(-1), c.size, c.size)
    on = np.zeros(c.F, dtype=bool)
    on[eo.active_features(c.ref, conv)] = True
    return on


# bright-prefix lengths (floats) of test_stream_steps_on_images' frame sequence: up and down across the conv patch at which
# the 4x4x64 model's count passes 512 | 513
PREFIX_LENGTHS = [1660, 1670, 1678, 1681, 1684, 3082, 3085, 3100, 3124, 3127, 3124, 3085, 3082, 1681, 1670]


def test_evaluate_compiled_model_selects_stacks(tmp_path, cases):
    import evaluate
    c = cases("4x4x64")
    K, classes, size = c.K, c.arch[5], c.size
    images = make_images(53, size, seed=31)
    gen = torch.Generator().manual_seed(1)
    labels = torch.randint(0, classes, (53,), generator=gen)
    loader = [(images[i:i + 16], labels[i:i + 16]) for i in (0, 16, 32)] + [(images[48:], labels[48:])]
    metrics = evaluate.evaluate_compiled_model(c.model.cuda(), loader, "nnue")
    assert set(metrics) == {"acc", "precision", "recall", "f1", "ms_per_sample", "latent_density"}
    outs, outs0, dens, used = [], [], [], []
    for img in images:
        flat = img.numpy().reshape(-1)
        n = eo.active_features(c.ref, eo.conv_forward(c.ref, flat, size, size)[0]).size
        lg, dn = eo.evaluate_logits(c.ref, flat, size, size, rule(n, K, c.F))
        outs.append(lg)
        outs0.append(eo.evaluate_logits(c.ref, flat, size, size, 0)[0])
        dens.append(float(dn))
        used.append(rule(n, K, c.F))
    assert set(used) == {0, 1, 2, 3}
    want = evaluate.compute_metrics(torch.from_numpy(np.stack(outs)), labels)
    stack0 = evaluate.compute_metrics(torch.from_numpy(np.stack(outs0)), labels)
    print("selected", want, "stack 0", stack0)
    assert all(abs(metrics[k] - want[k]) < 1e-12 for k in want)
    assert abs(metrics["latent_density"] - sum(dens) / len(dens)) < 1e-12
    assert any(metrics[k] != stack0[k] for k in stack0)
    # K = 1: what the single-stack engine gives
    one = make_model(CASES["10x10x8"][0], 1)
    x = make_images(21, 32, seed=37)
    y = torch.randint(0, 10, (21,), generator=gen)
    loader = [(x[:16], y[:16]), (x[16:], y[16:])]
    metrics = evaluate.evaluate_compiled_model(one.cuda(), loader, "nnue")
    path = tmp_path / "one.nnue"
    serialize.serialize_model(one, path)
    logits, density = EngineModel.load(path).evaluate_logits(x.cuda())
    want = evaluate.compute_metrics(logits, y.cuda())
    assert all(metrics[k] == want[k] for k in want)
    assert metrics["latent_density"] == float(density.double().mean().item())


@pytest.mark.parametrize("K", [1, 2])
def test_every_entry_agrees_past_the_first_column_slot(tmp_path, K):
    """L1 = 320: a thread owns columns tid and tid + 256, and the second one exists only for tid < 64, so the row walk's
    ``col < L1`` guard decides in slot 1.  F = 5*5*6 = 150 is three 64-bit words with a ragged last one.  Every way into the
    engine -- gather, matrix, feature maps, stream steps, refresh + a sparse update -- must give the same bits, the oracle's.
    K = 1 is the plain single-stack load, K = 2 selects per image."""
    c = Case(tmp_path, (5, 6, 320, 8, 8, 3, 17), K, 5)  # 17x17: stride 4, a 5x5 map, so all 150 ids can turn on
    assert c.F == 150 and c.ref["l1"] == 320
    engine = EngineModel.load(c.path, bucket="auto") if K > 1 else EngineModel.load(c.path)
    assert engine.num_stacks == K
    x = c.images.cuda()
    maps = torch.from_numpy(np.stack([_ids(c, c.images[i]) for i in range(c.B)]))
    assert [int(n) for n in maps.sum(1)] == c.counts and min(c.counts) == 0 and max(c.counts) == c.F

    want = engine.evaluate_logits(x, path="gather", return_stacks=True)
    got = {"matrix": engine.evaluate_logits(x, path="matrix", return_stacks=True),
           "features": engine.evaluate_features(maps.cuda(), return_stacks=True)}
    stream = engine.stream(c.B)
    got["step"] = stream.step(x)[:2] + (stream.stacks,)
    stream = engine.stream(c.B)
    got["step_features"] = stream.step_features(maps.cuda())[:2] + (stream.stacks,)
    # refresh to a set three ids short and three ids over, then one update back: with a duplicate and an id outside [0, F)
    start, added, removed = maps.clone(), [], []
    for s in range(c.B):
        on, off = np.nonzero(maps[s].numpy())[0], np.nonzero(~maps[s].numpy())[0]
        add, rem = [int(i) for i in on[1::max(1, on.size // 3)][:3]], [int(i) for i in off[::max(1, off.size // 3)][:3]]
        start[s, torch.tensor(add, dtype=torch.long)] = False
        start[s, torch.tensor(rem, dtype=torch.long)] = True
        added.append(add + add[:1] + [c.F + 5])
        removed.append(rem + rem[:1] + [-1])
    assert any(len(a) == 5 and len(r) == 5 for a, r in zip(added, removed))
    stream = engine.stream(c.B)
    stream.refresh([np.nonzero(start[s].numpy())[0] for s in range(c.B)])
    logits, density, changed = stream.update(added, removed)
    assert [int(v) for v in changed] == [len(set(a)) + len(set(r)) - 2 for a, r in zip(added, removed)]
    got["update"] = (logits, density, stream.stacks)

    for name, (logits, density, stack) in got.items():
        assert torch.equal(logits, want[0]), name
        assert torch.equal(density, want[1]), name
        assert torch.equal(stack, want[2]), name
    assert [int(k) for k in want[2]] == c.stacks and set(c.stacks) == set(range(K))
    for i in range(c.B):
        want_logits, want_density = c.oracle(i, c.stacks[i])
        assert np.array_equal(want[0][i].cpu().numpy(), want_logits), i
        assert float(want[1][i]) == float(want_density), i
