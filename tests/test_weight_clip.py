"""The weight clip's launch-free side (include/nnue_hip.h, "weight clip"): argument checks of the trainer, the drop-in
optimizers' groups, the config reader and the C entry points; the flat buffers' clip ranges and their shard windows; and the
step mode, which the option is not an input of.  CPU only."""
import ctypes
import inspect
import math
from types import SimpleNamespace

import pytest
import torch

import nnue
import trainer_modes as tm
from nnue_hip import lib, optim, step_mode, train_loop
from nnue_hip.trainer import CLIPPED, FlatLayout, NnueTrainer, clip_ranges

BAD = (-1.0, -1e-9, float("nan"), float("inf"), float("-inf"))


@pytest.mark.parametrize("value", BAD)
def test_trainer_refuses_a_bad_bound(value):
    """Refused before the model, the library or the device is touched."""
    with pytest.raises(ValueError, match="weight_clip"):
        NnueTrainer(None, 8, (8, 8), lr=0.1, weight_clip=value)


@pytest.mark.parametrize("value", BAD)
@pytest.mark.parametrize("cls", (optim.SGD, optim.Adam))
def test_optimizer_groups_refuse_a_bad_bound(cls, value):
    w, b = torch.nn.Parameter(torch.zeros(4, 4)), torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="weight_clip"):
        cls([w, b], lr=0.1, weight_clip=value)
    with pytest.raises(ValueError, match="weight_clip"):
        cls([dict(params=[w], weight_clip=value), dict(params=[b])], lr=0.1)
    opt = cls([w], lr=0.1)
    with pytest.raises(ValueError, match="weight_clip"):
        opt.add_param_group(dict(params=[b], weight_clip=value))
    assert len(opt.param_groups) == 1


@pytest.mark.parametrize("cls", (optim.SGD, optim.Adam))
def test_the_option_is_a_group_option_that_survives_the_state_dict(cls):
    w, b = torch.nn.Parameter(torch.full((4, 4), 3.0)), torch.nn.Parameter(torch.full((4,), 3.0))
    opt = cls([dict(params=[w], weight_clip=1.0), dict(params=[b])], lr=0.1)
    assert [g["weight_clip"] for g in opt.param_groups] == [1.0, 0.0] and opt.defaults["weight_clip"] == 0.0
    sd = opt.state_dict()
    assert [g["weight_clip"] for g in sd["param_groups"]] == [1.0, 0.0]
    other = cls([dict(params=[w]), dict(params=[b], weight_clip=0.5)], lr=0.1)
    other.load_state_dict(sd)
    assert [g["weight_clip"] for g in other.param_groups] == [1.0, 0.0]
    # a dict from torch's own optimizer has no such key: the groups keep their own
    for g in sd["param_groups"]:
        del g["weight_clip"]
    third = cls([dict(params=[w]), dict(params=[b], weight_clip=0.5)], lr=0.1)
    third.load_state_dict(sd)
    assert [g["weight_clip"] for g in third.param_groups] == [0.0, 0.5]
    # the CPU convenience path: stock torch, then clamp_ on the groups that ask for it
    w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
    opt.step()
    assert torch.all(w == 1.0) and torch.all(b == 3.0)


def test_the_config_reader():
    assert train_loop.config_weight_clip(SimpleNamespace()) == 0.0
    assert train_loop.config_weight_clip(SimpleNamespace(weight_clip=1)) == 1.0
    for value in BAD:
        with pytest.raises(ValueError, match="weight_clip"):
            train_loop.config_weight_clip(SimpleNamespace(weight_clip=value))


def _model(K):
    torch.manual_seed(0)
    return nnue.NNUE(nnue.GridFeatureSet(10, 8), 72, 7, 5, num_classes=3, input_size=32, num_ls_buckets=K)


@pytest.mark.parametrize("K", (1, 4))
def test_the_ranges_cover_the_four_tensors_and_their_padding(K):
    model = _model(K)
    layout = FlatLayout.of(model, pad_to=4)
    ranges = clip_ranges(layout)
    assert len(ranges) == 4 and all(lo % 4 == 0 and hi % 4 == 0 and lo < hi for lo, hi in ranges)
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    # mark the buffer: 1 = an element of a clipped tensor, 2 = of another tensor, 0 = padding
    kind = torch.zeros(layout.count, dtype=torch.int8)
    for k, v in layout.views(kind).items():
        v.fill_(1 if k in CLIPPED else 2)
    assert set(CLIPPED) <= set(layout.names)
    if K > 1:
        assert layout.shapes[layout.names.index("classifier.classifier.0.weight")][0] == K  # the stacked [K, out, in] weights
    covered = torch.zeros(layout.count, dtype=torch.bool)
    for lo, hi in ranges:
        covered[lo:hi] = True
    assert torch.all(covered[kind == 1]) and not torch.any(covered[kind == 2])
    assert K > 1 or int((kind == 0).sum()) > 0  # (one stack: odd tensor sizes, so there is padding; four: every size is a multiple of 4)
    clip = lib.WeightClip(1.0, ranges)
    assert clip.on and clip.args()[0] == 1.0 and list(clip.array) == [x for r in ranges for x in r]
    assert not lib.WeightClip(0.0, ranges).on


@pytest.mark.parametrize("world", (2, 3))
@pytest.mark.parametrize("K", (1, 4))
def test_the_shard_windows_tile_the_ranges(K, world):
    layout = FlatLayout.of(_model(K), pad_to=4 * world)
    clip = lib.WeightClip(1.0, clip_ranges(layout))
    per = layout.count // world
    assert per * world == layout.count and per % 4 == 0
    covered = torch.zeros(layout.count, dtype=torch.int32)
    for rank in range(world):
        win = clip.window(rank * per, (rank + 1) * per)
        assert len(win.ranges) <= 4 and win.bound == 1.0
        for lo, hi in win.ranges:
            assert 0 <= lo < hi <= per and lo % 4 == 0 and hi % 4 == 0
            covered[rank * per + lo:rank * per + hi] += 1
    want = torch.zeros(layout.count, dtype=torch.int32)
    for lo, hi in clip.ranges:
        want[lo:hi] = 1
    assert torch.equal(covered, want)  # every clipped element in exactly one shard's window, nothing else in any


def test_the_option_is_not_an_input_of_the_step_mode():
    """The clip is a hyper-parameter, not a mode: every mode supports it, and resolve() cannot see it."""
    assert not [p for p in inspect.signature(step_mode.resolve).parameters if "weight_clip" in p]
    assert not [f for f in step_mode.StepMode.__dataclass_fields__ if "weight_clip" in f]
    assert "weight_clip" in inspect.signature(NnueTrainer.__init__).parameters
    for row in tm.ROWS:  # (the table of tests/test_trainer_modes_policy.py: the same StepMode whatever the option is)
        assert tm.step_mode_of(row.config) == tm.step_mode_of(dict(row.config, weight_clip=1.0))


def test_the_entry_points_refuse_a_bad_bound_without_launching():
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ranges = (ctypes.c_int64 * 2)(0, 8)
    sgd = lambda c, r=ranges, n=1: L.nnue_sgd_step_clip(p, p, p, 16, 0.1, 0.9, 0.0, 1.0, 1.0, 1, None, p, 1 << 20, None, 0, 0, None, None,  # noqa: E731
                                                        None, 0, 0, 0, None, 0, None, c, r, n, None)
    adam = lambda c: L.nnue_adam_step_clip(p, p, p, p, p, 16, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, None, p, 1 << 20, None, c, ranges, 1, None)  # noqa: E731
    adam_ext = lambda c: L.nnue_adam_step_ext_clip(p, p, p, p, p, 16, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, None, p, 1 << 20, None, 0, 0, 0,  # noqa: E731
                                                   None, 0, None, c, ranges, 1, None)
    table = lambda c: L.nnue_ftm_backward_weight_update_clip(p, p, 8, 16, 16, 64, p, p, p, 0.1, 0.9, 0.0, 1.0, 0, c, None, None)  # noqa: E731
    table_adam = lambda c: L.nnue_ftm_backward_weight_update_adam_clip(p, p, 8, 16, 16, 64, p, p, p, p, p, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0,  # noqa: E731
                                                                       c, None, None)
    fused = lambda c: L.nnue_ftm_backward_weight_update_forward_clip(p, p, 8, 16, 16, 64, p, p, p, 0.1, 0.9, 0.0, 1.0, 0, c, None, p, p, 8, p,  # noqa: E731
                                                                     p, p, 1 << 20, None)
    fused_adam = lambda c: L.nnue_ftm_backward_weight_update_forward_adam_clip(p, p, 8, 16, 16, 64, p, p, p, p, p, 0.1, 0.9, 0.999, 1e-8,  # noqa: E731
                                                                               0.0, 1.0, c, None, p, p, 8, p, p, p, 1 << 20, None)
    ptrs, counts = (ctypes.c_void_p * 1)(p), (ctypes.c_int64 * 1)(16)
    one = lambda v: (ctypes.c_float * 1)(v)  # noqa: E731
    steps = (ctypes.c_void_p * 1)(p)
    multi_sgd = lambda c: L.nnue_multi_sgd_step_clip(ptrs, ptrs, ptrs, counts, 1, one(0.1), one(0.9), one(0.0), (ctypes.c_int32 * 1)(1),  # noqa: E731
                                                     one(c), 1.0, None, p, 1 << 20, None, None)
    multi_adam = lambda c: L.nnue_multi_adam_step_clip(ptrs, ptrs, ptrs, ptrs, steps, counts, 1, one(0.1), one(0.9), one(0.999), one(1e-8),  # noqa: E731
                                                       one(0.0), one(c), 1.0, None, p, 1 << 20, None, None)
    for call in (sgd, adam, adam_ext, table, table_adam, fused, fused_adam, multi_sgd, multi_adam):
        for value in BAD:
            assert call(value) == -1, (call, value)
            assert b"weight_clip" in L.nnue_hip_last_error()
    # ranges outside the buffer, reversed, or more than four
    for r in ((0, 17), (8, 4), (-4, 4)):
        assert sgd(1.0, (ctypes.c_int64 * 2)(*r)) == -1 and b"clip range" in L.nnue_hip_last_error()
    assert sgd(1.0, (ctypes.c_int64 * 10)(), 5) == -1
    assert sgd(1.0, None, 1) == -1
    assert math.isfinite(lib.checked_weight_clip(3.0))
