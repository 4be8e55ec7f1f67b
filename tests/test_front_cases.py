"""tests/front_cases.py, pinned on the CPU: the float64 restatement of the conv against torch's own conv, the exactness of the
dyadic cases, the ties the thresholds sit on, and the two conditions the random cases rest on."""
import pytest
import torch
import torch.nn.functional as F

import front_cases as fc

IDS = dict(ids=fc.shape_id)


def torch_conv(images, weight, stride, dtype):
    return F.conv2d(images.to(dtype), weight.to(dtype), stride=stride, padding=1)


@pytest.mark.parametrize("shape", fc.SHAPES, **IDS)
def test_conv64_is_torchs_float64_conv(shape):
    c = fc.random_case(shape, fc.seed_of(shape))
    got, ref = fc.conv64(c["images"], c["weight"], c["stride"]), torch_conv(c["images"], c["weight"], c["stride"], torch.float64)
    assert got.shape == ref.shape and got.dtype == torch.float64
    assert float((got - ref).abs().max()) <= 1e-12


def test_conv64_propagates_by_ieee_rules():
    images, weight = torch.ones(1, 3, 3, 3), torch.ones(2, 3, 3, 3)
    weight[1, 0, 1, 1] = 0.0
    images[0, 0, 1, 1] = float("inf")
    out = fc.conv64(images, weight, 1)
    assert bool(torch.isposinf(out[0, 0]).all())
    assert bool(torch.isnan(out[0, 1, 1, 1])) and int(torch.isposinf(out[0, 1]).sum()) == 8  # 0 * inf = NaN under the zero tap only
    images[0, 1, 1, 1] = float("-inf")
    assert bool(torch.isnan(fc.conv64(images, weight, 1)[0, 0]).all())  # inf - inf = NaN


def exact_variants():
    for shape in fc.ALL_SHAPES:
        yield shape, 0, 0
    for shape in fc.SCALED_SHAPES:
        for si, sw in fc.SCALES:
            yield shape, si, sw


@pytest.mark.parametrize("shape,si,sw", list(exact_variants()), ids=lambda v: fc.shape_id(v) if isinstance(v, tuple) else str(v))
def test_exact_cases_are_exact_tied_and_balanced(shape, si, sw):
    b, h, w, fps, stride, f, gh, gw, g, p = fc.geometry(shape)
    c = fc.exact_case(shape, fc.seed_of(shape), si, sw)
    ref = fc.front64(c["images"], c["weight"], c["thr"], stride, f)
    conv = ref["conv_out"]
    assert torch.equal(torch_conv(c["images"], c["weight"], stride, torch.float32).double(), conv), "float32 is not exact here"
    assert torch.equal(conv.float().double(), conv)
    if (si, sw) == (-70, -70):
        tiny = torch.finfo(torch.float32).tiny
        assert bool(((conv != 0) & (conv.abs() < tiny)).any()) and float(conv.abs().max()) < tiny, "outputs are subnormal"
    ties = (conv == c["thr"].double().view(1, -1, 1, 1)).sum((0, 2, 3))
    assert int(ties.min()) >= 1, "a channel without a tie"
    if g * b >= 100:
        density = float(ref["on"].double().mean())
        assert 0.3 <= density <= 0.7, density
    # the forms agree with each other
    assert torch.equal(ref["n"], (ref["idx"] >= 0).sum(1))
    assert ref["patches"].shape == (27, b * g)
    if f - 1 >= p:
        assert not bool(ref["sink"].any())


def test_patches_layout():
    """patches[q][b*G + hw] is the pixel under tap q = ci*9 + kh*3 + kw of position hw, 0 off the image (checked by index)."""
    shape = (3, 9, 9, 4, 4, 30)
    b, h, w, fps, stride, f, gh, gw, g, p = fc.geometry(shape)
    c = fc.exact_case(shape, 5)
    pt = fc.front64(c["images"], c["weight"], c["thr"], stride, f)["patches"]
    for s in range(b):
        for hw in range(g):
            for q in range(27):
                ci, kh, kw = q // 9, q // 3 % 3, q % 3
                iy, ix = hw // gw * stride + kh - 1, hw % gw * stride + kw - 1
                want = float(c["images"][s, ci, iy, ix]) if 0 <= iy < h and 0 <= ix < w else 0.0
                assert float(pt[q, s * g + hw]) == want


@pytest.mark.parametrize("shape", fc.SHAPES, **IDS)
def test_random_cases_meet_their_conditions(shape):
    b, h, w, fps, stride, f, gh, gw, g, p = fc.geometry(shape)
    c = fc.random_case(shape, fc.seed_of(shape))
    conv = fc.conv64(c["images"], c["weight"], stride)
    undecided = (conv - c["thr"].double().view(1, -1, 1, 1)).abs() <= c["bound"]
    assert int(undecided.sum()) <= 0.001 * conv.numel(), "too many positions within the bound of their threshold"
    err = (torch_conv(c["images"], c["weight"], stride, torch.float32).double() - conv).abs()
    assert bool((err <= c["bound"]).all()), "torch's float32 conv leaves the derived bound"
    print(f"{fc.shape_id(shape)}: undecided {int(undecided.sum())}, torch f32 worst error / bound {float((err / c['bound']).max()):.3f}")


@pytest.mark.parametrize("shape", fc.NONFINITE_SHAPES, **IDS)
def test_nonfinite_cases_hold_every_kind(shape):
    c = fc.nonfinite_case(shape, fc.seed_of(shape))
    conv = fc.conv64(c["images"], c["weight"], c["stride"])
    assert bool(torch.isnan(conv).any()) and bool(torch.isposinf(conv).any()) and bool(torch.isneginf(conv).any())
    assert bool(torch.isfinite(conv).any()) and bool((conv[-1] == 0).any())
    assert bool(torch.isfinite(c["thr"]).all())


@pytest.mark.parametrize("map_shape,f,first", fc.MAP_SHAPES, ids=lambda v: fc.shape_id(v) if isinstance(v, tuple) else str(v))
def test_edge_maps_hold_every_value_and_threshold(map_shape, f, first):
    x, thr = fc.edge_map(map_shape, sum(map_shape), first)
    assert x.shape == map_shape and x.dtype == torch.float32
    bits = x.view(torch.int32)
    for c in range(map_shape[1]):
        ch = x[:, c]
        assert bool(torch.isnan(ch).any()) and bool(torch.isposinf(ch).any()) and bool(torch.isneginf(ch).any())
        for v in (0.0, -0.0, fc.SUBNORMAL, -fc.SUBNORMAL, fc.FLT_MAX):
            assert bool((bits[:, c] == torch.tensor(v).view(torch.int32)).any()), (c, v)
        if fc.THR_KINDS[(first + c) % 7] == "attained":
            assert bool((ch == thr[c]).any())
    kinds = {fc.THR_KINDS[(first + c) % 7] for c in range(map_shape[1])}
    assert len(kinds) == min(7, map_shape[1])
    # with the smallest subnormal in the map and +0.0 / the subnormal among the thresholds, a flush to zero changes the answer
    on = x > thr.view(1, -1, 1, 1)
    assert bool(on[x == fc.SUBNORMAL].any()) and not bool(on[x == fc.SUBNORMAL].all())
