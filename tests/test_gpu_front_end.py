"""The float front end -- nnue_conv3x3_forward, nnue_ftm_conv_binarize[_patches], nnue_ftm_binarize, nnue_binarize_bits,
nnue_binarize_features, nnue_act_to_padded and nnue_conv3x3_backward_input -- against tests/front_cases.py, the float64
restatement that is the root of the front end's chain of bitwise tests.  ``-m gpu``.

Every output is an interior, 16-byte aligned view of an allocation prefilled with NaN / 0xFF whose bands must stay untouched, and
every call is made twice into the same buffers: the second result must be the first (counters re-zeroed).

a  exact inputs (every partial sum is exact in float32): everything bit for bit, thresholds on attained values;
b  random inputs: conv_out inside the derived fma-chain bound, bits wherever the bound decides them;
c  NaN / +Inf / -Inf / signed-zero pixels through the conv;
d  NaN, Inf, signed zeros, subnormals and FLT_MAX as map values and thresholds at every comparison site;
e  the pixel gradient, exact as well.
"""
import pytest
import torch

import front_cases as fc
import nnue_oracle as orc
from nnue_hip import lib
from test_gpu_forward_planes import Banded
from test_gpu_ftb import unpack

pytestmark = pytest.mark.gpu
DEV = "cuda"
L1 = 256  # sizes the scratch of the bit form only
RAW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def same(a, b):
    """Bit for bit (NaN payloads and the sign of zero included)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(RAW[a.element_size()]), b.view(RAW[b.element_size()]))


def filled(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.view(torch.uint8).fill_(0xFF)
    return t


def twice(launch, outs, band):
    """Two launches into the same buffers: the CPU copies of the first, which the second must repeat; bands untouched."""
    launch()
    torch.cuda.synchronize()
    first = [o.cpu().clone() for o in outs]
    launch()
    torch.cuda.synchronize()
    for k, (a, o) in enumerate(zip(first, outs)):
        assert same(a, o.cpu()), f"output {k}: the second call differs from the first"
    assert band.untouched(), "a guard band was written"
    return first


# ---------------------------------------------------------------------------------------------------------------- entry points
def run_conv(images, weight, stride):
    b, _, h, w = images.shape
    gh, gw = lib.conv_out_hw(h, w, stride)
    band = Banded()
    out = band(filled((b, weight.shape[0], gh, gw)))
    return twice(lambda: lib.conv3x3_forward(images, weight, stride, out=out), [out], band)[0]


def run_fused(images, weight, thr, stride, f, with_patches):
    b, _, h, w = images.shape
    fps = weight.shape[0]
    gh, gw = lib.conv_out_hw(h, w, stride)
    p = fps * gh * gw
    band = Banded()
    conv = band(filled((b, fps, gh, gw)))
    # own buffers: the launch takes any P, FeatureMatrix.empty sizes a forward's scratch as well
    fm = lib.FeatureMatrix(band(filled((b, p), torch.uint8)), band(filled((b,), torch.int32)), band(filled((b,))), None, p, f)
    patches = band(filled((27, b * gh * gw))) if with_patches else None
    outs = [conv, fm.bits, fm.n, fm.sink] + ([patches] if with_patches else [])
    got = twice(lambda: lib.ftm_conv_binarize(images, weight, thr, stride, f, L1, conv_out=conv, fm=fm, patches=patches), outs, band)
    return dict(zip(("conv", "bits", "n", "sink", "patches"), got))


def run_ftm_binarize(conv, thr, f):
    b, p = conv.shape[0], conv[0].numel()
    band = Banded()
    fm = lib.FeatureMatrix(band(filled((b, p), torch.uint8)), band(filled((b,), torch.int32)), band(filled((b,))), None, p, f)
    got = twice(lambda: lib.ftm_binarize(conv, thr, f, L1, fm=fm), [fm.bits, fm.n, fm.sink], band)
    return dict(zip(("bits", "n", "sink"), got))


def run_bits(conv, thr, f):
    b, p = conv.shape[0], conv[0].numel()
    band = Banded()
    e = lib.FeatureBits.empty(b, p, f, L1, DEV)
    w = lambda t: band(filled(t.shape, t.dtype))  # noqa: E731
    fb = lib.FeatureBits(w(e.maskW), w(e.maskT), w(e.sink), w(e.n), w(e.tlW), w(e.tcW), w(e.tlT), w(e.tcT), e.scratch, p, f)
    got = twice(lambda: lib.binarize_bits(conv, thr, f, L1, bits=fb), [fb.maskW, fb.maskT, fb.n, fb.sink], band)
    return dict(zip(("maskW", "maskT", "n", "sink"), got))


def run_features(conv, thr, f):
    """nnue_binarize_features, then nnue_act_to_padded at M = max(max n, 1) on its lists."""
    b, p = conv.shape[0], conv[0].numel()
    band = Banded()
    e = lib.ActList.empty(b, p, f, DEV)
    w = lambda t: band(filled(t.shape, t.dtype))  # noqa: E731
    act = lib.ActList(w(e.rows), w(e.pos), w(e.coef), w(e.n), w(e.coefT), e.cap, e.ldb)
    got = dict(zip(("rows", "pos", "coef", "n", "coefT"),
                   twice(lambda: lib.binarize_features(conv, thr, f, act=act), [act.rows, act.pos, act.coef, act.n, act.coefT], band)))
    m = max(int(got["n"].max()), 1)
    idx, val = band(filled((b, m), torch.int64)), band(filled((b, m)))
    launch = lambda: lib._call("nnue_act_to_padded", act.pos.data_ptr(), act.coef.data_ptr(), act.n.data_ptr(), act.cap, b, m,  # noqa: E731
                               idx.data_ptr(), val.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got["idx"], got["val"] = twice(launch, [idx, val], band)
    return got


# ---------------------------------------------------------------------------------------------------------------- checks
def check_counts(got, ref, f, undecided, what):
    """n and sink: exact where nothing is undecided, else within the number of undecided positions of that sample."""
    slack_n, slack_s = undecided.sum(1), undecided[:, f - 1:].sum(1)
    assert bool(((got["n"].long() - ref["n"]).abs() <= slack_n).all()), f"{what}: n"
    assert bool(((got["sink"] - ref["sink"]).abs() <= slack_s).all()), f"{what}: sink"


def check_bytes(got, ref, f, undecided, what):
    on = ref["on"]
    assert got["bits"].dtype == torch.uint8 and bool((got["bits"] <= 1).all()), f"{what}: bytes other than 0 / 1"
    wrong = (got["bits"] != on.to(torch.uint8)) & ~undecided
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} bits differ, first at {wrong.nonzero()[0].tolist()}"
    check_counts(got, ref, f, undecided, what)


def check_bit_form(got, ref, f, undecided, what):
    on = ref["on"]
    b, p = on.shape
    words = unpack(got["maskW"], got["maskW"].shape[1] * 64)
    assert not bool(((words[:, :p] != on) & ~undecided).any()), f"{what}: maskW"
    assert not bool(words[:, p:].any()), f"{what}: maskW padding bits"
    check_counts(got, ref, f, undecided, what)
    direct = min(f - 1, p)
    rows = unpack(got["maskT"], got["maskT"].shape[1] * 64)
    assert not bool(((rows[:direct, :b] != on[:, :direct].t()) & ~undecided[:, :direct].t()).any()), f"{what}: maskT"
    assert not bool(rows[direct:f - 1].any()) and bool(rows[f, :b].all()) and not bool(rows[:, b:].any()), f"{what}: maskT rows / padding"
    if not bool(undecided.any()):
        assert torch.equal(rows[f - 1, :b], ref["sink"] != 0), f"{what}: maskT sink row"


def check_lists(got, ref, f, what):
    """rows / pos / coef ascending and equal to the lists (entries past n[b] keep their 0xFF / NaN fill), coefT, the padded form."""
    idx = ref["idx"]
    b, p = idx.shape
    keep = idx >= 0
    assert torch.equal(got["n"].long(), ref["n"]), f"{what}: n"
    assert torch.equal(got["pos"].long(), idx), f"{what}: pos"  # the 0xFF fill reads as -1, the lists' own padding
    assert torch.equal(got["rows"].long(), torch.where(keep, idx.clamp(max=f - 1), idx)), f"{what}: rows"
    assert same(got["coef"], torch.where(keep, 1.0, float("nan")).float()), f"{what}: coef"
    want = orc.coefficient_matrix(idx, keep.float(), f)  # [B, F]
    assert torch.equal(got["coefT"][:, :b], want.t()), f"{what}: coefT"
    assert not bool(got["coefT"].view(torch.int32)[:, b:].any()), f"{what}: coefT columns past B"
    m = got["idx"].shape[1]
    assert m == max(int(ref["n"].max()), 1)
    assert torch.equal(got["idx"], idx[:, :m]) and torch.equal(got["val"], keep[:, :m].float()), f"{what}: act_to_padded"


def check_binarisers(conv, thr, f, ref, undecided=None, what=""):
    """The three stand-alone binarisers on a device map against a reference's on / n / sink / idx."""
    b, p = ref["on"].shape
    exact = undecided is None
    undecided = torch.zeros(b, p, dtype=torch.bool) if exact else undecided
    if p % 4 == 0:
        check_bytes(run_ftm_binarize(conv, thr, f), ref, f, undecided, f"{what} ftm_binarize")
    check_bit_form(run_bits(conv, thr, f), ref, f, undecided, f"{what} binarize_bits")
    feats = run_features(conv, thr, f)
    if exact:
        check_lists(feats, ref, f, f"{what} binarize_features")
    else:
        assert bool(((feats["n"].long() - ref["n"]).abs() <= undecided.sum(1)).all()), f"{what} binarize_features: n"


def check_fused(images, weight, thr, stride, f, ref, conv_ok, undecided=None, what=""):
    """nnue_ftm_conv_binarize and nnue_ftm_conv_binarize_patches against a front64 result; conv_ok(conv_out, what) asserts."""
    b, p = ref["on"].shape
    undecided = torch.zeros(b, p, dtype=torch.bool) if undecided is None else undecided
    for with_patches in (False, True):
        tag = f"{what} ftm_conv_binarize" + ("_patches" if with_patches else "")
        got = run_fused(images, weight, thr, stride, f, with_patches)
        conv_ok(got["conv"], tag)
        check_bytes(got, ref, f, undecided, tag)
        if with_patches:
            assert same(got["patches"], ref["patches"].float()), f"{tag}: patches"


def bitwise(ref_conv):
    want = ref_conv.float()
    assert torch.equal(want.double(), ref_conv), "the reference is not a float32 value"

    def ok(conv, what):
        bad = conv.view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), f"{what}: conv_out differs at {int(bad.sum())} positions, first {bad.nonzero()[0].tolist()}"
    return ok


def on_device(c):
    """The images as an interior view too: a read past a sample's last row or the batch's end meets NaN, not a neighbour's zeros."""
    return Banded()(c["images"].to(DEV)), c["weight"].to(DEV), c["thr"].to(DEV)


def variant_id(v):
    return fc.shape_id(v) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------------------------------------------------------- a
EXACT = [(s, 0, 0) for s in fc.ALL_SHAPES] + [(s, si, sw) for s in fc.SCALED_SHAPES for si, sw in fc.SCALES]


@pytest.mark.parametrize("shape,si,sw", EXACT, ids=variant_id)
def test_exact_inputs_bit_for_bit(shape, si, sw):
    c = fc.exact_case(shape, fc.seed_of(shape), si, sw)
    stride, f = c["stride"], c["F"]
    ref = fc.front64(c["images"], c["weight"], c["thr"], stride, f)
    ties = (ref["conv_out"] == c["thr"].double().view(1, -1, 1, 1)).sum((0, 2, 3))
    assert int(ties.min()) >= 1, "a channel without a tie: the verdict below would not see a >= in a kernel"
    images, weight, thr = on_device(c)
    ok = bitwise(ref["conv_out"])
    conv = run_conv(images, weight, stride)
    ok(conv, "conv3x3_forward")
    check_fused(images, weight, thr, stride, f, ref, ok)
    check_binarisers(conv.to(DEV), thr, f, ref)


# ---------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.shape_id)
def test_random_inputs_inside_the_chain_bound(shape):
    c = fc.random_case(shape, fc.seed_of(shape))
    stride, f, bound = c["stride"], c["F"], c["bound"]
    ref = fc.front64(c["images"], c["weight"], c["thr"], stride, f)
    b, p = ref["on"].shape
    undecided = ((ref["conv_out"] - c["thr"].double().view(1, -1, 1, 1)).abs() <= bound).reshape(b, p)
    left_out = int(undecided.sum())
    assert left_out <= 0.001 * b * p, "a condition of the case (tests/test_front_cases.py)"
    worst = []

    def ok(conv, what):
        ratio = float(((conv.double() - ref["conv_out"]).abs() / bound).max())
        worst.append(ratio)
        assert ratio <= 1.0, f"{what}: conv_out error is {ratio:.3f} of the bound"

    images, weight, thr = on_device(c)
    conv = run_conv(images, weight, stride)
    ok(conv, "conv3x3_forward")
    check_fused(images, weight, thr, stride, f, ref, ok, undecided)
    check_binarisers(conv.to(DEV), thr, f, ref, undecided if left_out else None)
    print(f"front end {fc.shape_id(shape)}: worst error / bound {max(worst):.3f}, positions left out {left_out} of {b * p}")


# ---------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("shape", fc.NONFINITE_SHAPES, ids=fc.shape_id)
def test_nonfinite_and_signed_zero_pixels(shape):
    c = fc.nonfinite_case(shape, fc.seed_of(shape))
    stride, f = c["stride"], c["F"]
    ref = fc.front64(c["images"], c["weight"], c["thr"], stride, f)
    r = ref["conv_out"]
    assert bool(torch.isnan(r).any()) and bool(torch.isposinf(r).any()) and bool(torch.isneginf(r).any()) and bool((r[-1] == 0).any())
    flat, on = r.reshape(r.shape[0], -1), ref["on"]
    assert not bool(on[torch.isnan(flat)].any()) and not bool(on[torch.isneginf(flat)].any()) and bool(on[torch.isposinf(flat)].all())
    want = r.float()

    def ok(conv, what):
        assert torch.equal(torch.isnan(conv), torch.isnan(r)), f"{what}: NaN not exactly where the reference has it"
        assert torch.equal(torch.isposinf(conv), torch.isposinf(r)) and torch.equal(torch.isneginf(conv), torch.isneginf(r)), f"{what}: Inf"
        fin = torch.isfinite(r)
        assert same(conv[fin], want[fin]), f"{what}: finite outputs"

    images, weight, thr = on_device(c)
    conv = run_conv(images, weight, stride)
    ok(conv, "conv3x3_forward")
    check_fused(images, weight, thr, stride, f, ref, ok)
    check_binarisers(conv.to(DEV), thr, f, ref)


# ---------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("map_shape,f,first", fc.MAP_SHAPES, ids=variant_id)
def test_map_and_threshold_edges_at_the_binarisers(map_shape, f, first):
    x, thr = fc.edge_map(map_shape, sum(map_shape), first)
    on = (x > thr.view(1, -1, 1, 1)).reshape(map_shape[0], -1)  # torch's own comparison on the CPU
    check_binarisers(x.to(DEV), thr.to(DEV), f, fc.forms_of(on, f))


def test_threshold_edges_at_the_fused_comparison():
    shape = (2, 33, 31, 20, 3, 1000)
    c = fc.exact_case(shape, fc.seed_of(shape))
    c["thr"] = fc.edge_thresholds(c["thr"])
    stride, f = c["stride"], c["F"]
    ref = fc.front64(c["images"], c["weight"], c["thr"], stride, f)
    per_channel = ref["on"].reshape(shape[0], shape[3], -1).sum((0, 2))
    assert int((per_channel == 0).sum()) >= 4 and int((per_channel == ref["on"].shape[1] // shape[3] * shape[0]).sum()) >= 2  # +Inf / NaN, -Inf
    images, weight, thr = on_device(c)
    check_fused(images, weight, thr, stride, f, ref, bitwise(ref["conv_out"]))


@pytest.mark.parametrize("shape", fc.SCALED_SHAPES, ids=fc.shape_id)
def test_threshold_one_subnormal_step_below_an_attained_value(shape):
    """Outputs are subnormal multiples of 2**-145; the threshold sits 2**-149 under an attained one, which is therefore active.
    A device that flushes subnormals in the conv or in the comparison fails here."""
    c = fc.exact_case(shape, fc.seed_of(shape), -70, -70)
    attained = c["thr"]
    c["thr"] = torch.nextafter(attained, torch.full_like(attained, float("-inf")))
    assert torch.equal(attained.double() - c["thr"].double(), torch.full_like(attained, fc.SUBNORMAL, dtype=torch.float64))
    stride, f = c["stride"], c["F"]
    ref = fc.front64(c["images"], c["weight"], c["thr"], stride, f)
    tie = (ref["conv_out"] == attained.double().view(1, -1, 1, 1)).reshape(shape[0], -1)
    assert int(tie.reshape(shape[0], shape[3], -1).sum((0, 2)).min()) >= 1 and bool(ref["on"][tie].all())
    images, weight, thr = on_device(c)
    ok = bitwise(ref["conv_out"])
    conv = run_conv(images, weight, stride)
    ok(conv, "conv3x3_forward")
    check_fused(images, weight, thr, stride, f, ref, ok)
    check_binarisers(conv.to(DEV), thr, f, ref)


# ---------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("shape", fc.BACKWARD_SHAPES, ids=fc.shape_id)
def test_pixel_gradient_bit_for_bit(shape):
    """d_conv_out and the weights on the exact grid: a pixel receives at most 9 * fps <= 576 terms, each a multiple of 1/32 of
    magnitude at most 2, so every partial sum is exact in float32 and float64 conv2d_input is the answer bit for bit."""
    b, h, w, fps, stride = shape
    gh, gw = lib.conv_out_hw(h, w, stride)
    gen = torch.Generator().manual_seed(fc.seed_of(shape))
    d_out = torch.randint(-8, 9, (b, fps, gh, gw), generator=gen).float() / 4
    weight = torch.randint(-8, 9, (fps, 3, 3, 3), generator=gen).float() / 8
    ref = torch.nn.grad.conv2d_input((b, 3, h, w), weight.double(), d_out.double(), stride=stride, padding=1)
    assert torch.equal(ref.float().double(), ref)
    rows = torch.zeros(h, dtype=torch.bool)
    cols = torch.zeros(w, dtype=torch.bool)
    for k in (-1, 0, 1):  # pixels under some patch
        ry, rx = torch.arange(gh) * stride + k, torch.arange(gw) * stride + k
        rows[ry[(ry >= 0) & (ry < h)]] = True
        cols[rx[(rx >= 0) & (rx < w)]] = True
    covered = rows.view(-1, 1) & cols.view(1, -1)
    assert (stride <= 3 or bool((~covered).any())) and bool(ref.abs().sum((0, 1))[covered].ne(0).any())
    band = Banded()
    d_img = band(filled((b, 3, h, w)))
    d_out_d, weight_d = d_out.to(DEV), weight.to(DEV)
    launch = lambda: lib._call("nnue_conv3x3_backward_input", d_out_d.data_ptr(), weight_d.data_ptr(), b, h, w, fps, stride,  # noqa: E731
                               d_img.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = twice(launch, [d_img], band)[0]
    bad = got != ref.float()
    assert not bool(bad.any()), f"{int(bad.sum())} pixels differ, first {bad.nonzero()[0].tolist()}"
    assert not bool(got[:, :, ~covered].view(torch.int32).any()), "a pixel no patch covers is not +0.0"
