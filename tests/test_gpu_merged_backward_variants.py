"""Every instantiation of the merged FeatureTransformer backward (nnue_ftm_backward / nnue_ftm_backward_bucketed:
ftm_backward_kernel and ftm_backward_bf_kernel) that the shape policy can launch with per-call knobs, at ragged shapes, against
float64.  GPU tests are marked ``gpu``; the policy test at the top runs without one.

The policy (merged_backward_plan in csrc/ftm_kernels.hip) picks the kernel from the shape alone:
  big    the two products give >= 448 tiles of 64 x 64: 64 x 64 x 64 tiles for both
  mid    fewer tiles, but the value product alone takes 64-row tiles: 64 x 64 x 64 value tiles, 32-row f32 weight tiles
  small  32 x 64 x 128 value tiles (the batch-512 CIFAR launch; every other test of the merged launch at a ragged shape lands here)
and L1 % 8 == 0 turns the 64 x 64 value tiles into six bf16 plane products.  NNUE_FTM_BF_WM=32 and NNUE_FTM_BF16=0 (both read
per call) swap the weight tiles.  ROWS below are the smallest shapes of each class with a ragged batch, at least two row tiles and
tails on every axis; each names the kernel it must reach under the three knob settings, and test_which_kernel_serves_the_call
reads that name off the profiler, so a policy change that moves a shape elsewhere fails instead of hollowing the file.

Nine instantiations are reachable this way and all are named in ROWS.

Two value regimes per (shape, knob):
  grid    weight and d_out are multiples of 2^-6 in [-1, 1], the map has density 0.3 below the clamp sink and at most 16 active
          positions per sample at or past row F - 1.  Every sum the launch forms (<= 512 products that are multiples of 2^-12,
          <= 257 batch terms, sink counts <= 16) is exact in float32 in any order -- asserted on the CPU, not assumed -- and
          the three-way bf16 split of such operands is exact, so results are compared for EQUALITY with float64.
  randn   full-mantissa operands against the float64 restatement at the bar the stand-alone kernels meet (2e-5 of the
          tensor's scale), plus the merged-vs-stand-alone relations of test_merged_backward_is_bitwise_the_two_launches.
Every output of every launch here is an interior view of a NaN-filled buffer whose bands must stay NaN.
"""
import os

import pytest
import torch

from conftest import assert_close_grad
from nnue_hip import lib
from test_gpu_ftm import dense_reference

gpu = pytest.mark.gpu
DEV = "cuda"
L2 = 72  # rider rows: three 32-row tiles / two 64-row tiles, the last with 8 rows

BF64_V6 = "ftm_backward_bf_kernel<64, 64, 64, 64, true, true>"
BF64_F32 = "ftm_backward_bf_kernel<64, 64, 64, 64, false, true>"
BF64_SMALL = "ftm_backward_bf_kernel<64, 32, 64, 128, false, true>"
BF32_V6 = "ftm_backward_bf_kernel<32, 64, 64, 64, true, false>"
BF32_F32 = "ftm_backward_bf_kernel<32, 64, 64, 64, false, false>"
BF32_SMALL = "ftm_backward_bf_kernel<32, 32, 64, 128, false, false>"
F32_BIG = "ftm_backward_kernel<64, 64, 64, 64, 64, 64>"
F32_MID = "ftm_backward_kernel<32, 64, 128, 64, 64, 64>"
F32_SMALL = "ftm_backward_kernel<32, 64, 128, 32, 64, 128>"
REACHABLE = {BF64_V6, BF64_F32, BF64_SMALL, BF32_V6, BF32_F32, BF32_SMALL, F32_BIG, F32_MID, F32_SMALL}

# (B, fps, Gh, Gw, F, L1), class, kernel under (defaults, NNUE_FTM_BF_WM=32, NNUE_FTM_BF16=0).  direct = min(F - 1, P).
ROWS = (
    # B % 64 = 8, P = 4048 (% 64 = 16), L1 % 64 = 56, clamp sink (P > F - 1): 224 + 256 tiles
    ((200, 8, 23, 22, 2000, 440), "big", (BF64_V6, BF32_V6, F32_BIG)),
    ((200, 8, 23, 22, 2000, 444), "big", (BF64_F32, BF32_F32, F32_BIG)),  # L1 % 8 = 4: f32 value tiles
    # table larger than the map (direct = P, 951 rows the map cannot reach): 192 + 256 = 448 tiles, the threshold itself
    ((200, 8, 23, 22, 5000, 184), "big", (BF64_V6, BF32_V6, F32_BIG)),
    ((193, 8, 23, 22, 1501, 512), "big", (BF64_V6, BF32_V6, F32_BIG)),    # one row in the last row tile; L1 % 128 == 0: the rider
    # P = 3240: the value plan alone is 32 x 64 (5 x 51 = 255 tiles of 64 rows), the pair is big all the same (224 + 255)
    ((257, 4, 27, 30, 2000, 440), "big", (BF64_V6, BF32_V6, F32_BIG)),
    ((200, 8, 23, 22, 2000, 312), "mid", (BF64_V6, BF32_V6, F32_MID)),    # 160 + 256 tiles
    ((200, 8, 23, 22, 2000, 316), "mid", (BF64_F32, BF32_F32, F32_MID)),
    ((200, 8, 23, 22, 2000, 256), "mid", (BF64_V6, BF32_V6, F32_MID)),    # the rider
    ((130, 8, 10, 10, 800, 200), "small", (BF64_SMALL, BF32_SMALL, F32_SMALL)),
)
KNOBS = ("default", "wm32", "f32")
RIDER_ROWS = (ROWS[3], ROWS[7])
ROW_ID = lambda row: "x".join(map(str, row[0]))  # noqa: E731
STATIC_KNOBS = ("NNUE_FTM_SPLIT_BACKWARD",)
_CASES = {}


def test_rows_name_every_reachable_instantiation():
    assert {k for _, _, kernels in ROWS for k in kernels} == REACHABLE and len(REACHABLE) == 9


@pytest.fixture(autouse=True)
def per_call_knobs_unset(monkeypatch):
    if any(os.environ.get(k) for k in STATIC_KNOBS):
        pytest.skip("a knob that is read once per process forces another kernel family")
    for knob in ("NNUE_FTM_BF16", "NNUE_FTM_BF_WM", "NNUE_FTM_BF_BM"):
        monkeypatch.delenv(knob, raising=False)


def set_knob(monkeypatch, knob):
    if knob == "wm32":
        monkeypatch.setenv("NNUE_FTM_BF_WM", "32")
    elif knob == "f32":
        monkeypatch.setenv("NNUE_FTM_BF16", "0")


def geometry(shape):
    b, fps, gh, gw, f, l1 = shape
    p = fps * gh * gw
    return b, f, p, l1, min(f - 1, p)


# ------------------------------------------------------------------ the policy, without a GPU
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_host_queries_report_the_variant(row, knob, monkeypatch):
    shape, cls, kernels = row
    b, f, p, l1, direct = geometry(shape)
    set_knob(monkeypatch, knob)
    L = lib.load()
    kernel = kernels[KNOBS.index(knob)]
    six_plane = kernel in (BF64_V6, BF32_V6)
    assert six_plane == (knob != "f32" and cls != "small" and l1 % 8 == 0)
    assert L.nnue_ftm_uses_bf16(5, b, f, p, l1) == int(six_plane)
    assert L.nnue_ftm_uses_bf16(2, b, f, p, l1) == int(knob != "f32")
    assert lib.ftm_backward_cw_supported(b, f, p, l1, L2) == (l1 % 128 == 0)
    wm = {"default": 64, "wm32": 32, "f32": 64 if cls == "big" else 32}[knob]
    assert lib.ftm_backward_sq_count(b, f, p, l1) == -(-direct // wm) * -(-l1 // 64)
    # the shape's edges: ragged batch, two or more row tiles, tails on the value tiles' rows and columns
    assert b % 64 and b > 64 and p % 64 and (l1 % 64 or l1 % 128 == 0)


# ------------------------------------------------------------------ operands and float64 references
def wide(gen, *shape, span=20):  # random sign, exponent uniform in [-span, span], full 24-bit mantissa
    mant = 1.0 + torch.rand(*shape, generator=gen, dtype=torch.float64)
    e = torch.randint(-span, span + 1, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * mant * torch.exp2(e)).float()


def grid_map(gen, b, p, f):
    """+1 / -1 map (threshold 0): density 0.3 below row F - 1, sixteen positions per sample at or past it (or all there are)."""
    below = min(f - 1, p)
    act = torch.zeros(b, p, dtype=torch.bool)
    act[:, :below] = torch.rand(b, below, generator=gen) < 0.3
    if p > below:
        past = torch.rand(b, p - below, generator=gen).topk(min(16, p - below), dim=1).indices
        act[:, below:].scatter_(1, past, True)
    return act


def case(shape, regime):
    """Operands of a shape in one regime (grid | unit | randn | wide), their float64 references and the device copies; built
    once and shared by the knob settings, never modified."""
    if (shape, regime) in _CASES:
        return _CASES[shape, regime]
    b, f, p, l1, direct = geometry(shape)
    fps = shape[1]
    gen = torch.Generator().manual_seed(1000 * b + f + l1)
    q = lambda den, *size: torch.randint(-den, den + 1, size, generator=gen).float() / den  # noqa: E731
    if regime in ("grid", "unit"):
        # unit: d_out in {-1, 0, 1} (still on the 2^-6 grid) makes d_weight integer, so the squared-norm partials are exact too
        weight, d_out = q(64, f, l1), q(64 if regime == "grid" else 1, b, l1)
        conv_out, thr = grid_map(gen, b, p, f).float() * 2 - 1, torch.zeros(fps)
    elif regime == "randn":
        weight, d_out = torch.randn(f, l1, generator=gen) * 0.1, torch.randn(b, l1, generator=gen) / b
        conv_out, thr = torch.randn(b, p, generator=gen), torch.full((fps,), 0.52)  # density 0.3
    else:  # one active position per sample: distinct ones below the clamp sink, the last eight samples at or past row F - 1
        weight, d_out = wide(gen, f, l1), wide(gen, b, l1)
        pos = torch.cat([torch.randperm(f - 1, generator=gen)[:b - 8], f - 1 + torch.randperm(p - f + 1, generator=gen)[:8]])
        conv_out, thr = torch.full((b, p), -1.0), torch.zeros(fps)
        conv_out[torch.arange(b), pos] = 1.0
    conv_out = conv_out.reshape(b, *shape[1:4])
    _, d_w, d_b, d_v, n, sink = dense_reference(conv_out, thr, weight, torch.zeros(l1), d_out)
    active = (conv_out > thr.view(1, -1, 1, 1)).reshape(b, p)
    c = dict(ref_w=d_w, ref_b=d_b, ref_v=d_v.reshape(b, p), active=active.to(DEV), regime=regime, shape=shape)
    if regime in ("grid", "unit"):  # the float64 values are float32 numbers: equality is meaningful
        assert float(sink.max()) <= 16 and 0.25 < float(active[:, :direct].float().mean()) < 0.35
        for k in ("ref_w", "ref_b", "ref_v"):
            assert torch.equal(c[k].float().double(), c[k]), k
        assert float(c["ref_v"].abs().max()) < 2.0 ** 9
    if regime == "unit":  # integer squares whose sum over any 64 x 64 tile stays below 2^24: every partial is exact in any order
        sq = torch.zeros(-(-direct // 64) * 64, -(-l1 // 64) * 64, dtype=torch.float64)
        sq[:direct, :l1] = d_w[:direct] ** 2
        assert float(sq.view(sq.shape[0] // 64, 64, sq.shape[1] // 64, 64).sum((1, 3)).max()) < 2.0 ** 24
    if regime == "wide":
        c["pos"] = pos
    c.update(weight=weight.to(DEV), d_out=d_out.to(DEV))
    c["fm"] = lib.ftm_binarize(conv_out.to(DEV), thr.to(DEV), f, l1)
    assert torch.equal(c["fm"].n.cpu(), n) and torch.equal(c["fm"].sink.cpu(), sink)
    _CASES[shape, regime] = c
    return c


class Banded:
    """NaN-filled outputs as interior views (16-byte aligned) of NaN-filled buffers; the bands are 64 rows deep on either side, so a
    store of any tile row past the last row lands in one."""

    def __init__(self):
        self.bufs = []

    def __call__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        band = 64 * shape[-1] + 256
        assert band % 4 == 0
        buf = torch.full((n + 2 * band,), float("nan"), device=DEV)
        self.bufs.append((buf, band, n))
        return buf[band:band + n].view(shape)

    def untouched(self):
        return all(bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[band + n:]).all()) for buf, band, n in self.bufs)


def launch(c, **riders):
    """One lib.ftm_backward call into banded NaN-prefilled outputs: (d_weight, d_bias, d_conv_out)."""
    b, f, p, l1, _ = geometry(c["shape"])
    band = Banded()
    out = lib.ftm_backward(c["d_out"], c["weight"], c["fm"], d_weight=band(f, l1), d_bias=band(l1), dst=band(b, p), **riders)
    torch.cuda.synchronize()
    assert band.untouched(), "a guard band of d_weight / d_bias / d_conv_out was written"
    return out


def same_bits(xs, ys):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(xs, ys))


# ------------------------------------------------------------------ which kernel
def backward_kernels(c):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        launch(c)
    found = []
    for name in (e.name for e in prof.events()):
        at = max(name.find("ftm_backward_bf_kernel<"), name.find("ftm_backward_kernel<"))
        if at < 0:
            continue
        depth, end = 0, at
        for end in range(at, len(name)):
            depth += (name[end] == "<") - (name[end] == ">")
            if name[end] == ">" and depth == 0:
                break
        # (the value epilogue, a defaulted type argument, is not part of the expected strings)
        found.append(name[at:end + 1].replace(", (anonymous namespace)::ValEpi>", ">"))
    return found


@gpu
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_which_kernel_serves_the_call(row, knob, monkeypatch):
    shape, _, kernels = row
    set_knob(monkeypatch, knob)
    assert backward_kernels(case(shape, "grid")) == [kernels[KNOBS.index(knob)]]


# ------------------------------------------------------------------ the three outputs against float64
@gpu
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_grid_operands_equal_float64(row, knob, monkeypatch):
    """Exact regime: d_weight (all F rows: zeros where the map cannot reach, the sink row), d_bias and d_conv_out (zeros at the
    inactive positions included) equal the float64 value; a second call gives the same bits."""
    c = case(row[0], "grid")
    set_knob(monkeypatch, knob)
    d_w, d_b, d_v = launch(c)
    for name, got, ref in (("d_weight", d_w, c["ref_w"]), ("d_bias", d_b, c["ref_b"]), ("d_conv_out", d_v, c["ref_v"])):
        wrong = got.cpu().double() != ref  # (a NaN left from the prefill compares unequal)
        assert not bool(wrong.any()), f"{name}: {int(wrong.sum())} of {ref.numel()} elements differ from float64, first at {wrong.nonzero()[0].tolist()}"
    assert not bool(d_v[~c["active"]].any())
    assert same_bits(launch(c), (d_w, d_b, d_v))


@gpu
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_randn_operands_against_float64_and_the_two_launches(row, knob, monkeypatch):
    c = case(row[0], "randn")
    b, f, p, l1, direct = geometry(row[0])
    set_knob(monkeypatch, knob)
    d_w, d_b, d_v = launch(c)
    assert_close_grad(d_w, c["ref_w"], "d_weight", rtol=2e-5)
    assert_close_grad(d_b, c["ref_b"], "d_bias", rtol=2e-5)
    assert_close_grad(d_v, c["ref_v"], "d_conv_out", rtol=2e-5)
    assert not bool(d_v[~c["active"]].any()) and not bool(d_w[direct:f - 1].any())
    assert same_bits(launch(c), (d_w, d_b, d_v))
    s_w, s_b = lib.ftm_backward_weight(c["d_out"], c["fm"])
    s_v = lib.ftm_backward_values(c["d_out"], c["weight"], c["fm"])
    assert torch.equal(d_b, s_b)
    if knob == "f32":
        assert torch.equal(d_w, s_w) and torch.equal(d_v, s_v)
    else:
        assert_close_grad(d_w, s_w, "d_weight, merged vs stand-alone", rtol=2e-6)
        assert_close_grad(d_v, s_v, "d_conv_out, merged vs stand-alone", rtol=2e-6)
        assert torch.equal(d_v == 0, s_v == 0)


@gpu
@pytest.mark.parametrize("knob", KNOBS)
def test_wide_exponents_with_one_active_position(knob, monkeypatch):
    """Magnitudes from 2^-20 to 2^20, one active position per sample: d_conv_out there is weight[row] . d_out[b] (the six plane
    products must carry the full mantissa), d_weight[row] is d_out[b] bit for bit, every other row below the sink is zero."""
    shape = ROWS[0][0]
    c = case(shape, "wide")
    b, f, p, l1, direct = geometry(shape)
    set_knob(monkeypatch, knob)
    d_w, d_b, d_v = launch(c)
    assert_close_grad(d_v, c["ref_v"], "d_conv_out", rtol=2e-5)
    assert_close_grad(d_w, c["ref_w"], "d_weight", rtol=2e-5)
    assert_close_grad(d_b, c["ref_b"], "d_bias", rtol=2e-5)
    own = c["pos"][:b - 8].to(DEV)
    assert same_bits((d_w[own],), (c["d_out"][:b - 8],))
    rest = torch.ones(f - 1, dtype=torch.bool, device=DEV)
    rest[own] = False
    assert not bool(d_w[:f - 1][rest].any()) and not bool(d_v[~c["active"]].any())
    assert same_bits(launch(c), (d_w, d_b, d_v))


# ------------------------------------------------------------------ what rides in those launches
def rider_operands(c, regime):
    """ft [B, L1], d_z1 [B, L2] and the float64 pairwise block l0 of ft; on grids (ft k / 16 in [0, 1], d_z1 k / 64 in [-1, 1]) in
    the exact regime, where d_z1^T l0 sums <= 200 multiples of 2^-14 below 1."""
    b, _, _, l1, _ = geometry(c["shape"])
    gen = torch.Generator().manual_seed(b + l1)
    if regime == "unit":
        ft = torch.randint(0, 17, (b, l1), generator=gen).float() / 16
        d_z1 = torch.randint(-64, 65, (b, L2), generator=gen).float() / 64
    else:
        ft, d_z1 = torch.rand(b, l1, generator=gen), torch.randn(b, L2, generator=gen) / b
    x = ft.double()
    l0 = torch.cat([x[:, :l1 // 2] * x[:, l1 // 2:], x[:, :l1 // 2]], dim=1)
    return ft, d_z1, l0


def check_d_w1(got, ref, regime, what):
    if regime == "unit":
        assert torch.equal(ref.float().double(), ref)
        assert torch.equal(got.cpu().double(), ref), f"{what}: {int((got.cpu().double() != ref).sum())} elements differ from float64"
    else:
        assert_close_grad(got, ref, what)


RIDER_KNOBS = ("default", "f32")


@gpu
@pytest.mark.parametrize("regime", ("unit", "randn"))
@pytest.mark.parametrize("knob", RIDER_KNOBS)
@pytest.mark.parametrize("row", RIDER_ROWS, ids=ROW_ID)
def test_rider_and_squared_norm_partials(row, knob, regime, monkeypatch):
    """d_w1 = d_z1^T l0 and the per-tile squared norms in the launch of the 64-row variants: both against float64, the launch's
    own outputs bitwise what they are alone, nothing written past either buffer."""
    c = case(row[0], regime)
    b, f, p, l1, direct = geometry(row[0])
    set_knob(monkeypatch, knob)
    assert lib.ftm_backward_cw_supported(b, f, p, l1, L2)
    plain = launch(c)
    ft, d_z1, l0 = rider_operands(c, regime)
    n_sq = lib.ftm_backward_sq_count(b, f, p, l1)
    band = Banded()
    d_w1, sq = band(L2, l1), torch.full((n_sq + 8,), float("nan"), device=DEV)
    got = launch(c, ft=ft.to(DEV), d_z1=d_z1.to(DEV), d_w1=d_w1, sq_partial=sq)
    assert band.untouched(), "a guard band of d_w1 was written"
    assert same_bits(got, plain)
    check_d_w1(d_w1, d_z1.double().t() @ l0, regime, "d_w1 (rider)")
    assert bool(torch.isfinite(sq[:n_sq]).all()) and bool(torch.isnan(sq[n_sq:]).all())
    want, total = float((got[0][:direct].double() ** 2).sum()), float(sq[:n_sq].double().sum())
    if regime == "unit":
        assert total == want == float((c["ref_w"][:direct] ** 2).sum())
    else:
        assert abs(total - want) <= 1e-5 * want
    d_w1_again = torch.full_like(d_w1, float("nan"))
    sq_again = torch.full_like(sq, float("nan"))
    launch(c, ft=ft.to(DEV), d_z1=d_z1.to(DEV), d_w1=d_w1_again, sq_partial=sq_again)
    assert same_bits((d_w1_again, sq_again[:n_sq]), (d_w1, sq[:n_sq]))


@gpu
@pytest.mark.parametrize("regime", ("unit", "randn"))
@pytest.mark.parametrize("knob", RIDER_KNOBS)
@pytest.mark.parametrize("row", RIDER_ROWS, ids=ROW_ID)
def test_bucketed_rider(row, knob, regime, monkeypatch):
    """K = 3 layer stacks, the middle one empty: d_w1[k] is the float64 product over bucket k's samples only, the empty bucket's
    slab is zero, and the grouped rows past the last segment (NaN here) are never read."""
    c = case(row[0], regime)
    b, f, p, l1, direct = geometry(row[0])
    set_knob(monkeypatch, knob)
    plain = launch(c)
    ft, d_z1, l0 = rider_operands(c, regime)
    bucket = 2 * (torch.arange(b) % 3 == 0).to(torch.int32)  # a third of the batch in bucket 2, the rest in bucket 0
    plan = lib.bucket_group(bucket.to(DEV), 0, 3)
    rows, seg = plan.rows.cpu().long(), plan.seg.cpu().tolist()
    assert seg[1] == seg[2] and 0 < seg[1] < seg[3] <= plan.tiles * 16 - 16  # bucket 1 is empty; whole tiles lie past the last segment
    member = rows >= 0
    grouped = []
    for t in (ft, d_z1):  # grouped-row order: a segment's padding rows are zero, as the classifier step leaves them
        g = torch.full((plan.tiles * 16, t.shape[1]), float("nan"))
        g[:seg[3]] = 0.0
        g[member] = t[rows[member]]
        grouped.append(g.to(DEV))
    band = Banded()
    d_w1 = band(3, L2, l1)
    got = launch(c, ft=grouped[0], d_z1=grouped[1], d_w1=d_w1, buckets=plan)
    assert band.untouched(), "a guard band of d_w1 was written"
    assert same_bits(got, plain)
    for k in range(3):
        mine = bucket == k
        check_d_w1(d_w1[k], d_z1[mine].double().t() @ l0[mine], regime, f"d_w1[{k}]")
    assert not bool(d_w1[1].any())
