"""The STE / conv-weight gradient's first stage riding in the merged FeatureTransformer backward launch (ValSteEpi):
the value tiles' partials give the same d_thr / d_weight as nnue_ste_conv_backward on the same d_conv_out, the trainer
takes the ride at the CIFAR shapes, stays deterministic, and NNUE_FTM_RIDE_STE=0 keeps the STE launch.  ``-m gpu``.

The ride against float64 (cases, reference and check in tests/ste_ride_cases.py): the launch restated in float64 from its own
inputs, held to 2e-5 max|ref| per tensor for d_thr, d_w and d_conv_out at fifteen shapes the policy takes (windows leaving the
image at the bottom and right, H != W, ragged grids and batches, F below P), from the pixels and from the im2col patches; the
value regimes (thresholds at -1e6 and +1e6, images x 50, NaN / 0xFF guard bands round every operand); both 64 x 64 ValSteEpi
instantiations in one child process with NNUE_FTM_RIDE_STE_V64=1; the bucketed entry point and a K = 4 trainer.  Each float64
case prints its ratios max|got - ref| / max|ref| (``-s``), the child its worst one."""
import os
import subprocess
import sys

import pytest
import torch

import nnue
import ste_ride_cases as cases
from conftest import assert_close_grad
from nnue_hip import lib
from nnue_hip.trainer import NnueTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ste_case(b, image, fps, grid, l1, stride=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(b, 3, image, image, generator=g).to(DEV)
    w = (0.3 * torch.randn(fps, 3, 3, 3, generator=g)).to(DEV)
    thr = (0.1 * torch.randn(fps, generator=g)).to(DEV)
    f = grid * grid * fps
    conv_out, fm = lib.ftm_conv_binarize(images, w, thr, stride, f, l1)
    d_out = torch.randn(b, l1, generator=g).to(DEV)
    weight = (0.05 * torch.randn(f, l1, generator=g)).to(DEV)
    return images, conv_out, thr, fm, d_out, weight


# C2 (32 x 64 value tiles) and a batch that ends inside a tile
@pytest.mark.parametrize("b,l1", ((512, 1024), (40, 256)))
def test_fused_partials_give_the_ste_kernels_gradients(b, l1):
    images, conv_out, thr, fm, d_out, weight = ste_case(b, 32, 8, 10, l1)
    chunks = lib.ftm_backward_ste_chunks(b, fm.num_rows, fm.positions, l1, 32, 32, 3)
    assert chunks > 0, "the CIFAR shapes take the ride"
    part = torch.full((8 * 28 * chunks,), float("nan"), device=DEV)
    ref_w, ref_b, ref_v = lib.ftm_backward(d_out, weight, fm)
    d_w, d_b, d_v = lib.ftm_backward(d_out, weight, fm, dst=torch.empty_like(ref_v), ste=(images, conv_out, thr, 3, part))
    torch.cuda.synchronize()
    # the value tiles' other outputs are untouched by the epilogue
    assert torch.equal(d_w, ref_w) and torch.equal(d_b, ref_b) and torch.equal(d_v, ref_v)
    ref_thr, ref_wt = lib.ste_conv_backward(images, conv_out, thr, ref_v, 3, stages=3)
    sums = part.view(8 * 28, chunks).double().sum(1).view(8, 28)
    assert torch.isfinite(sums).all(), "every partial slot is written"
    assert_close_grad(sums[:, :27].float().view(8, 3, 3, 3), ref_wt, "d_weight", rtol=1e-4)
    assert_close_grad((-sums[:, 27]).float(), ref_thr, "d_thr", rtol=1e-4)
    # without dst the value gradient is not stored
    _, _, none = lib.ftm_backward(d_out, weight, fm, ste=(images, conv_out, thr, 3, part))
    assert none is None


@pytest.mark.parametrize("b,image,stride,grid", ((512, 32, 3, 10), (32, 64, 4, 16)))
def test_partials_from_patches_are_bitwise_those_from_pixels(b, image, stride, grid):
    images, conv_out, thr, fm, d_out, weight = ste_case(b, image, 8, grid, 256, stride=stride, seed=2)
    gh = (image - 1) // stride + 1
    patches = torch.empty((27, b * gh * gh), device=DEV)
    w = (0.3 * torch.randn(8, 3, 3, 3, generator=torch.Generator().manual_seed(2))).to(DEV)
    conv_out, fm = lib.ftm_conv_binarize(images, w, thr, stride, fm.num_rows, 256)
    conv_p, fm_p = lib.ftm_conv_binarize(images, w, thr, stride, fm.num_rows, 256, patches=patches)
    assert torch.equal(conv_out, conv_p) and torch.equal(fm.bits, fm_p.bits)
    chunks = lib.ftm_backward_ste_chunks(b, fm.num_rows, fm.positions, 256, image, image, stride)
    assert chunks > 0
    part = torch.full((8 * 28 * chunks,), float("nan"), device=DEV)
    part_p = torch.full_like(part, float("nan"))
    lib.ftm_backward(d_out, weight, fm, ste=(images, conv_out, thr, stride, part))
    lib.ftm_backward(d_out, weight, fm_p, ste=(images, conv_p, thr, stride, part_p, patches))
    torch.cuda.synchronize()
    assert torch.isfinite(part).all() and torch.equal(part, part_p)


def test_shapes_the_epilogue_does_not_take_fall_back():
    # fps != 8: the 224x224 shape, four channels on the CIFAR grid
    assert lib.ftm_backward_ste_chunks(128, 32 * 32 * 64, 32 * 32 * 64, 1024, 224, 224, 7) == 0
    assert lib.ftm_backward_ste_chunks(512, 400, 484, 1024, 32, 32, 3) == 0
    assert lib.ftm_backward_ste_chunks(512, 800, 968, 1024, 32, 32, 3) > 0
    # C3 keeps the STE launch by default (its 64 x 64 value tiles lose with the epilogue)
    if os.environ.get("NNUE_FTM_RIDE_STE_V64", "0") == "0":
        assert lib.ftm_backward_ste_chunks(1024, 800, 968, 1024, 32, 32, 3) == 0


def c2_trainer(seed=0):
    torch.manual_seed(seed)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 1024, 128, 32, num_classes=10).to(DEV)
    return model, NnueTrainer(model, 512, (32, 32), lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0, use_graph=True)


def run_steps(tr, n=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        tr.step(torch.randn(512, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (512,), generator=g).to(DEV))
    torch.cuda.synchronize()
    return tr.flat_params.clone()


def test_trainer_rides_and_two_runs_are_bitwise_equal(monkeypatch):
    monkeypatch.delenv("NNUE_FTM_RIDE_STE", raising=False)
    _, a = c2_trainer()
    _, b = c2_trainer()
    assert a.ride_ste and b.ride_ste
    pa, pb = run_steps(a), run_steps(b)
    assert torch.equal(pa, pb), "the fused path is deterministic (no atomics)"


def test_knob_off_keeps_the_ste_launch_and_agrees(monkeypatch):
    monkeypatch.setenv("NNUE_FTM_RIDE_STE", "0")
    _, off = c2_trainer()
    assert not off.ride_ste
    p_off = run_steps(off, n=1)  # one step: both runs see the same forward (no threshold decision can differ)
    monkeypatch.setenv("NNUE_FTM_RIDE_STE", "1")
    _, on = c2_trainer()
    assert on.ride_ste
    p_on = run_steps(on, n=1)
    # the two paths sum the same products in another order: equal up to float32 summation error
    for k in ("visual_threshold", "conv.weight"):
        assert_close_grad(on.g[k], off.g[k], f"{k} gradient", rtol=1e-4)
    assert_close_grad(p_on, p_off, "parameters after one step", rtol=2e-4)


# ------------------------------------------------------------------ the ride against float64 (tests/ste_ride_cases.py)
def show(what, got):
    print(f"ratio {what}: " + " ".join(f"{k} {v:.2e}" for k, v in got.items()))


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_the_ride_against_float64(shape):
    """Pixels and patches, every slot written, d_conv_out, the launch's other outputs and a second run: cases.check_case."""
    assert cases.ste_chunks(shape) > 0, "a policy change must not empty this test"
    show(cases.shape_id(shape), cases.check_case(cases.build_case(shape)))


@pytest.mark.parametrize("shape", cases.REGIME_SHAPES, ids=cases.shape_id)
def test_thresholds_far_below_every_conv_output(shape):
    # every position active; s = 1 exactly, so the slope k s (1 - s) and with it d_thr are exactly 0 while d_w meets float64
    c = cases.build_case(shape, thr_fill=-1e6)
    assert bool(c.bits.all())
    show(cases.shape_id(shape) + " thr=-1e6", cases.check_case(c))
    part = cases.launch(c, dst=False)[0]
    d_thr, d_w = cases.partial_sums(part, cases.ste_chunks(shape))
    assert bool((d_thr == 0.0).all()), "d_thr is exactly 0 where the sigmoid is saturated"
    assert bool(d_w.any())


@pytest.mark.parametrize("shape", cases.REGIME_SHAPES, ids=cases.shape_id)
def test_thresholds_far_above_every_conv_output(shape):
    c = cases.build_case(shape, thr_fill=1e6)
    assert not bool(c.bits.any())
    cases.check_case(c)
    for patches in (False, True):
        part, _, _, d_v = cases.launch(c, patches=patches)
        assert bool((part == 0.0).all()) and bool((d_v == 0.0).all()), "no position active: every partial is exactly 0"


@pytest.mark.parametrize("shape", cases.REGIME_SHAPES, ids=cases.shape_id)
def test_images_scaled_by_50(shape):
    # conv outputs of standard deviation 0.3 * 50 * sqrt(27) = 78: 10 |conv_out - thr| passes 88, where __expf overflows, at
    # nine positions in ten (P(|x| > 8.8 / 78))
    c = cases.build_case(shape, image_scale=50.0)
    over = 10.0 * (c.conv_out - c.thr.view(1, -1, 1, 1)).abs() > 88.0
    assert float(over.float().mean()) > 0.5
    show(cases.shape_id(shape) + " x50", cases.check_case(c))  # finite and within the bar


@pytest.mark.parametrize("shape", cases.REGIME_SHAPES, ids=cases.shape_id)
def test_guard_bands(shape):
    cases.check_guard_bands(cases.build_case(shape))


# One child with the knob set runs cases.V64_SHAPES.  The limit is five times the child's duration with a floor of 120 s.
# CHILD_SECONDS is an estimate, not a measurement on an MI355X: importing torch and the library 5 s, the three float64
# references 3 s on the CPU, the launches themselves microseconds.  The floor decides up to 24 s.
CHILD_SECONDS = 10.0
CHILD_TIMEOUT = max(120.0, 5.0 * CHILD_SECONDS)


def test_the_64_row_value_tiles_against_float64():
    """Both 64 x 64 ValSteEpi instantiations (bf16 planes and, at L1 % 8 == 4, f32) in a fresh process: the knob is read once."""
    if "NNUE_FTM_RIDE_STE_V64" in os.environ:
        pytest.skip("NNUE_FTM_RIDE_STE_V64 is set: this process's policy is not the default one")
    # -s where this interpreter runs with it: the child imports the packages this process sees (the same torch), no others
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [cases.__file__]
    try:
        res = subprocess.run(cmd, env=dict(os.environ, NNUE_FTM_RIDE_STE_V64="1"), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:  # subprocess.run has killed the child; a hang is a finding like a signal
        pytest.exit(f"the 64-row value tiles' child hung ({CHILD_TIMEOUT:.0f} s): nothing more is started on this GPU\n{e.stdout}\n{e.stderr}", returncode=1)
    print(res.stdout)
    print(res.stderr, file=sys.stderr)
    if res.returncode < 0:  # a finding, not something to run again: nothing more is started on this GPU
        pytest.exit(f"the 64-row value tiles' child died of signal {-res.returncode}\n{res.stdout}\n{res.stderr}", returncode=1)
    assert res.returncode == 0, f"{res.stdout}\n{res.stderr}"
    assert res.stdout.count("\nok ") + res.stdout.startswith("ok ") == len(cases.V64_SHAPES)


# ------------------------------------------------------------------ the bucketed entry point and the bucketed trainer
def test_bucketed_entry_point_carries_the_ride():
    """nnue_ftm_backward_bucketed with buckets=, the d_w1 rider, sq_partial and ste= together, as the trainer calls it."""
    c = cases.build_case(cases.C2)
    b, _, _, stride, l1, f, p, _, _ = cases.geometry(cases.C2)
    K, l2 = 4, 128
    chunks, n_sq = cases.ste_chunks(cases.C2), lib.ftm_backward_sq_count(b, f, p, l1)
    assert chunks > 0 and n_sq > 0 and lib.ftm_backward_cw_supported(b, f, p, l1, l2)
    g = torch.Generator().manual_seed(5)
    plan = lib.bucket_group(torch.randint(0, K, (b,), generator=g).to(DEV, torch.int32), 0, K)
    rows = plan.tiles * 16
    ft, d_z1 = torch.rand(rows, l1, generator=g).to(DEV), (torch.randn(rows, l2, generator=g) / b).to(DEV)
    d = c.dev
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    bits = lambda t: t.view(torch.int32)  # noqa: E731  (bit patterns: slots nobody writes keep their NaN)

    def run(ste):
        d_w1, sq, part, d_v = nan(K, l2, l1), nan(n_sq), nan(8 * 28 * chunks), nan(b, p)
        d_w, d_b, _ = lib.ftm_backward(d["d_out"], d["weight"], c.fm_p, dst=d_v, ft=ft, d_z1=d_z1, d_w1=d_w1, sq_partial=sq, buckets=plan,
                                       ste=(d["images"], d["conv_p"], d["thr"], stride, part, d["patches"]) if ste else None)
        torch.cuda.synchronize()
        return part, (d_w, d_b, d_v, d_w1, sq)

    part, outs = run(True)
    _, plain = run(False)
    for name, got, want in zip(("d_weight", "d_bias", "d_conv_out", "d_w1", "sq_partial"), outs, plain):
        assert torch.equal(bits(got), bits(want)), f"{name} differs from the bucketed launch without ste="
    assert bool(torch.isfinite(outs[3]).all()) and bool(torch.isfinite(outs[4]).all())
    assert torch.equal(part, cases.launch(c, patches=True)[0]), "the partials are those of the unbucketed entry point"


def c2_bucketed_trainer(seed=0):
    torch.manual_seed(seed)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 1024, 128, 32, num_classes=10, num_ls_buckets=4, clip_activations=1.0)
    with torch.no_grad():
        model.conv.weight.abs_()  # with the per-sample offsets below the active counts, and so the buckets, spread out
    model = model.to(DEV)
    return model, NnueTrainer(model, 512, (32, 32), lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0, use_graph=True)


def run_spread_step(tr, seed=1):
    g = torch.Generator().manual_seed(seed)
    shift = torch.linspace(-1.6, 1.6, 512)[torch.randperm(512, generator=g)].view(512, 1, 1, 1)
    images = torch.randn(512, 3, 32, 32, generator=g) * (0.5 + torch.rand(512, 1, 1, 1, generator=g)) + shift
    tr.step(images.to(DEV), torch.randint(0, 10, (512,), generator=g).to(DEV))
    torch.cuda.synchronize()
    return tr.flat_params.clone()


def test_bucketed_trainer_rides_and_agrees_with_the_ste_launch(monkeypatch):
    monkeypatch.setenv("NNUE_FTM_RIDE_STE", "0")
    _, off = c2_bucketed_trainer()
    assert off.K == 4 and not off.ride_ste
    p_off = run_spread_step(off)  # one step: both runs see the same forward (no threshold decision can differ)
    assert off.bucket_plan.bucket.unique().numel() == 4, "every layer stack is populated"
    monkeypatch.setenv("NNUE_FTM_RIDE_STE", "1")
    _, on = c2_bucketed_trainer()
    assert on.K == 4 and on.ride_ste
    p_on = run_spread_step(on)
    assert torch.equal(on.bucket_plan.bucket, off.bucket_plan.bucket)
    for k in ("visual_threshold", "conv.weight"):
        assert_close_grad(on.g[k], off.g[k], f"{k} gradient", rtol=1e-4)
    assert_close_grad(p_on, p_off, "parameters after one step", rtol=2e-4)
