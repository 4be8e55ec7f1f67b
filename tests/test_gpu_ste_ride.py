"""The STE / conv-weight gradient's first stage riding in the merged FeatureTransformer backward launch (ValSteEpi):
the value tiles' partials give the same d_thr / d_weight as nnue_ste_conv_backward on the same d_conv_out, the trainer
takes the ride at the CIFAR shapes, stays deterministic, and NNUE_FTM_RIDE_STE=0 keeps the STE launch.  ``-m gpu``."""
import os

import pytest
import torch

import nnue
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
