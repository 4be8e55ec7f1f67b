"""nnue_mix_batch (batch-level mixup / CutMix, in place, sample i with B-1-i) and GpuImageDataset.mixed_batch.  ``-m gpu``.

* mixup against float64: |d| <= 3 U (|x_i| + |x_j|) -- two products and a sum (U = 2^-24).
* CutMix bitwise against an index expression in torch: boxes that touch each border, an empty box, the whole image.
* labels_b_out, lam_out and mode 0 are exact; for odd B the middle sample keeps itself.
* mixed_batch is reproducible in (seed, step, indices) and equals batch followed by mix_batch with mix_draw's values.
"""
import numpy as np
import pytest
import torch

from nnue_hip import lib as hip
from nnue_hip.input_pipeline import GpuImageDataset, mix_draw

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
BATCHES = (1, 2, 7, 64)
SIZES = ((5, 7), (32, 32))


def make(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, H, W, generator=g) * 2, torch.randint(0, 10, (B,), generator=g)


def bits(t):
    return t.contiguous().view(torch.int32)


def run(images, labels, mode, lam=1.0, box=(0, 0, 0, 0)):
    x = images.to(DEV).clone()
    labels_b, lam_out = hip.mix_batch(x, labels.to(DEV), mode, lam, box)
    torch.cuda.synchronize()
    return x.cpu(), labels_b.cpu(), lam_out.cpu()


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_mixup_against_float64(B, H, W):
    images, labels = make(B, H, W, seed=B + H)
    for lam in (0.0, 0.3, 1.0, 0.8125):
        got, labels_b, lam_out = run(images, labels, 1, lam)
        x64 = images.double()
        lam32 = float(np.float32(lam))
        one_minus = float(np.float32(1.0) - np.float32(lam))  # the kernel's 1 - lam is a float32 operation
        ref = lam32 * x64 + one_minus * x64.flip(0)
        bound = 3 * U * (x64.abs() + x64.flip(0).abs())
        if B % 2:  # the middle sample keeps itself, bit for bit
            ref[B // 2], bound[B // 2] = x64[B // 2], 0.0
        assert bool(((got.double() - ref).abs() <= bound).all()), (lam, float(((got.double() - ref).abs() - bound).max()))
        assert torch.equal(labels_b, labels.flip(0))
        assert torch.equal(bits(lam_out), bits(torch.full((B,), lam, dtype=torch.float32)))


def boxes(H, W):
    return [(0, 0, 2, 3), (H - 2, W - 3, 2, 3), (0, W - 1, H, 1), (H - 1, 0, 1, W), (1, 2, 0, 3), (1, 2, 3, 0), (0, 0, H, W), (1, 1, H - 2, W - 2)]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_cutmix_is_a_bitwise_swap_inside_the_box(B, H, W):
    images, labels = make(B, H, W, seed=3 * B + W)
    for y0, x0, hh, hw in boxes(H, W):
        got, labels_b, lam_out = run(images, labels, 2, 0.5, (y0, x0, hh, hw))
        ref = images.clone()
        ref[:, :, y0:y0 + hh, x0:x0 + hw] = images.flip(0)[:, :, y0:y0 + hh, x0:x0 + hw]
        assert torch.equal(bits(got), bits(ref)), (y0, x0, hh, hw)
        assert torch.equal(labels_b, labels.flip(0))
        want = np.float32(H * W - hh * hw) / np.float32(H * W)
        assert torch.equal(bits(lam_out), bits(torch.full((B,), float(want), dtype=torch.float32))), (y0, x0, hh, hw)


@pytest.mark.parametrize("B", BATCHES)
def test_mode_0_leaves_the_images_and_pairs_the_labels(B):
    images, labels = make(B, 5, 7, seed=B)
    got, labels_b, lam_out = run(images, labels, 0)
    assert torch.equal(bits(got), bits(images)) and torch.equal(labels_b, labels.flip(0))
    assert torch.equal(lam_out, torch.ones(B))


def test_a_view_that_is_not_16_byte_aligned_takes_the_scalar_form():
    images, labels = make(4, 32, 32, seed=9)
    base = torch.zeros(images.numel() + 1, device=DEV)
    x = base[1:].view(images.shape)
    x.copy_(images)
    assert x.data_ptr() % 16 == 4
    hip.mix_batch(x, labels.to(DEV), 2, 0.5, (3, 5, 10, 9))
    ref = images.clone()
    ref[:, :, 3:13, 5:14] = images.flip(0)[:, :, 3:13, 5:14]
    assert torch.equal(bits(x.cpu()), bits(ref)) and float(base[0]) == 0.0


def test_bad_arguments_are_refused():
    images, labels = make(4, 5, 7, seed=1)
    x, y = images.to(DEV), labels.to(DEV)
    for kw in (dict(mode=3), dict(mode=1, lam=1.5), dict(mode=1, lam=-0.1), dict(mode=2, box=(0, 0, 6, 1)), dict(mode=2, box=(4, 0, 2, 1)),
               dict(mode=2, box=(0, 5, 1, 3)), dict(mode=2, box=(-1, 0, 1, 1))):
        with pytest.raises(hip.NnueHipError):
            hip.mix_batch(x, y, kw["mode"], kw.get("lam", 0.5), kw.get("box", (0, 0, 0, 0)))
    with pytest.raises(ValueError):
        hip.mix_batch(x, y, 0, labels_b_out=y)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), images)


def dataset(mixup, cutmix, seed=5, n=40):
    g = torch.Generator().manual_seed(11)
    return GpuImageDataset(torch.randint(0, 256, (n, 8, 12, 3), dtype=torch.uint8, generator=g), torch.randint(0, 10, (n,), generator=g),
                           device=DEV, augment="light", seed=seed, mixup_alpha=mixup, cutmix_alpha=cutmix)


def test_mixed_batch_is_reproducible_and_is_batch_then_mix_batch():
    idx = torch.tensor([3, 9, 1, 30, 22, 7, 7], device=DEV)
    a, b, plain = dataset(0.4, 1.0), dataset(0.4, 1.0), dataset(0.0, 0.0)
    modes = set()
    for _ in range(12):
        ra, rb = a.mixed_batch(idx), b.mixed_batch(idx)
        for ta, tb in zip(ra, rb):
            assert torch.equal(ta, tb)
        images, labels = plain.batch(idx)
        assert plain.step == a.step
        mode, lam, y0, x0, hh, hw = mix_draw(a.seed, a.step, 0.4, 1.0, 8, 12)
        modes.add(mode)
        labels_b, lam_out = hip.mix_batch(images, labels, mode, lam, (y0, x0, hh, hw))
        for got, ref in zip(ra, (images, labels, labels_b, lam_out)):
            assert torch.equal(got, ref)
        assert torch.equal(ra[2], ra[1].flip(0))
    assert modes == {1, 2}
    c = dataset(0.4, 1.0, seed=6)
    c.step = a.step - 1
    assert not torch.equal(c.mixed_batch(idx)[0], ra[0])  # another seed, another draw


def test_soft_out_receives_the_second_labels_and_weights():
    ds = dataset(1.0, 0.0)
    idx = torch.arange(6, device=DEV)
    out, labels_out = torch.empty(6, 3, 8, 12, device=DEV), torch.empty(6, dtype=torch.int64, device=DEV)
    soft = (torch.full((6,), -1, dtype=torch.int64, device=DEV), torch.ones(6, device=DEV))
    images, labels, labels_b, lam = ds.mixed_batch(idx, out=out, labels_out=labels_out, soft_out=soft)
    assert images.data_ptr() == out.data_ptr() and labels_b.data_ptr() == soft[0].data_ptr() and lam.data_ptr() == soft[1].data_ptr()
    assert torch.equal(soft[0], labels_out.flip(0))
    assert float(soft[1][0]) == float(np.float32(mix_draw(ds.seed, ds.step, 1.0, 0.0, 8, 12)[1]))
