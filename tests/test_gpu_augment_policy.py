"""nnue_load_batch_policy on the GPU: the medium policy and the resize against the float64 restatement
(tests/augment_reference.py, pinned on the CPU by test_augment_reference.py), the policy's statistics, the identities that
tie it to nnue_load_batch, reproducibility, and the way into the trainer.  ``-m gpu``.

The bar of the comparisons is 0.02 uint8 levels (0.02 / (255 std_c) after Normalize), derived, not measured: a float32
coordinate at <= 224 px is off by <= 1.5e-5 px against a gradient of <= 255 levels / px (4e-3 levels), some 30 float32
operations on values <= 255 add 5e-4 levels, and the bar is about four times their sum."""
import numpy as np
import pytest
import torch

import augment_reference as ar
from nnue_hip import lib
from nnue_hip.input_pipeline import GpuImageDataset, dataset_from_config, train_epoch

pytestmark = pytest.mark.gpu

BAR_LEVELS = 0.02
BAR = (BAR_LEVELS / (255.0 * ar.STD)).reshape(3, 1, 1)


def levels(err):
    """|difference| of normalised CHW images, in uint8 levels."""
    return np.abs(err) * (255.0 * ar.STD).reshape(3, 1, 1)


def run(images, labels, augment, out_hw=None, seed=0, indices=None, steps=1):
    ds = GpuImageDataset(images, labels, augment=augment, out_hw=out_hw, seed=seed)
    idx = torch.arange(len(ds), device="cuda") if indices is None else torch.as_tensor(indices, device="cuda")
    params = torch.zeros(idx.numel(), lib.load_batch_params_count(), device="cuda")
    for _ in range(steps):
        out, lab = ds.batch(idx, params_out=params)
    return out.cpu().numpy().astype(np.float64), params.cpu().numpy().astype(np.float64), lab.cpu().numpy()


@pytest.mark.parametrize("case", range(len(ar.CASES)))
def test_medium_policy_is_the_restatement(case):
    (h, w), (ho, wo) = ar.CASES[case]
    images, labels = ar.case_dataset(case)
    out, recs, lab = run(images, labels, "medium", (ho, wo), seed=ar.CASE_SEED)
    assert out.shape == (ar.CASE_IMAGES, 3, ho, wo) and lab.tolist() == labels.tolist()
    missing = [k for k, v in ar.coverage(recs).items() if not v]
    assert not missing, f"never fired: {missing}"
    tol = ar.record_tolerance(h, w, ho, wo)
    worst = worst_rec = 0.0
    left_out = hsv_pixels = 0
    for i in range(ar.CASE_IMAGES):
        own = ar.medium_record(ar.CASE_SEED, 1, i, h, w, ho, wo)  # the device's record against this side's own draw
        d = np.abs(recs[i] - own)
        worst_rec = max(worst_rec, float((d / np.maximum(tol, 1e-30))[tol > 0].max()))
        assert np.all(d <= tol), f"image {i}: record differs at slots {np.nonzero(d > tol)[0].tolist()}: {recs[i]} vs {own}"
        ref, ill = ar.medium_image(images[i], recs[i], ar.base_of(ar.CASE_SEED, 1, i), ho, wo)  # evaluated from the device's record
        if int(recs[i, ar.R_FLAGS]) & ar.F_HSV:
            left_out, hsv_pixels = left_out + int(ill.sum()), hsv_pixels + ill.size
        err = np.where(ill[None], 0.0, out[i] - ref)
        worst = max(worst, float(levels(err).max()))
        assert np.all(np.abs(err) <= BAR), f"image {i} (flags {int(recs[i, 0])}): off by {levels(err).max():.3e} levels"
    print(f"case {case}: max |error| {worst:.3e} levels (bar {BAR_LEVELS}), record at {worst_rec:.2f} of its bound, "
          f"{left_out} of {hsv_pixels} HSV pixels left out")
    assert left_out <= 0.001 * hsv_pixels


def test_policy_statistics():
    rng = np.random.RandomState(7)
    images = rng.randint(0, 256, size=(ar.STATS_IMAGES, 8, 8, 3), dtype=np.uint8)
    _, recs, _ = run(images, np.zeros(ar.STATS_IMAGES, dtype=np.int64), "medium", seed=ar.STATS_SEED)
    ar.check_statistics(recs, 8, 8)


def test_identities():
    rng = np.random.RandomState(8)
    images, labels = rng.randint(0, 256, size=(200, 17, 23, 3), dtype=np.uint8), rng.randint(0, 10, size=200)
    dev_images, dev_labels = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda()
    idx = torch.randperm(200, device="cuda")
    params = torch.zeros(200, lib.load_batch_params_count(), device="cuda")
    # policy 1 and policy 0 at equal sizes are nnue_load_batch with and without augment, bit for bit
    for policy, augment in ((1, True), (0, False)):
        old, old_lab = lib.load_batch(dev_images, dev_labels, idx, augment, 5, 3)
        new, new_lab = lib.load_batch_policy(dev_images, dev_labels, idx, policy, 5, 3, params_out=params)
        assert torch.equal(old, new) and torch.equal(old_lab, new_lab), f"policy {policy}"
    flags = params[:, 0].cpu().numpy()
    assert np.all(flags == 0)
    lib.load_batch_policy(dev_images, dev_labels, idx, 1, 5, 3, params_out=params)
    flags = params[:, 0].cpu().numpy().astype(np.int64)
    assert set(np.unique(flags)) <= {0, 1, 16, 17, 256, 257, 272, 273} and len(np.unique(flags)) >= 6  # flip, b/c, dropout only
    # the dataset class takes the old entry point's results through either path
    a = GpuImageDataset(images, labels, augment="light", seed=5)
    b = GpuImageDataset(images, labels, augment=True, seed=5)
    assert torch.equal(a.batch(idx)[0], b.batch(idx, params_out=params)[0])
    # medium: an image on which no stage fired is policy 0, bit for bit
    plain, _ = lib.load_batch_policy(dev_images, dev_labels, idx, 0, 5, 3)
    medium, _ = lib.load_batch_policy(dev_images, dev_labels, idx, 2, 5, 3, params_out=params)
    untouched = (params[:, 0] == 0)
    assert int(untouched.sum()) >= 2 and int((~untouched).sum()) >= 100
    assert torch.equal(medium[untouched], plain[untouched])
    assert not torch.equal(medium[~untouched], plain[~untouched])
    # policy 0 with 32 -> 96 is the clamped bilinear resize (and 17 x 23 -> 9 x 40, down one way and up the other)
    for (h, w), (ho, wo) in (((32, 32), (96, 96)), ((17, 23), (9, 40))):
        imgs = rng.randint(0, 256, size=(6, h, w, 3), dtype=np.uint8)
        out, recs, _ = run(imgs, np.zeros(6, dtype=np.int64), False, (ho, wo))
        assert np.all(recs[:, 0] == 0)
        worst = 0.0
        for i in range(6):
            err = out[i] - ar.resize_image(imgs[i], ho, wo)
            worst = max(worst, float(levels(err).max()))
            assert np.all(np.abs(err) <= BAR)
        print(f"resize {h}x{w} -> {ho}x{wo}: max |error| {worst:.3e} levels")


def test_reproducibility():
    rng = np.random.RandomState(9)
    images, labels = rng.randint(0, 256, size=(64, 20, 20, 3), dtype=np.uint8), rng.randint(0, 10, size=64)
    a = GpuImageDataset(images, labels, augment="medium", out_hw=(24, 18), seed=3)
    b = GpuImageDataset(images, labels, augment="medium", out_hw=(24, 18), seed=3)
    idx = torch.arange(64, device="cuda")
    x1 = a.batch(idx)[0]
    assert torch.equal(x1, b.batch(idx)[0])            # same seed, same step -> the same tensor
    x2 = a.batch(idx)[0]
    assert not torch.equal(x2, x1)                      # the next visit of the same samples: new draws
    assert not torch.equal(GpuImageDataset(images, labels, augment="medium", out_hw=(24, 18), seed=4).batch(idx)[0], x1)
    # neither the position in the batch nor B matters: (seed, step, dataset index) decide
    perm = torch.randperm(64, device="cuda")
    assert torch.equal(b.batch(perm)[0], x2[perm])      # b's second visit, shuffled
    few = torch.tensor([41, 7, 7, 63], device="cuda")
    c = GpuImageDataset(images, labels, augment="medium", out_hw=(24, 18), seed=3)
    assert torch.equal(c.batch(few)[0], x1[few])


def small_model():
    import nnue
    torch.manual_seed(0)
    return nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).cuda()


def test_medium_epoch_in_place_equals_copy_feeding():
    from nnue_hip.trainer import NnueTrainer
    rng = np.random.RandomState(10)
    images, labels = rng.randint(0, 256, size=(64 * 5 + 9, 24, 24, 3), dtype=np.uint8), rng.randint(0, 10, size=64 * 5 + 9)
    models, sums = [], []
    for mode in ("sequential", "in_place"):
        model = small_model()
        ds = GpuImageDataset(images, labels, augment="medium", out_hw=(32, 32), seed=5)
        assert ds.image_hw == (24, 24) and ds.output_hw == (32, 32)
        tr = NnueTrainer(model, 64, ds.output_hw, lr=0.01, momentum=0.9, input_slots=2)
        loader = ds.loader(64, shuffle=True, generator=torch.Generator().manual_seed(11))
        if mode == "sequential":
            losses = [float(tr.step(x, y)) for x, y in loader]
            total, n = sum(losses), len(losses)
            assert all(np.isfinite(losses))
        else:
            s, n = train_epoch(tr, loader)
            total = float(s)
        assert n == 6 and np.isfinite(total)
        models.append(model)
        sums.append(total)
    assert abs(sums[0] - sums[1]) <= 1e-4 * abs(sums[0])
    for (k, p), (_, q) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert float((p - q).detach().abs().max()) <= 1e-5 * max(1.0, float(q.detach().abs().max())), k


def test_run_training_from_config_loaders(tmp_path):
    from nnue_hip import train_loop
    from test_train_loop import write_config
    cfg = train_loop.load_config(write_config(tmp_path, opt="sgd", lr=0.02, epochs=2))
    cfg.use_augmentation = True  # augmentation_strength is left unset: "medium", the reference's default
    rng = np.random.RandomState(0)
    labels = rng.randint(0, 10, size=200)
    images = np.clip(rng.randint(0, 120, size=(200, 24, 24, 3)) + labels[:, None, None, None] * 12, 0, 255).astype(np.uint8)
    train_ds = dataset_from_config(cfg, images[:135], labels[:135], train=True, seed=2)
    val_ds = dataset_from_config(cfg, images[135:], labels[135:], train=False)
    assert train_ds.augment == "medium" and val_ds.augment is False and train_ds.output_hw == val_ds.output_hw == (32, 32)
    torch.manual_seed(0)
    res = train_loop.run_training(cfg, train_ds.loader(16, shuffle=True), val_ds.loader(16), checkpoint_dir=tmp_path / "ckpt",
                                  log=lambda line: None)
    assert res.steps == 2 * 9 and len(res.history) == 2  # 8 full batches and one of 7, twice
    assert all(np.isfinite(row["train/epoch_loss"]) and np.isfinite(row["val/loss"]) for row in res.history)
    with pytest.raises(ValueError, match="heavy"):
        GpuImageDataset(images, labels, augment="heavy")
