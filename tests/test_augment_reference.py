"""The float64 restatement of the input pipeline's policies (tests/augment_reference.py) pinned against independent code
-- scipy.ndimage for the warp and the blurs, colorsys for the colour space -- and the parts of the policy path that need
no GPU: argument validation of nnue_load_batch_policy, the ``augment=`` strings, ``dataset_from_config``'s defaults, and
that the seeds the GPU tests use cover what those tests assert.  CPU only."""
import colorsys
import ctypes
import types

import numpy as np
import pytest
import scipy.ndimage as ndi

import augment_reference as ar
from nnue_hip import input_pipeline, lib


def test_array_hash_is_the_integer_hash():
    rng = np.random.RandomState(0)
    z = rng.randint(0, 2 ** 63, size=50, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    assert [int(v) for v in ar.mix64_array(z)] == [ar.mix64(int(v)) for v in z]
    assert ar.mix64(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for state 0
    assert 0.0 <= ar.u01(ar.mix64(1)) < 1.0 and ar.u01(ar.MASK) == 1 - 2.0 ** -24


def test_warp_is_scipys_linear_map_coordinates():
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, size=(17, 23, 3)).astype(np.float64)
    ho, wo = 19, 13
    rec = np.zeros(ar.PARAMS)
    rec[[ar.R_FLAGS, ar.R_K, ar.R_ROT, ar.R_AFF_ROT, ar.R_AFF_SCALE, ar.R_TX, ar.R_TY]] = (
        ar.F_FLIP | ar.F_ROT90 | ar.F_ROTATE | ar.F_AFFINE, 1, 11.0, -7.0, 0.93, 1.1, -1.7)
    m = ar.compose_map(rec, 17, 23, ho, wo)
    oy, ox = np.meshgrid(np.arange(ho, dtype=np.float64), np.arange(wo, dtype=np.float64), indexing="ij")
    sy, sx = m[3] * ox + m[4] * oy + m[5], m[0] * ox + m[1] * oy + m[2]
    assert (sx < 0).any() and (sx > 23).any()  # the map leaves the source: the border rule is exercised
    got = ar.sample(img, m, ho, wo, True)
    for c in range(3):
        ref = ndi.map_coordinates(img[..., c], [sy, sx], order=1, mode="grid-constant", cval=0.0)
        assert np.abs(got[..., c] - ref).max() <= 1e-10
    got = ar.sample(img, m, ho, wo, False)
    for c in range(3):
        ref = ndi.map_coordinates(img[..., c], [np.clip(sy, 0, 16), np.clip(sx, 0, 22)], order=1, mode="nearest")
        assert np.abs(got[..., c] - ref).max() <= 1e-10


def test_map_composition():
    # the resize map is the identity at equal sizes, and each stage's map does what its name says
    assert np.array_equal(ar.resize_map(17, 23, 17, 23)[:2].reshape(6), [1, 0, 0, 0, 1, 0])
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, size=(6, 9, 3), dtype=np.uint8)
    plain = np.transpose((img.astype(np.float64) - ar.MEAN * 255) / (ar.STD * 255), (2, 0, 1))
    assert np.array_equal(ar.resize_image(img, 6, 9), plain)
    rec = np.zeros(ar.PARAMS)
    rec[ar.R_FLAGS] = ar.F_FLIP
    assert np.array_equal(ar.sample(img.astype(np.float64), ar.compose_map(rec, 6, 9, 6, 9), 6, 9, False), img[:, ::-1])
    sq = rng.randint(0, 256, size=(7, 7, 3)).astype(np.float64)
    for k in (1, 2, 3):  # quarter turns of a square are numpy's rot90
        rec[ar.R_FLAGS], rec[ar.R_K] = ar.F_ROT90, k
        assert np.abs(ar.sample(sq, ar.compose_map(rec, 7, 7, 7, 7), 7, 7, False) - np.rot90(sq, k)).max() <= 1e-9
    # an affine stage of angle 0 and scale 1 is a shift by (tx, ty); a rotation by t then by -t is the identity
    rec[:] = 0
    rec[[ar.R_FLAGS, ar.R_AFF_SCALE, ar.R_TX, ar.R_TY]] = (ar.F_AFFINE, 1.0, 2.0, -1.0)
    assert np.allclose(ar.compose_map(rec, 6, 9, 6, 9), [1, 0, -2, 0, 1, 1], atol=1e-12)
    rec[:] = 0
    rec[[ar.R_FLAGS, ar.R_ROT, ar.R_AFF_ROT, ar.R_AFF_SCALE]] = (ar.F_ROTATE | ar.F_AFFINE, 9.0, 9.0, 1.0)
    assert np.allclose(ar.compose_map(rec, 6, 9, 6, 9), [1, 0, 0, 0, 1, 0], atol=1e-12)
    # a non-square output: the quarter turn maps the rectangle onto itself (corners of the pixel grid to corners)
    rec[:] = 0
    rec[[ar.R_FLAGS, ar.R_K]] = (ar.F_ROT90, 1)
    m = ar.compose_map(rec, 5, 8, 5, 8)
    assert np.allclose([m[0] * -.5 + m[1] * -.5 + m[2], m[3] * -.5 + m[4] * -.5 + m[5]], [7.5, -.5], atol=1e-12)


def test_blurs_are_scipys_mirror_correlation():
    rng = np.random.RandomState(3)
    v = rng.rand(9, 12, 3) * 255
    for kind, sigma, direction in ((0, 0.0, 0), (1, 0.5, 0), (1, 1.7, 0), (1, 3.0, 0), (2, 0.0, 0), (2, 0.0, 1), (2, 0.0, 2), (2, 0.0, 3)):
        w = ar.blur_weights(kind, sigma, direction)
        assert abs(w.sum() - 1) <= 1e-12
        got = ar.blur(v, w)
        for c in range(3):
            assert np.abs(got[..., c] - ndi.correlate(v[..., c], w, mode="mirror")).max() <= 1e-10
    g = np.exp(-np.array([1., 0., 1.]) / (2 * 1.7 ** 2))
    assert np.allclose(ar.blur_weights(1, 1.7, 0), np.outer(g, g) / g.sum() ** 2)
    assert np.array_equal(ar.blur_weights(2, 0, 3) > 0, np.eye(3)[::-1] > 0) and np.array_equal(ar.blur_weights(2, 0, 2) > 0, np.eye(3) > 0)


def test_colour_space_is_colorsys():
    rng = np.random.RandomState(4)
    v = np.concatenate([rng.rand(500, 3) * 255, [[0, 0, 0], [255, 255, 255], [90, 90, 90], [255, 0, 0], [10, 200, 200]]])
    h, s, val = ar.rgb_to_hsv(v)
    ref = np.array([colorsys.rgb_to_hsv(*(p / 255.0)) for p in v])
    assert np.abs(h / 360 - ref[:, 0]).max() <= 1e-12 and np.abs(s - ref[:, 1]).max() <= 1e-12 and np.abs(val - ref[:, 2]).max() <= 1e-12
    assert h[-3] == 0 and s[-3] == 0  # greys: hue 0
    back = ar.hsv_to_rgb(h, s, val)
    assert np.abs(back - v).max() <= 1e-10
    ref_back = np.array([colorsys.hsv_to_rgb(a, b, c) for a, b, c in zip(h / 360, s, val)]) * 255
    assert np.abs(back - ref_back).max() <= 1e-10
    # the shifts: hue wraps, saturation and value clamp
    rec = np.zeros(ar.PARAMS)
    rec[[ar.R_FLAGS, ar.R_HUE, ar.R_SAT, ar.R_VAL]] = (ar.F_HSV, 10.0, -15.0, 10.0)
    out, spread = ar.point_chain(np.array([[250.0, 10.0, 20.0]]), rec)
    hh, ss, vv = colorsys.rgb_to_hsv(250 / 255, 10 / 255, 20 / 255)
    want = np.array(colorsys.hsv_to_rgb((hh + 20 / 360) % 1, ss - 15 / 255, min(1.0, vv + 10 / 255))) * 255
    assert np.abs(out[0] - want).max() <= 1e-10 and spread[0] == 240.0


def test_noise_field_is_standard_normal():
    z = ar.gaussian_field(ar.base_of(1, 2, 3), 64, 64)
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03 and np.abs(z).max() < 6
    assert not np.array_equal(z, ar.gaussian_field(ar.base_of(1, 2, 4), 64, 64))


def test_policy_entry_point_validates_before_launching():
    L = lib.load()
    assert L.nnue_load_batch_params_count() == ar.PARAMS > 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    call = L.nnue_load_batch_policy
    assert call(p, p, p, 2, 8, 8, 4, 8, 8, 3, 0, 0, p, p, None, None) == -1  # policy 3
    assert b"policy 3" in L.nnue_hip_last_error()
    assert call(p, p, p, 2, 8, 8, 4, 8, 8, -1, 0, 0, p, p, None, None) == -1
    for null in (0, 1, 2, 12, 13):  # images, labels, indices, out, labels_out
        args = [p, p, p, 2, 8, 8, 4, 8, 8, 2, 0, 0, p, p, None, None]
        args[null] = None
        assert call(*args) == -1
        assert b"null pointer" in L.nnue_hip_last_error()
    assert call(p, p, p, 2, 8, 8, 4, 0, 8, 2, 0, 0, p, p, None, None) == -1   # Ho <= 0
    assert call(p, p, p, 2, 8, 8, 4, 8, -3, 2, 0, 0, p, p, None, None) == -1  # Wo <= 0
    assert call(p, p, p, 0, 8, 8, 4, 8, 8, 2, 0, 0, p, p, None, None) == -1   # B <= 0
    assert call(p, p, p, 2, 8, 8, 4, 4096, 4096, 2, 0, 0, p, p, None, None) == -2  # Ho * Wo >= 2^24
    assert call(p, p, p, 2, 4096, 4096, 4, 8, 8, 2, 0, 0, p, p, None, None) == -2


def test_augment_strings():
    assert [input_pipeline.resolve_augment(a) for a in (False, None, True, "light", "medium")] == [0, 0, 1, 1, 2]
    assert lib.LOAD_POLICIES == {"none": 0, "light": 1, "medium": 2}
    with pytest.raises(ValueError, match="heavy"):
        input_pipeline.resolve_augment("heavy")
    for bad in ("strong", "", 2, 1.0):
        with pytest.raises(ValueError, match="expected False, True"):
            input_pipeline.resolve_augment(bad)
    assert input_pipeline.resolve_out_hw(None) is None and input_pipeline.resolve_out_hw(96) == (96, 96)
    assert input_pipeline.resolve_out_hw((19, 13)) == (19, 13)
    for bad in (0, (32, 0), (-1, 8), (8,), (8.5, 8)):
        with pytest.raises(ValueError, match="out_hw"):
            input_pipeline.resolve_out_hw(bad)
    images, labels = np.zeros((4, 8, 8, 3), dtype=np.uint8), np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match="heavy"):
        input_pipeline.GpuImageDataset(images, labels, device="cpu", augment="heavy")
    with pytest.raises(ValueError, match="out_hw"):
        input_pipeline.GpuImageDataset(images, labels, device="cpu", out_hw=(8, 0))
    ds = input_pipeline.GpuImageDataset(images, labels, device="cpu", augment="medium", out_hw=(12, 10))
    assert ds.image_hw == (8, 8) and ds.output_hw == (12, 10)
    assert input_pipeline.GpuImageDataset(images, labels, device="cpu").output_hw == (8, 8)


def test_dataset_from_config_defaults():
    images, labels = np.zeros((4, 24, 24, 3), dtype=np.uint8), np.zeros(4, dtype=np.int64)
    bare = types.SimpleNamespace()
    ds = input_pipeline.dataset_from_config(bare, images, labels, train=True, device="cpu")
    assert ds.augment == "medium" and ds.output_hw == (24, 24)  # the reference's defaults; no input_size: no resize
    assert input_pipeline.dataset_from_config(bare, images, labels, train=False, device="cpu").augment is False
    cfg = types.SimpleNamespace(use_augmentation=True, augmentation_strength="light", input_size=32, num_classes=10)
    ds = input_pipeline.dataset_from_config(cfg, images, labels, train=True, device="cpu", seed=9)
    assert ds.augment == "light" and ds.output_hw == (32, 32) and ds.image_hw == (24, 24) and ds.seed == 9
    val = input_pipeline.dataset_from_config(cfg, images, labels, train=False, device="cpu")
    assert val.augment is False and val.output_hw == (32, 32)  # evaluation batches are resized too, never augmented
    cfg.use_augmentation = False
    assert input_pipeline.dataset_from_config(cfg, images, labels, train=True, device="cpu").augment is False
    cfg.use_augmentation, cfg.augmentation_strength = True, "heavy"
    with pytest.raises(ValueError, match="heavy"):
        input_pipeline.dataset_from_config(cfg, images, labels, train=True, device="cpu")
    cfg.num_classes = 0
    cfg.augmentation_strength = "medium"
    with pytest.raises(ValueError, match="labels must lie"):
        input_pipeline.dataset_from_config(cfg, images, labels, train=True, device="cpu")


def test_the_gpu_tests_seeds_cover_what_they_assert():
    """The GPU tests assert coverage and rates from the device's record; the same draw is made here, so a seed that skips a
    stage (or an excluded share above 0.1 %) shows without a GPU."""
    for case, ((h, w), (ho, wo)) in enumerate(ar.CASES):
        images, _ = ar.case_dataset(case)
        recs = np.stack([ar.medium_record(ar.CASE_SEED, 1, i, h, w, ho, wo) for i in range(ar.CASE_IMAGES)])
        missing = [k for k, v in ar.coverage(recs).items() if not v]
        assert not missing, f"case {case}: seed {ar.CASE_SEED} never fires {missing}"
        ill = total = 0
        for i in range(ar.CASE_IMAGES):
            if int(recs[i, ar.R_FLAGS]) & ar.F_HSV:
                out, mask = ar.medium_image(images[i], recs[i], ar.base_of(ar.CASE_SEED, 1, i), ho, wo)
                assert out.shape == (3, ho, wo) and np.isfinite(out).all()
                ill, total = ill + int(mask.sum()), total + mask.size
        assert total > 0 and ill <= 0.001 * total, f"case {case}: {ill} of {total} pixels have an ill-conditioned hue"
    recs = np.stack([ar.draw_medium(ar.STATS_SEED, 1, i, 8, 8) for i in range(ar.STATS_IMAGES)])
    ar.check_statistics(recs, 8, 8)
    # an image on which nothing fires is the plain resize
    none = next(i for i in range(ar.CASE_IMAGES) if ar.draw_medium(ar.CASE_SEED, 1, i, 5, 7)[ar.R_FLAGS] == 0)
    images, _ = ar.case_dataset(0)
    rec = ar.medium_record(ar.CASE_SEED, 1, none, 5, 7, 5, 7)
    assert np.array_equal(ar.medium_image(images[none], rec, 0, 5, 7)[0], ar.resize_image(images[none], 5, 7))
