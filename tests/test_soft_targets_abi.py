"""Soft targets at the C ABI and on the host, with no launch: the new symbols are exported and bound, their refusals return
the argument code before anything reaches the device (the pointers are host memory a rejected call never dereferences), and
``mix_draw`` -- the host function behind the batch-level mixing -- is deterministic, stays inside the image and has the
distribution it documents.  CPU only."""
import ctypes
import math
import re

import numpy as np
import pytest

from conftest import ROOT
from nnue_hip import input_pipeline, lib
from nnue_hip.input_pipeline import GpuImageDataset, mix_draw
from nnue_hip.trainer import NnueTrainer

HEADER = (ROOT / "include" / "nnue_hip.h").read_text()
E_ARG, E_SHAPE = -1, -2
NEW = ("nnue_cross_entropy_soft", "nnue_classifier_train_step_soft", "nnue_classifier_train_step_soft_bucketed", "nnue_mix_batch")
# chosen on the CPU so that the three statistical checks below hold with room (the first of 1..5 that does)
STATS_SEED = 1


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_uint8 * (1 << 16))()
    yield (ctypes.addressof(buf) + 15) & ~15
    del buf


def _err():
    return lib.load().nnue_hip_last_error()


def test_symbols_are_exported_bound_and_documented():
    raw = ctypes.CDLL(str(lib.LIB_PATH))
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in lib.SIGNATURES and lib.SIGNATURES[name][0] is ctypes.c_int, name
        doc = re.search(r"/\*((?:(?!/\*).)*?)\*/\s*int\s+" + name + r"\(", HEADER, flags=re.S)
        assert doc and re.search(r"(train|nnue|datasets|loaders)\.py:\d+", doc.group(1)), name
    plain, soft = lib.SIGNATURES["nnue_classifier_train_step"][1], lib.SIGNATURES["nnue_classifier_train_step_soft"][1]
    assert soft[:len(plain) - 1] == plain[:-1] and len(soft) == len(plain) + 3  # the plain arguments, then labels_b, lam, eps
    plain, soft = lib.SIGNATURES["nnue_classifier_train_step_bucketed"][1], lib.SIGNATURES["nnue_classifier_train_step_soft_bucketed"][1]
    assert soft[:len(plain) - 2] == plain[:-2] and soft[-2:] == plain[-2:] and len(soft) == len(plain) + 3
    assert "t_c" in HEADER and "sum_c (mx - z_c)" in HEADER  # the definition is in the header, once
    for fn in (lib.cross_entropy_soft, lib.mix_batch):
        assert callable(fn)
    assert lib.MIX_MODES == {"none": 0, "mixup": 1, "cutmix": 2}


def _step(p, eps=0.1, labels_b="p", lam="p", phases=3, bucketed=False, B=64, L1=128):
    L = lib.load()
    args = (p, 1, p, p, p, p, p, p, 0.0, p, 1.0, B, L1, 64, 16, 10, p, p, p, p, p, p, p, p, p, p, p, p, p, 1 << 30, phases,
            p if labels_b == "p" else labels_b, p if lam == "p" else lam, eps)
    if bucketed:
        return L.nnue_classifier_train_step_soft_bucketed(*args, None, None)
    return L.nnue_classifier_train_step_soft(*args, None)


@pytest.mark.parametrize("bucketed", (False, True))
def test_train_step_soft_refusals(p, bucketed):
    for eps in (-0.01, 1.0, 1.5, float("nan")):
        assert _step(p, eps=eps, bucketed=bucketed) == E_ARG, eps
        assert b"eps" in _err()
    assert _step(p, lam=None, bucketed=bucketed) == E_ARG
    assert b"labels_b without lam" in _err()
    # ... and the plain call's refusals, with the same codes
    assert _step(p, phases=0, bucketed=bucketed) == E_ARG and b"phases" in _err()
    assert _step(p, phases=123, L1=96, bucketed=bucketed) == E_SHAPE
    assert _step(p, B=0, bucketed=bucketed) == E_ARG


def test_cross_entropy_soft_refusals(p):
    L = lib.load()
    for eps in (-0.5, 1.0, float("nan")):
        assert L.nnue_cross_entropy_soft(p, p, p, p, eps, 4, 10, 1.0, p, p, p, None) == E_ARG and b"eps" in _err()
    assert L.nnue_cross_entropy_soft(p, p, p, None, 0.1, 4, 10, 1.0, p, p, p, None) == E_ARG and b"labels_b without lam" in _err()
    assert L.nnue_cross_entropy_soft(None, p, p, p, 0.1, 4, 10, 1.0, p, p, p, None) == E_ARG and b"null pointer" in _err()
    assert L.nnue_cross_entropy_soft(p, p, p, p, 0.1, 0, 10, 1.0, p, p, p, None) == E_ARG
    assert L.nnue_cross_entropy_soft(p, p, p, p, 0.1, 4, 0, 1.0, p, p, p, None) == E_ARG


def test_mix_batch_refusals(p):
    L = lib.load()
    ok = dict(images=p, labels=p, B=4, H=5, W=7, mode=1, lam=0.5, y0=0, x0=0, hh=0, hw=0, labels_b_out=p, lam_out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nnue_mix_batch(a["images"], a["labels"], a["B"], a["H"], a["W"], a["mode"], a["lam"], a["y0"], a["x0"], a["hh"], a["hw"],
                                a["labels_b_out"], a["lam_out"], None)

    for name in ("images", "labels", "labels_b_out", "lam_out"):
        assert call(**{name: None}) == E_ARG and b"null pointer" in _err(), name
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(mode=3), dict(mode=-1), dict(lam=1.01), dict(lam=-0.01), dict(lam=float("nan")),
               dict(mode=2, hh=6), dict(mode=2, y0=4, hh=2), dict(mode=2, x0=5, hw=3), dict(mode=2, y0=-1, hh=1), dict(mode=2, hw=-1)):
        assert call(**kw) == E_ARG, kw


def test_mix_draw_is_a_function_of_seed_and_step():
    a = [mix_draw(7, s, 0.4, 1.0, 32, 48) for s in range(50)]
    assert a == [mix_draw(7, s, 0.4, 1.0, 32, 48) for s in range(50)]
    assert a != [mix_draw(8, s, 0.4, 1.0, 32, 48) for s in range(50)]
    assert len(set(a)) == 50
    assert mix_draw(7, 3, 0.0, 0.0, 32, 48) == (0, 1.0, 0, 0, 0, 0)
    assert {mix_draw(7, s, 0.4, 0.0, 32, 48)[0] for s in range(20)} == {1}
    assert {mix_draw(7, s, 0.0, 0.4, 32, 48)[0] for s in range(20)} == {2}


@pytest.mark.parametrize("H,W", ((5, 7), (32, 32), (1, 1), (224, 160)))
def test_mix_draw_boxes_lie_inside_the_image(H, W):
    for step in range(500):
        mode, lam, y0, x0, hh, hw = mix_draw(STATS_SEED, step, 0.0, 1.0, H, W)
        assert mode == 2 and 0.0 <= lam <= 1.0
        assert 0 <= y0 and 0 <= x0 and hh >= 0 and hw >= 0 and y0 + hh <= H and x0 + hw <= W
        assert hh <= int(H * math.sqrt(1 - lam)) and hw <= int(W * math.sqrt(1 - lam))  # the usual rule, then clipped


def test_mix_draw_statistics():
    n = 4000
    lam = np.array([mix_draw(STATS_SEED, s, 1.0, 0.0, 32, 32)[1] for s in range(n)])
    assert lam.min() >= 0.0 and lam.max() <= 1.0
    assert abs(lam.mean() - 0.5) <= 4 * math.sqrt(1.0 / 12.0 / n)  # Beta(1, 1) is uniform: variance 1/12
    draws = [mix_draw(STATS_SEED, s, 1.0, 1.0, 32, 32) for s in range(n)]
    modes = np.array([d[0] for d in draws])
    assert set(modes.tolist()) == {1, 2}
    assert abs((modes == 1).mean() - 0.5) <= 4 * math.sqrt(0.25 / n)
    both = np.array([d[1] for d in draws])
    assert both.min() >= 0.0 and both.max() <= 1.0 and abs(both.mean() - 0.5) <= 4 * math.sqrt(1.0 / 12.0 / n)


def test_dataset_refuses_negative_alphas():
    images, labels = np.zeros((4, 4, 4, 3), dtype=np.uint8), np.zeros(4, dtype=np.int64)
    for kw in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mixup_alpha=float("nan"))):
        with pytest.raises(ValueError, match="must not be negative"):
            GpuImageDataset(images, labels, device="cpu", **kw)
    ds = GpuImageDataset(images, labels, device="cpu", mixup_alpha=0.2)
    assert ds.mixes and not GpuImageDataset(images, labels, device="cpu").mixes


class _Config:
    num_classes, use_augmentation, mixup_alpha, cutmix_alpha = 10, False, 0.2, 1.0


def test_only_the_training_dataset_mixes():
    images, labels = np.zeros((4, 4, 4, 3), dtype=np.uint8), np.zeros(4, dtype=np.int64)
    train = input_pipeline.dataset_from_config(_Config, images, labels, train=True, device="cpu")
    val = input_pipeline.dataset_from_config(_Config, images, labels, train=False, device="cpu")
    assert (train.mixup_alpha, train.cutmix_alpha) == (0.2, 1.0) and not val.mixes


@pytest.mark.parametrize("value", (-0.1, 1.0, 2.0, float("nan")))
def test_trainer_refuses_label_smoothing_outside_the_unit_interval(value):
    """Refused before the model, the library or the device is touched."""
    with pytest.raises(ValueError, match="label_smoothing"):
        NnueTrainer(None, 8, (8, 8), lr=0.1, label_smoothing=value)
