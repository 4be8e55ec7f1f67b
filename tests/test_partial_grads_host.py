"""The freeze masks of tests/partial_grads_cases.py on the CPU host path (NNUE._host_forward, float32) against the float64
oracle at the suite's gradient bar: what a frozen conv, table or classifier must leave in the other parameters' gradients,
pinned without a GPU.  The batches keep a margin to the binarisation and ReLU gates (trainer_modes.draw_batch), so float32
and float64 take the same branches.  CPU only."""
import pytest
import torch

import nnue_oracle as orc
from conftest import assert_close_logits
import partial_grads_cases as pg
import trainer_modes as tm

BATCH = 9
_REFS = {}


def case(path, K):
    """A model on the CPU, a batch, and the float64 oracle's gradients with everything (the images too) trainable."""
    key = (path, K)
    if key not in _REFS:
        cfg = pg.config(path, K)
        model = tm.build_model(cfg)
        gen = torch.Generator().manual_seed(1000 + K)
        p64 = {k: v.detach().double() for k, v in model.state_dict().items()}
        images, labels = tm.draw_batch(cfg, p64, tm.geometry(cfg)["stride"], gen, BATCH)
        q = {k: v.clone().requires_grad_(k != "nnue2score") for k, v in p64.items()}
        x = images.double().requires_grad_(True)
        logits = orc.model_forward_loop(q, x, tm.geometry(cfg)["stride"], None, cfg["clip"])
        torch.nn.functional.cross_entropy(logits, labels).backward()
        _REFS[key] = (model, images, labels, logits.detach(), {k: q[k].grad for k in pg.TRAINABLE}, x.grad)
    return _REFS[key]


def close(got, ref):
    """conftest.assert_close_grad's bar: 1e-4 of the largest reference magnitude."""
    return float((got.double() - ref).abs().max()) <= 1e-4 * max(float(ref.abs().max()), 1e-12)


@pytest.mark.parametrize("mask", list(pg.MASKS))
@pytest.mark.parametrize("K", pg.STACKS)
@pytest.mark.parametrize("path", list(pg.CONFIGS))
def test_host_path_under_a_freeze_mask_is_the_oracle(path, K, mask):
    model, images, labels, ref_logits, ref, ref_d_images = case(path, K)
    assert not images.is_cuda
    logits, grads, d_images = pg.run(model, images, labels, mask)
    assert_close_logits(logits, ref_logits)
    assert float(ref["input.weight"].abs().max()) > 0 and float(ref["conv.weight"].abs().max()) > 0 and float(ref_d_images.abs().max()) > 0
    pg.check_mask(mask, grads, d_images, ref, ref_d_images, close)


def test_masks_cover_the_branches_of_the_bridges():
    frozen = {m: set(f) for m, (f, _) in pg.MASKS.items()}
    assert frozen["none"] == set() and frozen["front"] == set(pg.FRONT)
    assert frozen["table_weight"] == {"input.weight"} and frozen["table_bias"] == {"input.bias"}
    assert set(pg.TRAINABLE) - frozen["classifier_only"] == set(pg.CLS)
    assert frozen["images_only"] == set(pg.TRAINABLE) and pg.MASKS["images_only"][1]
    for path, want in (("mfma", (968, 800, 256)), ("bits", (75, 75, 256)), ("list", (75, 75, 24))):
        cfg = pg.config(path, 1)
        g = tm.geometry(cfg)
        assert (g["P"], g["F"], cfg["l1"]) == want and cfg["batch"] <= 40
