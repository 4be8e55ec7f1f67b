"""The autograd bridges of nnue_hip/ops.py with part of the graph frozen: NnueFn, FeatureTransformerFn and ClassifierFn
pick their backward launches from ctx.needs_input_grad (NULL-output forms of the weight gradients, no value
gradient, no STE launch, no d_x).  ``-m gpu``.

A small model on each FeatureTransformer path (mfma: the CIFAR map at batch 40; bits and list: the 5 x 5 grids of
tests/trainer_modes.py), one and three layer stacks, under every mask of tests/partial_grads_cases.py: the gradients of the
trainable parameters are BITWISE those of the unfrozen run -- itself held to the float64 oracle here -- and frozen parameters
keep ``.grad is None``.  tests/test_partial_grads_host.py pins the same masks on the host path against the oracle."""
import pytest
import torch

import nnue_oracle as orc
import partial_grads_cases as pg
import trainer_modes as tm
from conftest import assert_close_grad, assert_close_logits

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CASES = {}


@pytest.fixture(autouse=True)
def policy_knobs_unset(monkeypatch):
    for k in tm.KNOBS:
        monkeypatch.delenv(k, raising=False)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def case(path, K):
    """The model on the device, a batch that keeps its margins to the gates, the unfrozen run (images trainable too) and the
    float64 oracle's gradients; built once."""
    key = (path, K)
    if key not in _CASES:
        from nnue_hip import lib
        cfg = pg.config(path, K)
        g = tm.geometry(cfg)
        assert lib.ft_path(g["F"], g["P"], cfg["l1"], cfg["batch"]) == path
        model = tm.build_model(cfg)
        p64 = {k: v.detach().double() for k, v in model.state_dict().items()}
        images, labels = tm.draw_batch(cfg, p64, g["stride"], torch.Generator().manual_seed(500 + K), cfg["batch"])
        q = {k: v.clone().requires_grad_(k != "nnue2score") for k, v in p64.items()}
        x = images.double().requires_grad_(True)
        ref_logits = orc.model_forward_loop(q, x, g["stride"], None, cfg["clip"])
        torch.nn.functional.cross_entropy(ref_logits, labels).backward()
        model = model.to(DEV)
        images, labels = images.to(DEV), labels.to(DEV)
        logits, grads, d_images = pg.run(model, images, labels, "images_and_all")
        assert_close_logits(logits, ref_logits.detach(), f"{path} K={K} logits")
        for name in pg.TRAINABLE:
            assert_close_grad(grads[name], q[name].grad, f"{path} K={K} {name}")
        assert_close_grad(d_images, x.grad, f"{path} K={K} d_images")
        _CASES[key] = (model, images, labels, logits, grads, d_images)
    return _CASES[key]


@pytest.mark.parametrize("mask", list(pg.MASKS))
@pytest.mark.parametrize("K", pg.STACKS)
@pytest.mark.parametrize("path", list(pg.CONFIGS))
def test_trainable_gradients_under_a_mask_are_bitwise_the_unfrozen_runs(path, K, mask):
    model, images, labels, full_logits, full, full_d_images = case(path, K)
    logits, grads, d_images = pg.run(model, images, labels, mask)
    assert same(logits, full_logits)
    pg.check_mask(mask, grads, d_images, full, full_d_images, same)


@pytest.mark.parametrize("path", list(pg.CONFIGS))
def test_two_forwards_then_two_backwards_and_a_retained_graph(path):
    model, images, labels, _, full, _ = case(path, 1)
    pg.apply_mask(model, "none")
    half = images.shape[0] // 2
    batches = [(images[:half], labels[:half]), (images[half:], labels[half:])]
    alone = []
    for x, y in batches:
        _, grads, _ = pg.run(model, x, y, "none")
        alone.append(grads)
    pg.apply_mask(model, "none")
    losses = [torch.nn.functional.cross_entropy(model(x), y) for x, y in batches]  # both forwards first
    for loss, want in zip(reversed(losses), reversed(alone)):  # backwards in the other order
        for p in model.parameters():
            p.grad = None
        loss.backward()
        for name, p in model.named_parameters():
            if name != "nnue2score":
                assert same(p.grad, want[name]), f"{name}: a second graph alive during backward changed the gradient"
    # retain_graph: the second backward through the same node accumulates the same bits once more
    for p in model.parameters():
        p.grad = None
    loss = torch.nn.functional.cross_entropy(model(images), labels)
    loss.backward(retain_graph=True)
    loss.backward()
    for name, p in model.named_parameters():
        if name != "nnue2score":
            assert same(p.grad, full[name] + full[name]), f"{name}: two backwards do not accumulate exactly twice the gradient"


# ------------------------------------------------------------------ the stand-alone modules
@pytest.mark.parametrize("l1", (300, 768))
def test_stand_alone_feature_transformer_with_and_without_a_value_gradient(l1):
    """nnue.FeatureTransformer always takes the list family: L1 = 300 runs the one-column-per-thread kernels, 768 the
    three-wave wide ones with the simple value gradient."""
    import nnue
    f, b, m = 50, 37, 40
    gen = torch.Generator().manual_seed(l1)
    torch.manual_seed(l1)
    ft = nnue.FeatureTransformer(f, l1).to(DEV)
    with torch.no_grad():
        ft.bias.copy_(torch.randn(l1, generator=gen) * 0.1)
    idx = torch.stack([torch.randperm(f + 1, generator=gen)[:m] for _ in range(b)])  # at most two entries per row and sample
    idx = torch.where(torch.rand(b, m, generator=gen) < 0.25, torch.full_like(idx, -1), idx)
    val, up = torch.randn(b, m, generator=gen), torch.randn(b, l1, generator=gen)
    r_w, r_b, r_val = orc.ft_backward(ft.weight.detach().cpu().double(), idx, val.double(), up.double())

    def run(val_grad, weight=True, bias=True):
        ft.weight.requires_grad_(weight)
        ft.bias.requires_grad_(bias)
        ft.weight.grad = ft.bias.grad = None
        v = val.to(DEV).requires_grad_(val_grad)
        out = ft(idx.to(DEV), v)
        out.backward(up.to(DEV))
        return out.detach(), ft.weight.grad, ft.bias.grad, v.grad

    out, d_w, d_b, d_val = run(True)
    assert_close_logits(out, orc.ft_forward(ft.weight.detach().cpu().double(), ft.bias.detach().cpu().double(), idx, val.double()), "out")
    assert_close_grad(d_w, r_w, "d_weight")
    assert_close_grad(d_b, r_b, "d_bias")
    assert_close_grad(d_val, r_val, "d_val")
    out2, d_w2, d_b2, none = run(False)
    assert none is None and same(out2, out) and same(d_w2, d_w) and same(d_b2, d_b)
    _, d_w3, none_b, d_val3 = run(True, bias=False)
    assert none_b is None and same(d_w3, d_w) and same(d_val3, d_val)
    _, none_w, d_b4, none = run(False, weight=False)
    assert none_w is None and none is None and same(d_b4, d_b)
    _, none_w, none_b, d_val5 = run(True, weight=False, bias=False)
    assert none_w is None and none_b is None and same(d_val5, d_val)


@pytest.mark.parametrize("shape", ((33, 256, 48, 16, 7), (5, 24, 7, 5, 3)))
def test_stand_alone_classifier_with_a_detached_input(shape):
    import nnue
    b, l1, l2, l3, c = shape
    torch.manual_seed(sum(shape))
    cls = nnue.SimpleClassifier(l1, l2, l3, c).to(DEV)
    gen = torch.Generator().manual_seed(b)
    x, up = torch.randn(b, l1, generator=gen).to(DEV), torch.randn(b, c, generator=gen).to(DEV)

    def run(x_grad):
        for p in cls.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(x_grad)
        out = cls(xi)
        out.backward(up)
        return out.detach(), [p.grad for p in cls.parameters()], xi.grad

    out, grads, d_x = run(True)
    out2, grads2, none = run(False)
    assert none is None and d_x is not None and same(out, out2)
    for a, r in zip(grads2, grads):
        assert same(a, r)
    # the unfrozen run against float64
    p64 = [p.detach().cpu().double() for p in cls.parameters()]
    d_x_ref, want = orc.classifier_backward(x.cpu().double(), *p64, up.cpu().double())
    assert_close_logits(out, orc.classifier_forward(x.cpu().double(), *p64), "logits")
    assert_close_grad(d_x, d_x_ref, "d_x")
    for a, r in zip(grads, want):
        assert_close_grad(a, r, "classifier gradient")
