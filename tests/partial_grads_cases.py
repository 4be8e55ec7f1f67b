"""Freeze masks for the autograd bridges of nnue_hip/ops.py (NnueFn, FeatureTransformerFn, ClassifierFn branch on
ctx.needs_input_grad) and the small models they are tried on, one per FeatureTransformer path.  Shared by the CPU test (the
host path against the float64 oracle) and the GPU test (the HIP path: trainable gradients bitwise those of the unfrozen run)."""
import torch

import trainer_modes as tm

FRONT = ("conv.weight", "visual_threshold")
TABLE = ("input.weight", "input.bias")
CLS = tuple(f"classifier.classifier.{i}.{n}" for i in (0, 2, 4) for n in ("weight", "bias"))
TRAINABLE = FRONT + TABLE + CLS  # nnue2score takes no part in forward: never a gradient

MASKS = {  # name: (frozen parameters, images.requires_grad)
    "none": ((), False),
    "front": (FRONT, False),                       # a frozen conv and threshold: no value gradient, no STE launch
    "table_weight": (("input.weight",), False),    # d_weight NULL, d_bias requested
    "table_bias": (("input.bias",), False),        # the reverse
    "classifier_only": (FRONT + TABLE, False),     # neither table launch
    "images_only": (TRAINABLE, True),              # the value gradient and the conv's input gradient alone
    "images_and_all": ((), True),
}

CONFIGS = {  # ft_path: configuration over trainer_modes.A
    "mfma": dict(tm.A, batch=40),
    "bits": dict(tm.A, **tm.BITS),
    "list": dict(tm.A, **tm.BY_NAME["g5_list"].cfg),
}
STACKS = (1, 3)


def config(path, K):
    return dict(CONFIGS[path], K=K)


def apply_mask(model, mask):
    frozen, _ = MASKS[mask]
    for name, p in model.named_parameters():
        p.requires_grad_(name not in frozen)
        p.grad = None


def run(model, images, labels, mask, backward=True):
    """One forward / backward under a mask; returns (logits, {name: grad or None}, d_images or None)."""
    apply_mask(model, mask)
    x = images.detach().clone().requires_grad_(MASKS[mask][1])
    logits = model(x)
    if backward:
        torch.nn.functional.cross_entropy(logits, labels).backward()
    return logits.detach(), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}, x.grad


def check_mask(mask, grads, d_images, full, full_d_images, same):
    """Trainable parameters hold the unfrozen run's gradients (`same`: the comparison), frozen ones hold none."""
    frozen, want_images = MASKS[mask]
    for name in TRAINABLE:
        if name in frozen:
            assert grads[name] is None, f"{mask}: the frozen {name} received a gradient"
        else:
            assert grads[name] is not None, f"{mask}: {name} has no gradient"
            assert same(grads[name], full[name]), f"{mask}: the gradient of {name} differs from the unfrozen run's"
    assert grads["nnue2score"] is None
    if want_images:
        assert d_images is not None and same(d_images, full_d_images), f"{mask}: d_images differs from the unfrozen run's"
    else:
        assert d_images is None
