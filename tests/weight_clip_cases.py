"""What the weight-clip tests share (a helper, not a test module): the rescale that makes the clamp bite, and the driver that
holds a trainer built with ``weight_clip = c`` to its definition -- after every step it is, bit for bit, the trainer built with
``weight_clip = 0`` on which the four clipped tensors were ``clamp_``ed after that step (include/nnue_hip.h, "weight clip").

The clamp bites by construction, not by luck: before training each of the four tensors (and the conv weights, which must NOT be
clamped) is rescaled so that its median |w| equals the bound -- half of it lies outside the range at step 1 -- and ``pair_steps``
asserts on the plain-plus-``clamp_`` side that in every compared step the clamp changed at least ``BITE`` of every tensor.

From step 2 on the clamp bites where an element on the bound moves outward.  Measured on the reference side alone (row A of
tests/trainer_modes.py, shares of input.weight / the three classifier weights changed at steps 2 and 3):
* at the rows' own max_grad_norm = 1 the clipped gradient of a rescaled model is smaller than the weight decay's pull inward:
  0.024 / 0.062 / 0.109 / 0.194 -- so the pairs run at ``GRAD_NORM`` = 100 (0.24 / 0.17 / 0.12 / 0.21; 37 of the 45 rows pass so);
* rows with several layer stacks, with clipped activations (saturated by the rescaled table: its gradient is zero) or with a last
  layer of 15 weights stay below the bar whatever the learning rate (x 1, 10, 100) and the seed (three tried), e.g. A_k4_clip
  0.04 / 0.02 / 0.11 / 0.12 and A_k4_adam 0.23 / 0.08 / 0.09 / 0.09.  There ``respread`` doubles the four tensors on BOTH sides before
  every later step: half of each tensor lies outside the range again, the same perturbation on both sides keeps the pair's
  definition, and the bar is the same.
"""
from typing import Callable, Dict, List, Sequence

import torch

from nnue_hip.trainer import CLIPPED

BITE = 0.10  # the least share of each clipped tensor the reference side's clamp_ must change in every compared step
GRAD_NORM = 100.0  # the pairs' max_grad_norm (see above)


def rescale(params: Dict[str, torch.Tensor], c: float) -> None:
    """w *= c / median|w| on the four clipped tensors and on the conv weights (in place; `params`: name -> tensor)."""
    with torch.no_grad():
        for name in CLIPPED + ("conv.weight",):
            w = params[name]
            w.mul_(c / float(w.abs().median()))


def clamp_and_count(params: Dict[str, torch.Tensor], c: float) -> Dict[str, float]:
    """clamp_(-c, c) on the four tensors; returns the share of each that the clamp changed."""
    share = {}
    with torch.no_grad():
        for name in CLIPPED:
            w = params[name]
            before = w.clone()
            w.clamp_(-c, c)
            share[name] = float((w != before).float().mean())
    return share


def state_of(tr) -> List[torch.Tensor]:
    return [tr.flat_params.clone()] + [t.clone() for t in tr._optimizer_buffers()]


def pair_steps(clipped, plain, c: float, feed: Sequence[Callable], what: str, respread: bool = False) -> None:
    """Runs ``feed[i](trainer)`` -- one optimizer step, returning its loss -- on both trainers for every i and holds the pair to
    the definition after each: parameters (the whole flat buffer: conv weights, thresholds and biases with it), momentum or both
    moments, and the loss, all ``torch.equal``."""
    assert clipped.weight_clip == c and plain.weight_clip == 0.0
    for tr in (clipped, plain):
        rescale(tr.p, c)
        tr.max_grad_norm = GRAD_NORM
    assert torch.equal(clipped.flat_params, plain.flat_params)
    assert float(plain.p["conv.weight"].abs().max()) > c  # (left alone although it exceeds the bound)
    for i, step in enumerate(feed):
        if respread and i > 0:
            with torch.no_grad():
                for tr in (clipped, plain):
                    for name in CLIPPED:
                        tr.p[name].mul_(2.0)
        loss_c = step(clipped).clone()
        loss_p = step(plain).clone()
        torch.cuda.synchronize()
        conv = plain.p["conv.weight"].clone()
        share = clamp_and_count(plain.p, c)
        print(f"{what} step {i}: loss {float(loss_p):.6g}; clamp_ changed " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
        assert min(share.values()) >= BITE, f"{what} step {i}: the reference's clamp_ changed only {share} of the tensors"
        assert torch.equal(conv, plain.p["conv.weight"]) and float(conv.abs().max()) > c
        assert torch.equal(loss_c, loss_p), f"{what} step {i}: loss {float(loss_c)} != {float(loss_p)}"
        got, ref = state_of(clipped), state_of(plain)
        assert len(got) == len(ref)
        for j, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (f"{what} step {i}: buffer {j} (0: parameters, then the optimizer's) differs in "
                                       f"{int((a != b).sum())} of {a.numel()} elements")


def fresh_batches(count: int, batch: int, image: int, classes: int, seed: int = 11):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 3, image, image, generator=gen), torch.randint(0, classes, (batch,), generator=gen))
            for _ in range(count)]
