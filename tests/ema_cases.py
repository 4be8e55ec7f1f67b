"""What the weight-average tests share (a helper, not a test module): the driver that holds a trainer built with ``ema_decay`` to
its definition (include/nnue_hip.h, "weight average") -- after every step it is, bit for bit, the plain trainer on parameters,
optimizer state and losses, and its ``flat_ema`` is ``nnue_ema_update`` (the stand-alone pass) applied to the previous average
and the plain trainer's new parameters.

The average moves by construction: the rows train with weight decay and a learning rate above 0, so every element of a tensor
moves in every step and the average follows it; ``pair_steps`` asserts that the average left its start and is not the
parameters themselves.
"""
from typing import Callable, List, Optional, Sequence

import torch

DECAY = 0.9  # the pairs' decay: an average that visibly lags the parameters after three steps


def state_of(tr) -> List[torch.Tensor]:
    return [tr.flat_params.clone()] + [t.clone() for t in tr._optimizer_buffers()]


def reference_step(ref_ema: torch.Tensor, new_params: torch.Tensor, omd: float, omd_dev: Optional[torch.Tensor] = None) -> None:
    """ref_ema <- the stand-alone pass on it and `new_params` (in place)."""
    from nnue_hip import lib
    lib.ema_update(ref_ema, new_params, omd, omd_dev)


def pair_steps(averaged, plain, feed: Sequence[Callable], what: str, omd_of_step: Optional[Callable] = None) -> torch.Tensor:
    """Runs ``feed[i](trainer)`` -- one optimizer step, returning its loss -- on both trainers for every i and holds the pair to
    the definition after each.  omd_of_step(i): the rate of step i (a warm-up's), else the decay's.  Returns the reference
    average after the last step."""
    from nnue_hip import lib
    assert averaged.ema_decay > 0.0 and plain.ema_decay == 0.0 and plain.flat_ema is None
    assert torch.equal(averaged.flat_params, plain.flat_params)
    ref = averaged.flat_ema.clone()
    start = ref.clone()
    for i, step in enumerate(feed):
        loss_a = step(averaged).clone()
        loss_p = step(plain).clone()
        torch.cuda.synchronize()
        omd = lib.ema_omd(averaged.ema_decay) if omd_of_step is None else omd_of_step(i)
        reference_step(ref, plain.flat_params, omd)
        torch.cuda.synchronize()
        assert torch.equal(loss_a, loss_p), f"{what} step {i}: loss {float(loss_a)} != {float(loss_p)}"
        got, want = state_of(averaged), state_of(plain)
        assert len(got) == len(want)
        for j, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (f"{what} step {i}: buffer {j} (0: parameters, then the optimizer's) differs in "
                                       f"{int((a != b).sum())} of {a.numel()} elements")
        averaged.ema_state()  # (under the sharded update with several ranks: the on-demand gather of the ranks' shards)
        diff = averaged.flat_ema != ref
        assert not bool(diff.any()), (f"{what} step {i}: the average differs from nnue_ema_update in {int(diff.sum())} of {ref.numel()} "
                                      f"elements, first at {int(diff.nonzero()[0])}")
    moved = float((ref != start).float().mean())
    print(f"{what}: after {len(feed)} steps the average left its start in {moved:.3f} of the flat buffer")
    assert moved > 0.5 and not torch.equal(ref, plain.flat_params)
    return ref


def fresh_batches(count: int, batch: int, image: int, classes: int, seed: int = 11):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 3, image, image, generator=gen), torch.randint(0, classes, (batch,), generator=gen))
            for _ in range(count)]
