"""The per-iteration learning-rate schedule of the reference's training configs, on the host.

``config/train_nnue.py:39-46`` asks for a schedule (``use_cosine_scheduler``, ``decay_lr``, ``use_cyclical_lr`` ...) whose
formula is ``training_utils.py:283-336`` (``get_lr``: linear warm-up, cosine decay to ``min_lr``, optional cyclical
modulation, one value per iteration).  ``LrSchedule.lr`` restates that formula in float64 with the reference's operation
order, so the doubles are bit-equal; ``values(n)`` tabulates it, rounded once to float32, for
``NnueTrainer.set_lr_schedule`` -- the device only indexes the table (nnue_lr_schedule_step), so any schedule that can be
tabulated works and a scheduled step group is bitwise the single steps under the same values.

The reference never calls ``get_lr``; neither does this build unless a config opts in with the NEW attribute
``lr_schedule = True`` (``from_config``).  Host only: no GPU, no library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class LrSchedule:
    learning_rate: float
    min_lr: float = 0.0
    warmup_iters: int = 0
    lr_decay_iters: int = 0
    decay_lr: bool = True
    use_cyclical_lr: bool = False
    cyclical_lr_period: int = 1000
    cyclical_lr_amplitude: float = 0.1

    def __post_init__(self):
        # the reference divides by zero at it == warmup_iters == lr_decay_iters (training_utils.py:312-314)
        if self.decay_lr and self.lr_decay_iters <= self.warmup_iters:
            raise ValueError(f"lr_decay_iters ({self.lr_decay_iters}) must exceed warmup_iters ({self.warmup_iters}) when decay_lr is set")
        if self.use_cyclical_lr and self.cyclical_lr_period <= 0:
            raise ValueError(f"cyclical_lr_period must be positive, got {self.cyclical_lr_period}")

    def lr(self, it: int) -> float:
        """training_utils.py:283-336, operation for operation (its quirks included: with ``decay_lr=False`` any
        ``it > lr_decay_iters`` still returns ``min_lr``)."""
        if it < self.warmup_iters:
            if self.warmup_iters > 0:
                base_lr = self.learning_rate * (it + 1) / self.warmup_iters
            else:
                base_lr = self.learning_rate
        elif it > self.lr_decay_iters:
            base_lr = self.min_lr
        else:
            if not self.decay_lr:
                base_lr = self.learning_rate
            else:
                decay_ratio = (it - self.warmup_iters) / (self.lr_decay_iters - self.warmup_iters)
                coeff = 0.5 * (1.0 + math.cos(math.pi * decay_ratio))
                base_lr = self.min_lr + coeff * (self.learning_rate - self.min_lr)
        final_lr = base_lr
        if self.use_cyclical_lr and it >= self.warmup_iters:
            period = self.cyclical_lr_period
            amplitude = self.cyclical_lr_amplitude
            progress_in_decay = it - self.warmup_iters
            cycle_progress = (progress_in_decay % period) / period
            cyclical_factor = 1.0 + amplitude * math.sin(2 * math.pi * cycle_progress)
            final_lr *= cyclical_factor
        if it < self.warmup_iters:
            return final_lr
        return max(self.min_lr, final_lr)

    def values(self, n: int) -> torch.Tensor:
        """The first n iterations' rates, float64 rounded once to float32 (what the device table holds)."""
        if n < 1:
            raise ValueError(f"values: n = {n} must be at least 1")
        return torch.tensor([self.lr(it) for it in range(int(n))], dtype=torch.float64).to(torch.float32)

    @staticmethod
    def from_config(config, steps_per_epoch: int) -> Optional["LrSchedule"]:
        """None unless the config sets the new attribute ``lr_schedule`` to something truthy (no reference config does, so
        their runs keep the constant rate of train.py:457-471).  Otherwise the schedule of the config's ``learning_rate``,
        ``warmup_iters`` (0), ``lr_decay_iters`` (``max_epochs * steps_per_epoch``), ``min_lr`` (0.0), ``decay_lr`` (the value of
        ``use_cosine_scheduler``, else False) and the three cyclical keys."""
        if not getattr(config, "lr_schedule", False):
            return None
        return LrSchedule(
            learning_rate=float(config.learning_rate),
            min_lr=float(getattr(config, "min_lr", 0.0)),
            warmup_iters=int(getattr(config, "warmup_iters", 0)),
            lr_decay_iters=int(getattr(config, "lr_decay_iters", int(config.max_epochs) * int(steps_per_epoch))),
            decay_lr=bool(getattr(config, "decay_lr", getattr(config, "use_cosine_scheduler", False))),
            use_cyclical_lr=bool(getattr(config, "use_cyclical_lr", False)),
            cyclical_lr_period=int(getattr(config, "cyclical_lr_period", 1000)),
            cyclical_lr_amplitude=float(getattr(config, "cyclical_lr_amplitude", 0.1)))
