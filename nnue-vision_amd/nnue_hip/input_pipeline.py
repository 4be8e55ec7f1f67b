"""GPU-resident input pipeline.

The reference feeds training through torchvision + albumentations + DataLoader workers
(data/datasets.py:173-372, data/loaders.py:95-120): per image, on the CPU.  At the step rates this build
reaches (a CIFAR-10 epoch is ~17 ms of GPU time) that path cannot keep up by orders of magnitude, so the
dataset (50 000 x 32 x 32 x 3 uint8 = 154 MB for CIFAR) lives in HBM and one kernel per batch gathers,
augments, resizes, normalises and transposes it straight into the trainer's input slot.

``augment`` selects the reference's ``augmentation_strength`` (data/datasets.py:173-195 "light", :301-350 "medium"):
``False``, ``True`` / ``"light"`` or ``"medium"``; ``out_hw`` is the ``A.Resize(target_size)`` that closes every reference
transform list (data/datasets.py:357-361).  The medium policy is HorizontalFlip, RandomRotate90, Rotate, Affine,
RandomBrightnessContrast, HueSaturationValue, OneOf(Blur, GaussianBlur, MotionBlur), GaussNoise and CoarseDropout with
the reference's probabilities and ranges; the geometric stages and the resize are one bilinear sample per image and
values stay float between stages (include/nnue_hip.h defines every stage).  Omitted from the medium list (each
p <= .2): RandomShadow, RandomFog, GridDistortion, ElasticTransform, CLAHE, ColorJitter, Posterize, Equalize.
``"heavy"`` (medium plus a second pass of stronger stages) is not built and raises ``ValueError``.

``mixup_alpha`` / ``cutmix_alpha`` (build extensions, both 0 by default) add one batch-level stage behind the per-image list
and the collate (data/loaders.py:95-120): ``mixed_batch`` is ``batch`` followed by one ``lib.mix_batch`` launch that mixes
sample i with sample B-1-i in place -- mixup with a weight drawn from Beta(alpha, alpha), or CutMix with the usual box --
and returns the second labels and the weights a trainer built with ``two_labels`` takes.  The draw is a host function of
(seed, step), ``mix_draw``: no device read, no synchronisation, and a resumed run mixes as the uninterrupted one does.

Datasets themselves (download / decode) are out of scope: construct ``GpuImageDataset`` from any uint8
``[N,H,W,3]`` array and integer labels.
"""
from __future__ import annotations

import math
import numbers
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from . import lib


def resolve_augment(augment) -> int:
    """``augment=`` of GpuImageDataset -> the policy number of nnue_load_batch_policy (0 none, 1 light, 2 medium)."""
    if augment is None or augment is False:
        return 0
    if augment is True:
        return 1
    if isinstance(augment, str):
        if augment in ("light", "medium"):
            return lib.LOAD_POLICIES[augment]
        if augment == "heavy":
            raise ValueError('augment="heavy" (medium plus a second pass of stronger stages, data/datasets.py:218-300) is not '
                             'built: use "medium"')
    raise ValueError(f'augment: expected False, True, "light" or "medium", got {augment!r}')


def resolve_out_hw(out_hw) -> Optional[Tuple[int, int]]:
    """``out_hw=`` of GpuImageDataset: None (the stored size), one side (square) or (height, width)."""
    if out_hw is None:
        return None
    hw = (out_hw, out_hw) if isinstance(out_hw, numbers.Real) else tuple(out_hw)
    if len(hw) != 2 or any(int(v) != v or int(v) <= 0 for v in hw):
        raise ValueError(f"out_hw: expected a positive (height, width), got {out_hw!r}")
    return int(hw[0]), int(hw[1])


def mix_draw(seed: int, step: int, mixup_alpha: float, cutmix_alpha: float, H: int, W: int):
    """The batch-level draw of step ``step``: (mode, lam, y0, x0, hh, hw), the host arguments of ``lib.mix_batch``.  mode 0 (both
    alphas 0): nothing is mixed.  With both alphas positive each of mixup (1) and CutMix (2) has probability 0.5.
    lam ~ Beta(alpha, alpha) of the chosen mode.  CutMix's box is the usual one -- r = sqrt(1 - lam), sides int(H r) and
    int(W r), centre uniform over the pixels -- clipped to the image (``mix_batch`` then derives the weight from the clipped
    area).  A function of (seed, step) alone: numpy's PCG64 seeded with the pair."""
    if mixup_alpha <= 0 and cutmix_alpha <= 0:
        return 0, 1.0, 0, 0, 0, 0
    rng = np.random.Generator(np.random.PCG64([int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)]))
    coin = rng.random()  # drawn in every case: the stream does not depend on which alphas are set
    mode = 1 if cutmix_alpha <= 0 else 2 if mixup_alpha <= 0 else (1 if coin < 0.5 else 2)
    alpha = mixup_alpha if mode == 1 else cutmix_alpha
    lam = min(1.0, max(0.0, float(rng.beta(alpha, alpha))))
    cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
    if mode == 1:
        return 1, lam, 0, 0, 0, 0
    r = math.sqrt(1.0 - lam)
    cut_h, cut_w = int(H * r), int(W * r)
    y0, y1 = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
    x0, x1 = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
    return 2, lam, y0, x0, y1 - y0, x1 - x0


class GpuImageDataset:
    def __init__(self, images_u8, labels, device=None, augment=False, seed: int = 0,
                 num_classes: Optional[int] = None, out_hw=None, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0):
        resolve_augment(augment)  # refuse "heavy" and unknown strings here, not at the first batch
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        if not (self.mixup_alpha >= 0.0 and self.cutmix_alpha >= 0.0):
            raise ValueError(f"mixup_alpha = {mixup_alpha} and cutmix_alpha = {cutmix_alpha} must not be negative")
        self.out_hw = resolve_out_hw(out_hw)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        images_u8 = torch.as_tensor(images_u8)
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            raise ValueError(f"images: expected uint8 [N,H,W,3], got {images_u8.dtype} {tuple(images_u8.shape)}")
        labels = torch.as_tensor(labels).to(torch.int64).reshape(-1)
        if labels.numel() != images_u8.shape[0]:
            raise ValueError("labels: one label per image expected")
        # validated once, on the host, outside every timed region: inside the step -1 is the padding sentinel of a
        # short last batch and the loss kernel ignores any out-of-range label, so a corrupt label must not get that far
        self.label_range = (int(labels.min()), int(labels.max())) if labels.numel() else (0, 0)
        if self.label_range[0] < 0 or (num_classes is not None and self.label_range[1] >= num_classes):
            raise ValueError(f"labels must lie in [0, {num_classes if num_classes is not None else 'C'}): "
                             f"found {self.label_range[0]} .. {self.label_range[1]}")
        self.images = images_u8.contiguous().to(device)
        self.labels = labels.to(device)
        self.augment, self.seed = augment, seed
        self.step = 0  # advances with every batch: a fresh draw for every visit of a sample

    def __len__(self) -> int:
        return self.images.shape[0]

    @property
    def image_hw(self) -> Tuple[int, int]:
        return int(self.images.shape[1]), int(self.images.shape[2])

    @property
    def output_hw(self) -> Tuple[int, int]:
        """The size of the batches (the trainer's ``hw``): ``out_hw`` if given, else the stored size."""
        return self.image_hw if self.out_hw is None else self.out_hw

    def batch(self, indices: torch.Tensor, out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
              params_out: Optional[torch.Tensor] = None):
        """One normalised (and, if enabled, augmented and resized) batch for the given dataset indices (device int64).
        ``params_out`` (float32 [b, lib.load_batch_params_count()]) receives what was drawn for each image."""
        self.step += 1
        policy = resolve_augment(self.augment)
        if policy <= 1 and self.output_hw == self.image_hw and params_out is None:
            return lib.load_batch(self.images, self.labels, indices.to(self.images.device), bool(policy), self.seed, self.step,
                                  out=out, labels_out=labels_out)
        return lib.load_batch_policy(self.images, self.labels, indices.to(self.images.device), policy, self.seed, self.step,
                                     out_hw=self.output_hw, out=out, labels_out=labels_out, params_out=params_out)

    @property
    def mixes(self) -> bool:
        return self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0

    def mixed_batch(self, indices: torch.Tensor, out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
                    soft_out=None):
        """``batch`` followed by one ``lib.mix_batch`` launch on the same stream, with ``mix_draw``'s values for this batch's
        step.  ``soft_out`` = (labels_b int64 [b], lam float32 [b]) receives the second labels and the weights (a trainer's
        ``soft_inputs[s]``).  Returns (images, labels, labels_b, lam)."""
        images, labels = self.batch(indices, out=out, labels_out=labels_out)
        mode, lam, y0, x0, hh, hw = mix_draw(self.seed, self.step, self.mixup_alpha, self.cutmix_alpha, *self.output_hw)
        labels_b, lam_out = soft_out if soft_out is not None else (None, None)
        labels_b, lam_out = lib.mix_batch(images, labels, mode, lam, (y0, x0, hh, hw), labels_b_out=labels_b, lam_out=lam_out)
        return images, labels, labels_b, lam_out

    def loader(self, batch_size: int, shuffle: bool = False, drop_last: bool = False,
               generator: Optional[torch.Generator] = None) -> "GpuLoader":
        return GpuLoader(self, batch_size, shuffle, drop_last, generator)


class GpuLoader:
    """Iterable of (images float32 [b,3,H,W], labels int64 [b]) device batches; re-iterable (one pass = one epoch);
    ``len()`` = number of batches, like a DataLoader.  Everything stays on the device; nothing synchronises."""

    def __init__(self, dataset: GpuImageDataset, batch_size: int, shuffle: bool, drop_last: bool, generator):
        self.dataset, self.batch_size, self.shuffle, self.drop_last, self.generator = dataset, batch_size, shuffle, drop_last, generator

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        for idx in self.index_batches():
            yield self.dataset.batch(idx)

    def index_batches(self):
        """The epoch's index tensors (device), one per batch -- for callers that place batches themselves."""
        n, dev = len(self.dataset), self.dataset.images.device
        if self.shuffle:
            order = torch.randperm(n, generator=self.generator).to(dev) if self.generator is not None \
                else torch.randperm(n, device=dev)
        else:
            order = torch.arange(n, device=dev)
        return [order[i * self.batch_size:(i + 1) * self.batch_size] for i in range(len(self))]


def train_epoch(trainer, loader: GpuLoader, teacher=None):
    """One epoch of ``trainer.step`` fed in place: each batch is written by the pipeline kernel straight into a trainer
    input slot (no staging copy), on the trainer's stream, then the step's graph is replayed on that slot.  With more than
    one input slot, whole rounds of full batches go through ``trainer.step_many``: one pipeline kernel per slot, then ONE
    graph replay for the round's steps (no gap between graph launches).  Returns (sum of per-step mean losses as a
    device scalar, number of steps); the short last batch of an epoch goes through ``trainer.step(images, labels)``
    (padded, see NnueTrainer.step).  A dataset that mixes (mixup_alpha / cutmix_alpha) is fed through ``mixed_batch``: one more
    launch per batch, the second labels and the weights into ``trainer.soft_inputs[s]``; the trainer must have been built with
    ``two_labels=True``.

    ``teacher`` (a trainer built with distill_alpha > 0 needs one; never called otherwise): any callable images [b,3,H,W] -> logits
    [b,C] on the device, such as a drop-in ``nnue.NNUE`` in eval mode or any ``nn.Module``.  It runs under ``torch.no_grad()``
    on the same stream between the batch fill (after mixing, if the dataset mixes) and the step, and its logits go into
    ``trainer.teacher_inputs[s]``.

    A side-stream double buffer was measured and is slower here (0.218 vs 0.177 ms per C2 step): the 9 us kernel is
    not worth two event waits per step on a host-launch-bound loop."""
    ds, slots = loader.dataset, len(trainer.inputs)
    if ds.label_range[1] >= trainer.C:
        raise ValueError(f"dataset labels reach {ds.label_range[1]} but the model has {trainer.C} classes")
    mixes = ds.mixes
    if mixes and not trainer.two_labels:
        raise ValueError("the dataset mixes batches (mixup_alpha / cutmix_alpha): build the trainer with two_labels=True")
    distils = trainer.teacher_inputs is not None
    if distils and teacher is None:
        raise ValueError("the trainer was built with distill_alpha > 0: train_epoch needs a teacher")

    def teach(images):  # the teacher's logits for one batch, as the trainer holds them
        with torch.no_grad():
            logits = teacher(images)
        if logits.shape != (images.shape[0], trainer.C):
            raise ValueError(f"the teacher returned {tuple(logits.shape)} for {images.shape[0]} images and {trainer.C} classes")
        return logits.detach().to(torch.float32)

    def fill(idx, s):  # one batch straight into input slot s
        if mixes:
            ds.mixed_batch(idx, out=trainer.inputs[s][0], labels_out=trainer.inputs[s][1], soft_out=trainer.soft_inputs[s])
        else:
            ds.batch(idx, out=trainer.inputs[s][0], labels_out=trainer.inputs[s][1])
        if distils:
            trainer.teacher_inputs[s].copy_(teach(trainer.inputs[s][0]))
    total = torch.zeros((), dtype=torch.float32, device=trainer.dev)
    batches = loader.index_batches()
    n, i, round_slots = len(batches), 0, tuple(range(slots))
    while i < n:
        if slots > 1 and i + slots <= n and batches[i + slots - 1].numel() == trainer.B:  # only the last batch can be short
            for s in round_slots:
                fill(batches[i + s], s)
            total += trainer.step_many(round_slots).sum()
            i += slots
            continue
        s, idx = i % slots, batches[i]
        if idx.numel() == trainer.B:
            fill(idx, s)
            total += trainer.step(slot=s)
        else:
            images, labels, labels_b, lam = ds.mixed_batch(idx) if mixes else (*ds.batch(idx), None, None)
            count = None
            if trainer.dp.world > 1:
                # short last batch with ranks: the exact mean needs the number of real samples over ALL ranks (every
                # rank's loader yields the same number of batches; a rank may hold fewer or no samples in the last one)
                import torch.distributed as dist
                cnt = torch.tensor([int(idx.numel())], dtype=torch.int64, device=trainer.dev if trainer.dp.backend == "nccl" else "cpu")
                dist.all_reduce(cnt, group=trainer.dp.group)
                count = int(cnt.item())
            total += trainer.step(images, labels, slot=s, global_count=count, labels_b=labels_b, lam=lam,
                                  teacher_logits=teach(images) if distils else None)
        i += 1
    return total, n


def augment_from_config(config, train: bool):
    """(augment, out_hw) as train.py:278-287 passes them to create_data_loaders: ``use_augmentation``,
    ``augmentation_strength`` (default "medium", data/loaders.py:23) and the model's ``input_size``; validation and test
    loaders get no augmentation (data/loaders.py:95-120)."""
    augment = False
    if train and bool(getattr(config, "use_augmentation", True)):
        augment = getattr(config, "augmentation_strength", "medium")
    size = getattr(config, "input_size", None)
    if isinstance(size, (tuple, list)):
        size = tuple(size[-2:])  # datasets.py keeps the last two entries of a (C, H, W) target
    return augment, resolve_out_hw(size)


def dataset_from_config(config, images_u8, labels, train: bool, device=None, seed: int = 0) -> GpuImageDataset:
    """A GpuImageDataset set up from a training config the way train.py:278-287 sets up the reference's loaders."""
    augment, out_hw = augment_from_config(config, train)
    num_classes = getattr(config, "num_classes", None)
    mix = {k: float(getattr(config, k, 0.0)) if train else 0.0 for k in ("mixup_alpha", "cutmix_alpha")}  # the training set only
    return GpuImageDataset(images_u8, labels, device=device, augment=augment, seed=seed,
                           num_classes=int(num_classes) if num_classes is not None else None, out_hw=out_hw, **mix)
