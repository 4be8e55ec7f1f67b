"""The training driver around the fused step: what ``train.py:257-454`` does for the
NNUE model, minus the parts that are out of scope here (W&B, RunPod, dataset download and the C++-engine compile).

* ``load_config`` executes a Python file as the config module (config/config_loader.py:16-50) -- the same
  ``config/train_*.py`` files work unchanged; only the attributes ``train_model`` reads are used.
* ``train_model`` builds the model from the config (train.py:289-302), picks SGD(lr, momentum, weight_decay)
  for ``optimizer_type == "sgd"`` and Adam(lr, weight_decay) otherwise (train.py:457-471), clips with
  ``max_grad_norm`` only if the attribute exists and is > 0 (train.py:363-364), trains ``max_epochs`` epochs,
  evaluates the train and validation loaders after each (train.py:378-387) and keeps the checkpoint with the
  best validation F1 in the reference's layout (checkpoint_manager.py:45-51):
  ``{"epoch", "model_state_dict", "optimizer_state_dict", "metrics", "config_name"}``.
  (serialize.py:536 expects "state_dict" or a bare state dict instead -- the reference's own inconsistency is
  kept: pass ``ckpt["model_state_dict"]`` to it.)
* ``compiled_eval`` (argument, or the config attribute of that name; off by default) adds the reference's per-epoch compiled
  evaluation (train.py:389-427): the integer engine is requantised from the live parameters on the device
  (``EngineModel.requantize``) and run over the validation loader (``evaluate.evaluate_engine``); the row gains
  ``compiled/f1``, ``compiled/accuracy``, ``compiled/ms_per_sample`` and ``compiled/latent_density``.  Unlike the reference,
  whose call clamps the live weights through ``serialize_model``, this leaves the parameters alone: a run with the metrics on
  is bitwise the run with them off.  The optional config attribute ``compiled_eval_source`` (default ``"float"``) is
  ``evaluate_engine``'s ``source``: ``"u8"`` evaluates straight from the uint8 store of a ``GpuLoader``'s dataset.
* ``lr_schedule`` (argument: an ``LrSchedule`` or a sequence of per-step rates; default ``LrSchedule.from_config``, which is
  None unless the config sets the new attribute ``lr_schedule``) attaches a per-step schedule to the trainer
  (training_utils.py:283-336, which the reference defines and never calls); each history row then gains ``train/lr``, the
  rate of the epoch's last step.
* ``label_smoothing``, ``mixup_alpha``, ``cutmix_alpha`` (optional config attributes, all 0 by default; build extensions): the
  training trainer is built with the smoothing constant, and -- when the training ``GpuLoader``'s dataset mixes
  (``dataset_from_config`` reads the two alphas) -- with ``two_labels``.  Only the training trainer and the training dataset
  see them: ``evaluate_model`` on the train, validation and test loaders stays plain cross-entropy on unmixed batches, so the
  reported losses stay comparable across runs.
* ``distill_alpha``, ``distill_temperature`` (optional config attributes, 0 and 1 by default; build extensions) and the argument
  ``teacher``: with ``distill_alpha > 0`` the training trainer adds alpha T^2 KL(teacher at T || student at T) to (1 - alpha) times
  its loss (include/nnue_hip.h, "soft targets"), on the logits ``teacher`` -- any callable images [b,3,H,W] -> logits [b,C] on
  the device, such as a drop-in ``nnue.NNUE`` in eval mode -- returns for each training batch under ``torch.no_grad()``.
  ``distill_alpha > 0`` without a teacher is a ValueError; with alpha 0 a teacher is never called.  Evaluation stays plain
  cross-entropy.
* ``ema_decay`` / ``ema_warmup`` (optional config attributes, 0 / False by default; a build extension): the trainer keeps a moving
  average of the weights inside its update launches (``NnueTrainer(ema_decay=, ema_warmup=)``).  With the average on every
  epoch's row gains ``val_ema/loss``, ``val_ema/f1`` and ``val_ema/accuracy`` -- and ``compiled_ema/*`` beside ``compiled/*`` --
  all measured through ``trainer.ema_weights()``, and the checkpoints gain ``ema_state_dict`` (the averaged parameters under the
  model's state-dict keys).  The best model is selected on ``val/f1`` as before.
* ``weight_clip`` (optional config attribute, 0 by default; a build extension): the trainer clamps the table and the classifier's
  weights to [-weight_clip, weight_clip] inside every optimizer update.  1.0 is what the export clamps to (``_clip_weights``,
  nnue.py:528-539): the metrics of a run trained with it describe the network ``serialize_model`` writes.
* ``save_last`` / ``resume_from`` (arguments, or the config attributes of those names; off by default): after each epoch's
  evaluations ``last.ckpt`` is written beside ``best-model.ckpt`` -- the five reference keys plus ``"run_state"`` (the
  trainer's state, the epoch and step counts, best-so-far values, the history, the GPU dataset's draw counter and the
  shuffle generator's state) -- and ``resume_from`` continues such a run at the next epoch with the same bits an
  uninterrupted run has.  Epoch boundaries only; validation and test loaders are expected to be deterministic, as
  data/loaders.py:95-120 builds them; the exact continuation of the input pipeline holds for a ``GpuLoader``.

Loaders are any iterables of ``(images float32 [b,3,H,W], labels int [b])`` batches; the data pipeline itself
(torchvision / albumentations) is out of scope.
"""
from __future__ import annotations

import importlib.util
from dataclasses import dataclass, field
from pathlib import Path
from types import ModuleType
from typing import Callable, Dict, Iterable, List, Optional

import os

import torch

from . import lib
from .trainer import NnueTrainer
from .lr_schedule import LrSchedule
from .input_pipeline import GpuLoader, train_epoch


class ConfigError(Exception):
    """Raised when a configuration file cannot be loaded (config/config_loader.py:10-13)."""


def load_config(config_path) -> ModuleType:
    path = Path(config_path)
    if not path.exists():
        raise ConfigError(f"Configuration file not found: {path}")
    if path.suffix != ".py":
        raise ConfigError(f"Configuration file must be a Python file (.py): {path}")
    try:
        spec = importlib.util.spec_from_file_location("config", path)
        if spec is None or spec.loader is None:
            raise ConfigError(f"Failed to create module spec for: {path}")
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return module
    except ConfigError:
        raise
    except Exception as e:  # same wrapping as the reference
        raise ConfigError(f"Failed to load configuration from {path}: {e}")


@dataclass
class TrainResult:
    best_val_f1: float = 0.0
    best_epoch: int = -1
    history: List[Dict[str, float]] = field(default_factory=list)
    test: Optional[Dict[str, float]] = None
    checkpoint_path: Optional[Path] = None
    steps: int = 0


def build_model(config, device):
    import nnue
    feature_set = nnue.GridFeatureSet(grid_size=config.grid_size, num_features_per_square=config.num_features_per_square)
    # the two build extensions are read from the config when present (reference configs never set them: train.py:289-302)
    return nnue.NNUE(feature_set=feature_set, l1_size=config.l1_size, l2_size=config.l2_size, l3_size=config.l3_size,
                     num_classes=config.num_classes, input_size=config.input_size, weight_decay=config.weight_decay,
                     num_ls_buckets=int(getattr(config, "num_ls_buckets", 1)),
                     clip_activations=getattr(config, "clip_activations", None)).to(device)


def config_weight_clip(config) -> float:
    """The config's ``weight_clip`` (0 where it has none), checked as the trainer checks it: ValueError for a negative, NaN or
    infinite value."""
    return lib.checked_weight_clip(getattr(config, "weight_clip", 0.0))


def config_ema(config):
    """(ema_decay, ema_warmup) of the config (0, False where it has none), checked as the trainer checks them: ValueError for a
    decay outside [0, 1) or NaN, and for a warm-up without a decay."""
    decay, warmup = lib.checked_ema_decay(getattr(config, "ema_decay", 0.0)), bool(getattr(config, "ema_warmup", False))
    if warmup and not decay:
        raise ValueError("the config sets ema_warmup without ema_decay > 0")
    return decay, warmup


def run_training(config, train_loader: Iterable, val_loader: Iterable, test_loader: Optional[Iterable] = None, model=None,
                 checkpoint_dir=None, log: Callable[[str], None] = print, use_graph: bool = True,
                 compiled_eval: Optional[bool] = None, save_last: Optional[bool] = None, resume_from=None,
                 lr_schedule=None, teacher=None) -> TrainResult:
    import evaluate
    distill_alpha, distill_temperature = lib.check_distill(getattr(config, "distill_alpha", 0.0), getattr(config, "distill_temperature", 1.0))
    if distill_alpha > 0.0 and teacher is None:
        raise ValueError(f"the config sets distill_alpha = {distill_alpha}: run_training needs a teacher")
    if distill_alpha == 0.0:
        teacher = None  # never called
    if save_last is None:
        save_last = bool(getattr(config, "save_last", False))
    if resume_from is None:
        resume_from = getattr(config, "resume_from", None)
    optimizer_type = "sgd" if config.optimizer_type == "sgd" else "adam"
    weight_clip = config_weight_clip(config)
    ema_decay, ema_warmup = config_ema(config)
    resumed = _read_resume_file(resume_from, config, optimizer_type) if resume_from else None
    if compiled_eval is None:
        compiled_eval = bool(getattr(config, "compiled_eval", False))
    compiled_eval_source = str(getattr(config, "compiled_eval_source", "float"))
    if not torch.cuda.is_available():
        raise lib.NnueHipError("training runs on the GPU only (no CPU fallback in this build)")
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_model(config, device) if model is None else model.to(device)
    if resumed is not None:
        model.load_state_dict(resumed["model_state_dict"])
    in_place = isinstance(train_loader, GpuLoader)  # GPU-resident dataset: batches are written straight into the input slots
    if in_place:
        hw = train_loader.dataset.output_hw  # the stored size unless the dataset resizes
    else:
        first_images, _ = next(iter(train_loader))
        hw = tuple(first_images.shape[2:])
    batch = int(config.batch_size)
    clip = float(config.max_grad_norm) if hasattr(config, "max_grad_norm") and config.max_grad_norm > 0 else 0.0
    if config.optimizer_type == "sgd":
        opt = dict(optimizer="sgd", momentum=float(config.momentum))
    else:
        opt = dict(optimizer="adam")
    mixes = in_place and train_loader.dataset.mixes
    if not mixes and (float(getattr(config, "mixup_alpha", 0.0)) > 0 or float(getattr(config, "cutmix_alpha", 0.0)) > 0):
        raise ValueError("the config sets mixup_alpha / cutmix_alpha but the train loader does not mix: build its dataset with "
                         "input_pipeline.dataset_from_config (a GpuLoader)")
    trainer = NnueTrainer(model, batch, hw, lr=float(config.learning_rate), weight_decay=float(config.weight_decay),
                          max_grad_norm=clip, use_graph=use_graph, input_slots=8 if in_place else 1,
                          label_smoothing=float(getattr(config, "label_smoothing", 0.0)), two_labels=mixes, weight_clip=weight_clip,
                          distill_alpha=distill_alpha, distill_temperature=distill_temperature, ema_decay=ema_decay,
                          ema_warmup=ema_warmup, **opt)
    if lr_schedule is None and getattr(config, "lr_schedule", False):
        lr_schedule = LrSchedule.from_config(config, len(train_loader))
    if isinstance(lr_schedule, LrSchedule):
        # the run's steps, and the whole decay with the constant that follows it (a run resumed under a longer max_epochs then
        # finds the same table)
        lr_schedule = lr_schedule.values(max(1, int(config.max_epochs) * len(train_loader), lr_schedule.lr_decay_iters + 2))
    if lr_schedule is not None:
        trainer.set_lr_schedule(lr_schedule)
    result = TrainResult()
    ckpt_dir = Path(checkpoint_dir) if checkpoint_dir is not None else None
    if save_last and ckpt_dir is None:
        raise ValueError("save_last needs checkpoint_dir")
    first_epoch = 0
    if resumed is not None:
        run = resumed["run_state"]
        trainer.load_state_dict(dict(run["trainer"], optimizer=resumed["optimizer_state_dict"]))
        _restore_loader_state(train_loader, run["loader"], device)
        result.history, result.steps = [dict(r) for r in run["history"]], int(run["steps"])
        result.best_val_f1, result.best_epoch = float(run["best_val_f1"]), int(run["best_epoch"])
        if ckpt_dir is not None and result.best_epoch >= 0 and (ckpt_dir / "best-model.ckpt").exists():
            result.checkpoint_path = ckpt_dir / "best-model.ckpt"
        first_epoch = int(run["epochs_done"])
    engine = None
    if compiled_eval:
        from .engine import EngineModel
        engine = EngineModel.from_model(model)
    for epoch in range(first_epoch, int(config.max_epochs)):
        model.train()
        if in_place:
            result.steps += train_epoch(trainer, train_loader, teacher=teacher)[1]
        else:
            for images, labels in train_loader:
                images = images.to(device, non_blocking=True)
                teacher_logits = None
                if teacher is not None:
                    with torch.no_grad():
                        teacher_logits = teacher(images).detach().to(torch.float32)
                trainer.step(images, labels.to(device, non_blocking=True).long(), teacher_logits=teacher_logits)
                result.steps += 1
        trainer = _density_check(trainer, log)
        model.eval()
        train_loss, train_metrics = evaluate.evaluate_model(model, train_loader, None, device)
        val_loss, val_metrics = evaluate.evaluate_model(model, val_loader, None, device)
        model.train()
        row = {"epoch": epoch, "train/epoch_loss": train_loss, "train/epoch_f1": train_metrics["f1"],
               "train/epoch_accuracy": train_metrics["acc"], "val/loss": val_loss, "val/f1": val_metrics["f1"],
               "val/accuracy": val_metrics["acc"]}
        if trainer.lr_table is not None:
            row["train/lr"] = trainer.lr_last
        line = (f"Epoch {epoch + 1}/{config.max_epochs} - Train Loss: {train_loss:.4f}, Train F1: {train_metrics['f1']:.4f}, "
                f"Train Acc: {train_metrics['acc']:.4f} | Val Loss: {val_loss:.4f}, Val F1: {val_metrics['f1']:.4f}, "
                f"Val Acc: {val_metrics['acc']:.4f}")
        if engine is not None:  # train.py:389-427
            engine.requantize(model)
            compiled = evaluate.evaluate_engine(engine, val_loader, source=compiled_eval_source)
            row.update({"compiled/f1": compiled["f1"], "compiled/accuracy": compiled["acc"],
                        "compiled/ms_per_sample": compiled["ms_per_sample"], "compiled/latent_density": compiled["latent_density"]})
            line += (f" | Compiled F1: {compiled['f1']:.4f}, Compiled Acc: {compiled['acc']:.4f}, "
                     f"Speed: {compiled['ms_per_sample']:.2f}ms/sample, Density: {compiled['latent_density']:.4f}")
        ema_state = None
        if trainer.flat_ema is not None:  # the averaged network, through the live parameters (every rank: a collective when sharded)
            with trainer.ema_weights():
                model.eval()
                ema_loss, ema_metrics = evaluate.evaluate_model(model, val_loader, None, device)
                model.train()
                row.update({"val_ema/loss": ema_loss, "val_ema/f1": ema_metrics["f1"], "val_ema/accuracy": ema_metrics["acc"]})
                line += f" | EMA Val Loss: {ema_loss:.4f}, EMA Val F1: {ema_metrics['f1']:.4f}, EMA Val Acc: {ema_metrics['acc']:.4f}"
                if engine is not None:
                    engine.requantize(model)
                    compiled = evaluate.evaluate_engine(engine, val_loader, source=compiled_eval_source)
                    row.update({"compiled_ema/f1": compiled["f1"], "compiled_ema/accuracy": compiled["acc"],
                                "compiled_ema/ms_per_sample": compiled["ms_per_sample"],
                                "compiled_ema/latent_density": compiled["latent_density"]})
                ema_state = {k: v.detach().cpu().clone() for k, v in trainer.ema_state().items()}
        result.history.append(row)
        log(line)
        # with save_last EVERY rank takes the trainer's state once per epoch, whatever its own best-F1 decision (under the
        # sharded update that call is a collective), and only rank 0 writes; without it everything is as it was
        state = _to_cpu(trainer.state_dict()) if save_last else None
        writes = ckpt_dir is not None and (not save_last or trainer.dp.rank == 0)

        def five_keys():
            keys = {"epoch": epoch,
                    "model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                    "optimizer_state_dict": state["optimizer"] if save_last else _to_cpu(trainer.optimizer_state_dict()),
                    "metrics": {"val_f1": val_metrics["f1"], "val_loss": val_loss},
                    "config_name": config.name}
            if ema_state is not None:  # (only with the average on: a run without it writes the five keys it always wrote)
                keys["ema_state_dict"] = ema_state
            return keys
        if val_metrics["f1"] > result.best_val_f1:
            result.best_val_f1, result.best_epoch = val_metrics["f1"], epoch
            if ckpt_dir is not None:
                result.checkpoint_path = ckpt_dir / "best-model.ckpt"
                if writes:
                    ckpt_dir.mkdir(parents=True, exist_ok=True)
                    torch.save(five_keys(), result.checkpoint_path)
        if save_last and writes:
            ckpt_dir.mkdir(parents=True, exist_ok=True)
            last = five_keys()
            last["run_state"] = {"trainer": {k: v for k, v in state.items() if k != "optimizer"},  # (the optimizer state is above)
                                 "epochs_done": epoch + 1, "steps": result.steps, "best_val_f1": float(result.best_val_f1),
                                 "best_epoch": result.best_epoch, "history": [_plain(r) for r in result.history],
                                 "loader": _loader_state(train_loader, device)}
            tmp = ckpt_dir / "last.ckpt.tmp"
            torch.save(last, tmp)
            os.replace(tmp, ckpt_dir / "last.ckpt")
    if test_loader is not None:
        model.eval()
        test_loss, test_metrics = evaluate.evaluate_model(model, test_loader, None, device)
        result.test = {"test/f1": test_metrics["f1"], "test/loss": test_loss}
    return result


# Active-feature density below which the gather kernels beat the dense products, by table size (measured on MI355X with
# `bench.py --density D`, which times both forms in one process; profiles/r03*_dens_*.json).  The thresholds
# are learnable (nnue.py:505-507), so the density is a property of the run, not of the shape: the check runs once per epoch on
# the counts the last step left, costs one read-back, and rebuilds the trainer (plans and graphs) only when it switches.
# NNUE_FT_DENSITY_SWITCH=0 disables it; a forced NNUE_FT_PATH is respected.
GATHER_BELOW_DENSITY = {"cache_resident_table": 0.0, "streamed_table": 0.0}  # 0 = the product form won at every measured density


def _density_check(trainer, log=print):
    if os.environ.get("NNUE_FT_DENSITY_SWITCH", "1") == "0" or os.environ.get("NNUE_FT_PATH", "auto") != "auto":
        return trainer
    if trainer.ft_path not in ("mfma", "bits") or not lib.ftb_supported(trainer.L1):
        return trainer
    density = trainer.active_stats()[0] / max(1, trainer.P)
    regime = "streamed_table" if trainer.F * trainer.L1 * 4 >= (200 << 20) else "cache_resident_table"
    want = "bits" if density < GATHER_BELOW_DENSITY[regime] else "mfma"
    if trainer.dp.world > 1:  # the same decision on every rank: take rank 0's
        import torch.distributed as dist
        flag = torch.tensor([1 if want == "bits" else 0], dtype=torch.int32, device=trainer.dev if trainer.dp.backend == "nccl" else "cpu")
        dist.broadcast(flag, src=dist.get_global_rank(trainer.dp.group, 0) if trainer.dp.group is not None else 0, group=trainer.dp.group)
        want = "bits" if int(flag.item()) else "mfma"
    if want == trainer.ft_path or (want == "mfma" and lib.ft_path(trainer.F, trainer.P, trainer.L1, trainer.B) != "mfma"):
        return trainer
    log(f"active-feature density {density:.4f}: FeatureTransformer kernels {trainer.ft_path} -> {want}")
    return trainer.rebuilt(want)


def train_model(config, model_type: str = "nnue", train_loader=None, val_loader=None, test_loader=None, **kwargs) -> int:
    """Same call shape and return value (0) as the reference's train_model; loaders are passed in."""
    if model_type != "nnue":
        raise ValueError(f"Unknown model type: {model_type} (EtinyNet training stays with the reference)")
    if train_loader is None or val_loader is None:
        raise ValueError("train_model needs train_loader and val_loader (the data pipeline is out of scope)")
    run_training(config, train_loader, val_loader, test_loader, **kwargs)
    return 0


def _plain(row: dict) -> dict:
    """A history row as plain Python numbers (what ``torch.load(..., weights_only=True)`` reads back)."""
    return {k: (int(v) if isinstance(v, (bool, int)) else float(v)) for k, v in row.items()}


def _loader_state(loader, device) -> Optional[dict]:
    """What the train loader carries from epoch to epoch: the GPU dataset's draw counter and the state of the generator its
    shuffle draws from -- its own, or the device's default one (``randperm(device=...)``) when it has none.  None for any
    other iterable: its state is the caller's."""
    if not isinstance(loader, GpuLoader):
        return None
    if loader.generator is not None:
        return {"dataset_step": int(loader.dataset.step), "generator": loader.generator.get_state().clone(), "device_rng": None}
    return {"dataset_step": int(loader.dataset.step), "generator": None, "device_rng": torch.cuda.get_rng_state(device).clone()}


def _restore_loader_state(loader, state: Optional[dict], device) -> None:
    if isinstance(loader, GpuLoader) != (state is not None):
        raise ValueError("the run was saved with another kind of train loader (GpuLoader or not)")
    if state is None:
        return
    if (loader.generator is not None) != (state["generator"] is not None):
        raise ValueError("the run was saved with a train loader whose shuffle generator was " +
                         ("its own" if state["generator"] is not None else "the device's default one"))
    loader.dataset.step = int(state["dataset_step"])
    if loader.generator is not None:
        loader.generator.set_state(state["generator"].cpu())
    else:
        torch.cuda.set_rng_state(state["device_rng"].cpu(), device)


def _read_resume_file(path, config, optimizer_type: str) -> dict:
    """The contents of a ``last.ckpt`` after the checks a resume refuses on (ValueError): no run state, another config,
    another optimizer type."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or "run_state" not in ckpt:
        raise ValueError(f"{path} holds no run state (a best-model.ckpt cannot be resumed from: save with save_last)")
    if ckpt.get("config_name") != config.name:
        raise ValueError(f"{path} was written by a run of config {ckpt.get('config_name')!r}, not {config.name!r}")
    saved = ckpt["run_state"]["trainer"].get("optimizer_type")
    if saved != optimizer_type:
        raise ValueError(f"{path} was written by a run with optimizer type {saved!r}, not {optimizer_type!r}")
    return ckpt


def _to_cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj
