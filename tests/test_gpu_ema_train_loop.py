"""The weight average in the train loop and around the trainer (nnue_hip/train_loop.py::run_training with the config attributes
``ema_decay`` / ``ema_warmup``; ``NnueTrainer.ema_weights()`` with the engine's quantisers): the epoch rows and checkpoints gain
the average's entries and nothing else moves, a run resumed from ``last.ckpt`` continues with the bits of the uninterrupted one,
and ``EngineModel.from_model`` / ``requantize`` under the context see the averaged network.  ``-m gpu``."""
import copy
import gc

import pytest
import torch

import ema_cases as ec
import trainer_modes as tm
from test_gpu_resume import _config, _train

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMA_ROWS = {"val_ema/loss", "val_ema/f1", "val_ema/accuracy"}
COMPILED_ROWS = {"compiled_ema/f1", "compiled_ema/accuracy", "compiled_ema/ms_per_sample", "compiled_ema/latent_density"}
TIMED = ("compiled/ms_per_sample", "compiled_ema/ms_per_sample")  # wall-clock figures: never equal between runs


@pytest.fixture(autouse=True)
def _collect_trainers():
    yield
    gc.collect()


def _cfg(tmp_path, epochs, **attrs):
    cfg = _config(tmp_path, epochs)
    for k, v in attrs.items():
        setattr(cfg, k, v)
    return cfg


def _untimed(history):
    return [{k: v for k, v in row.items() if k not in TIMED} for row in history]


def test_run_training_rows_checkpoints_and_resume(tmp_path):
    on = dict(ema_decay=0.9, ema_warmup=True, compiled_eval=True)
    full, full_params, _ = _train(_cfg(tmp_path, 3, **on), True, tmp_path / "full", save_last=True)
    plain, plain_params, _ = _train(_cfg(tmp_path, 3, compiled_eval=True), True, tmp_path / "plain", save_last=True)
    assert len(full.history) == 3
    for row, without in zip(_untimed(full.history), _untimed(plain.history)):
        assert EMA_ROWS | (COMPILED_ROWS - set(TIMED)) <= set(row) and not (EMA_ROWS | COMPILED_ROWS) & set(without)
        assert {k: v for k, v in row.items() if k not in EMA_ROWS | COMPILED_ROWS} == without  # nothing of the run reads the average
    assert (full.best_val_f1, full.best_epoch) == (plain.best_val_f1, plain.best_epoch)  # the best model is chosen as before
    assert all(torch.equal(full_params[k], plain_params[k]) for k in plain_params)
    # the averaged network is another network than the trained one: its validation loss is its own
    assert any(row["val_ema/loss"] != row["val/loss"] for row in full.history)
    last = torch.load(tmp_path / "full" / "last.ckpt", weights_only=True)
    assert set(last) == {"epoch", "model_state_dict", "optimizer_state_dict", "metrics", "config_name", "run_state", "ema_state_dict"}
    ema = last["ema_state_dict"]
    assert set(ema) == set(last["model_state_dict"]) - {"nnue2score"}
    assert all(ema[k].shape == last["model_state_dict"][k].shape for k in ema)
    assert not torch.equal(ema["input.weight"], last["model_state_dict"]["input.weight"])
    saved = last["run_state"]["trainer"]["ema"]
    assert saved["decay"] == 0.9 and saved["warmup"] is True and saved["position"] == full.steps
    assert all(torch.equal(saved["state"][k], ema[k]) for k in ema)
    assert set(torch.load(tmp_path / "plain" / "last.ckpt", weights_only=True)) == set(last) - {"ema_state_dict"}
    if full.checkpoint_path is not None:
        assert "ema_state_dict" in torch.load(full.checkpoint_path, weights_only=True)
    # two epochs, then the third from last.ckpt: the rows and the average of the uninterrupted run
    part, _, _ = _train(_cfg(tmp_path, 2, **on), True, tmp_path / "resumed", save_last=True)
    assert _untimed(part.history) == _untimed(full.history[:2])
    resumed, resumed_params, _ = _train(_cfg(tmp_path, 3, **on), True, tmp_path / "resumed", resume_from=tmp_path / "resumed" / "last.ckpt",
                                        save_last=True)
    assert _untimed(resumed.history) == _untimed(full.history)
    assert all(torch.equal(resumed_params[k], full_params[k]) for k in full_params)
    again = torch.load(tmp_path / "resumed" / "last.ckpt", weights_only=True)
    assert all(torch.equal(again["ema_state_dict"][k], ema[k]) for k in ema)
    # a run without the average cannot continue this one, nor the other way round
    with pytest.raises(ValueError, match="weight average"):
        _train(_cfg(tmp_path, 3, compiled_eval=True), True, tmp_path / "x", resume_from=tmp_path / "resumed" / "last.ckpt")
    with pytest.raises(ValueError, match="weight average"):
        _train(_cfg(tmp_path, 4, **on), True, tmp_path / "y", resume_from=tmp_path / "plain" / "last.ckpt")


def test_the_engine_quantisers_under_ema_weights(monkeypatch):
    from nnue_hip.engine import EngineModel
    row = tm.BY_NAME["A"]
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    with tm.trainer_for(cfg, ema_decay=ec.DECAY, weight_clip=1.0) as (tr, _):
        for images, labels in ec.fresh_batches(3, cfg["batch"], cfg["image"], cfg["classes"]):
            tr.step(images.to(DEV), labels.to(DEV))
        torch.cuda.synchronize()
        model = tr.model
        fresh = copy.deepcopy(model)
        named = dict(fresh.named_parameters())
        for k, v in tr.ema_state().items():
            named[k].data = v.detach().clone()
        want, trained = EngineModel.from_model(fresh), EngineModel.from_model(model)
        with tr.ema_weights():
            live = EngineModel.from_model(model)
            trained.requantize(model)
        assert live.tensors.keys() == want.tensors.keys()
        for k in want.tensors:
            assert torch.equal(live.tensors[k], want.tensors[k]), k
            assert torch.equal(trained.tensors[k], want.tensors[k]), k
        back = EngineModel.from_model(model)  # outside the context: the trained network again
        assert any(not torch.equal(back.tensors[k], want.tensors[k]) for k in want.tensors)
