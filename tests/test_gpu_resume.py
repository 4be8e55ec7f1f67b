"""Continuing a run exactly (NnueTrainer.state_dict / load_state_dict / load_optimizer_state_dict; run_training's
``save_last`` / ``resume_from``): the reference stores the optimizer state (checkpoint_manager.py:45-51) and loads it back
(checkpoint_manager.py:75-85); here the trainer also carries its step count and the per-step schedule's position, and the
train loop the input pipeline's draw counter and shuffle generator.  Every comparison is bitwise against the uninterrupted
run.  ``-m gpu``."""
import copy
import textwrap

import pytest
import torch

from nnue_hip import train_loop
from schedule_cases import (BIG_OPTS, DEV, RATES, big_model, big_trainer, optimizer_state, same_state, small_model, small_trainer)

pytestmark = pytest.mark.gpu

# the calls of one run: N = 5 steps, the state is taken, N more.  The second half starts with a one-step group (on a new trainer
# it records the plans), then a group of three that replays as one graph, then a single-step group.
FIRST_HALF = (("step", 0), ("many", (1, 2, 0)), ("step", 1))
SECOND_HALF = (("many", (2,)), ("many", (0, 1, 2)), ("many", (1,)))


def _run(tr, calls):
    losses = []
    for kind, arg in calls:
        losses.append(tr.step(slot=arg).clone().view(1) if kind == "step" else tr.step_many(arg).clone())
    return torch.cat(losses)


def _round_trip(obj, path):
    torch.save(obj, path)
    return torch.load(path, weights_only=True)


def _final(tr):
    extra = [tr.lr_pos.clone(), tr.lr_dev.clone()] + ([tr.adam_step_count.clone()] if tr.adam_step_count is not None else [])
    return [tr.flat_params.clone()] + optimizer_state(tr) + extra


def _builders(case, monkeypatch):
    if case == "small_sgd":
        return small_model, (lambda model: small_trainer(model)), RATES
    return big_model, (lambda model: big_trainer(monkeypatch, model, True, **BIG_OPTS["adam"])), RATES * 0.1


# ---------------------------------------------------------------------------------------------- 5. trainer level
@pytest.mark.parametrize("case", ("small_sgd", "big_adam_fused_next_forward"))
def test_resumed_trainer_continues_with_the_same_bits(tmp_path, monkeypatch, case):
    make_model, make_trainer, values = _builders(case, monkeypatch)
    # the uninterrupted run
    straight = make_trainer(make_model())
    straight.set_lr_schedule(values)
    _run(straight, FIRST_HALF)
    want_losses = _run(straight, SECOND_HALF)
    want = _final(straight)
    assert straight.steps_done == 10
    # N steps, state out through a file
    half_model = make_model()
    half = make_trainer(half_model)
    half.set_lr_schedule(values)
    _run(half, FIRST_HALF)
    sd = _round_trip({"trainer": half.state_dict(), "model": half_model.state_dict()}, tmp_path / "state.pt")
    assert sd["trainer"]["steps_done"] == 5 and sd["trainer"]["lr_schedule"]["position"] == 5 and sd["trainer"]["version"] == 1
    assert sd["trainer"]["optimizer_type"] == half.optimizer and sd["trainer"]["lr"] == float(values[4])
    assert sd["trainer"]["lr_schedule"]["values"].device.type == "cpu" and torch.equal(sd["trainer"]["lr_schedule"]["values"], values)
    del half
    # a NEW model and a NEW trainer
    new_model = make_model(seed=123)
    new_model.load_state_dict(sd["model"])
    new = make_trainer(new_model)
    new.set_lr_schedule(values)  # as a fresh run attaches it; the load then copies in place
    table = new.lr_table.data_ptr()
    new.load_state_dict(sd["trainer"])
    assert new.steps_done == 5 == new.lr_position == int(new.lr_pos) and new.lr_table.data_ptr() == table
    assert new.lr == float(values[5]) and float(new.lr_dev) == float(values[4])
    got_losses = _run(new, SECOND_HALF)
    assert new._plan_update_first is not None and ((0, 1, 2), "many") in new._g_local
    assert torch.equal(got_losses, want_losses), (got_losses, want_losses)
    for g, w in zip(_final(new), want):
        assert torch.equal(g, w)
    # ... and into a USED trainer whose graphs exist: they stay, the result is the same bits
    graphs, update_graph = dict(straight._g_local), straight._g_update
    buffers = [t.data_ptr() for t in [straight.flat_params, straight.lr_dev, straight.lr_pos, straight.lr_table] + straight._optimizer_buffers()]
    straight.model.load_state_dict(sd["model"])
    straight.load_state_dict(sd["trainer"])
    assert set(straight._g_local) == set(graphs) and all(straight._g_local[k] is graphs[k] for k in graphs)
    assert straight._g_update is update_graph
    assert buffers == [t.data_ptr() for t in [straight.flat_params, straight.lr_dev, straight.lr_pos, straight.lr_table]
                       + straight._optimizer_buffers()], "a buffer was re-bound"
    again = _run(straight, SECOND_HALF)
    assert torch.equal(again, want_losses)
    for g, w in zip(_final(straight), want):
        assert torch.equal(g, w)


def test_bare_optimizer_dict_of_a_best_model_checkpoint_loads():
    """load_optimizer_state_dict takes what best-model.ckpt holds (torch's own format) plus the step count; with a constant
    rate that is the whole state."""
    a = small_trainer(small_model())
    _run(a, FIRST_HALF)
    sd, params = train_loop._to_cpu(a.optimizer_state_dict()), {k: v.clone() for k, v in a.model.state_dict().items()}
    want_losses = _run(a, SECOND_HALF)
    model = small_model(seed=9)
    model.load_state_dict(params)
    b = small_trainer(model)
    b.load_optimizer_state_dict(sd, 5)
    assert b.steps_done == 5
    assert torch.equal(_run(b, SECOND_HALF), want_losses) and same_state(a, b)
    with pytest.raises(ValueError):
        b.load_optimizer_state_dict(sd, -1)


def test_first_step_plan_never_runs_after_a_load():
    """With steps_done > 0 the momentum-initialising plan (m <- g) must not run: a fresh trainer that loads a state and
    steps once equals the donor's next step, whose momentum was carried."""
    a = small_trainer(small_model())
    a.step(slot=0)
    sd, params = a.state_dict(), {k: v.clone() for k, v in a.model.state_dict().items()}
    a.step(slot=1)
    model = small_model(seed=4)
    model.load_state_dict(params)
    b = small_trainer(model)
    b.load_state_dict(sd)
    b.step(slot=1)
    assert same_state(a, b) and float(b.flat_momentum.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- 6. mismatched dicts
def test_mismatched_state_is_refused_and_changes_nothing(monkeypatch):
    sgd = small_trainer(small_model())
    sgd.set_lr_schedule(RATES)
    _run(sgd, FIRST_HALF)
    good = sgd.state_dict()
    adam = small_trainer(small_model(), optimizer="adam", momentum=0.0, lr=1e-3)
    adam.step(slot=0)
    plain = small_trainer(small_model(), momentum=0.0)
    plain.step(slot=0)
    index = {k: i for i, (k, _) in enumerate(sgd.model.named_parameters())}

    wrong_shape = copy.deepcopy(good)
    wrong_shape["optimizer"]["state"][index["input.bias"]]["momentum_buffer"] = torch.zeros(255, device=DEV)
    no_momentum = copy.deepcopy(good)
    for entry in no_momentum["optimizer"]["state"].values():
        del entry["momentum_buffer"]
    missing_entry = copy.deepcopy(good)
    del missing_entry["optimizer"]["state"][index["conv.weight"]]
    wrong_type = dict(copy.deepcopy(good), optimizer_type="adam")
    other_version = dict(copy.deepcopy(good), version=2)
    bad_schedule = copy.deepcopy(good)
    bad_schedule["lr_schedule"]["position"] = -3
    foreign = dict(copy.deepcopy(good), optimizer=adam.state_dict()["optimizer"])  # Adam's moments under the SGD label

    target = small_trainer(small_model(seed=2))
    target.set_lr_schedule(RATES.flip(0), position=1)
    target.step(slot=0)
    before = [t.clone() for t in [target.flat_params, target.flat_momentum, target.lr_dev, target.lr_pos, target.lr_table]]
    facts = (target.steps_done, target.lr_position, target.lr)
    for name, sd in (("shape", wrong_shape), ("momentum missing", no_momentum), ("entry missing", missing_entry), ("type", wrong_type),
                     ("version", other_version), ("schedule", bad_schedule), ("foreign moments", foreign)):
        with pytest.raises(ValueError):
            target.load_state_dict(sd)
        now = [target.flat_params, target.flat_momentum, target.lr_dev, target.lr_pos, target.lr_table]
        assert all(torch.equal(x, y) for x, y in zip(now, before)), name
        assert facts == (target.steps_done, target.lr_position, target.lr), name
    # the other directions: an SGD state into Adam, a momentum state into a trainer built without momentum
    for other in (adam, plain):
        kept = [other.flat_params.clone()] + optimizer_state(other)
        with pytest.raises(ValueError):
            other.load_state_dict(dict(copy.deepcopy(good), optimizer_type=other.optimizer))
        assert all(torch.equal(x, y) for x, y in zip([other.flat_params] + other._optimizer_buffers(), kept))
    target.load_state_dict(good)  # and the good one does load
    assert target.steps_done == 5 and torch.equal(target.flat_momentum, sgd.flat_momentum) and torch.equal(target.lr_table.cpu(), RATES)


# ---------------------------------------------------------------------------------------------- 7 / 8. run_training
CONFIG_TEXT = """
    name = "nnue_vision_test"
    batch_size = 16
    num_workers = 0
    num_classes = 10
    l1_size = 256
    l2_size = 32
    l3_size = 16
    input_size = 32
    grid_size = 10
    num_features_per_square = 8
    learning_rate = 0.02
    weight_decay = 2e-4
    momentum = 0.9
    optimizer_type = "{opt}"
    subset = 1.0
    max_epochs = {epochs}
    max_grad_norm = 1.0
    use_augmentation = False
    keep_alive = True
    log_dir = "logs"
    project_name = "test"
    lr_schedule = True
    use_cosine_scheduler = True
    warmup_iters = 3
    lr_decay_iters = 28
    min_lr = 1e-4
"""


def _config(tmp_path, epochs, opt="sgd", name=None):
    path = tmp_path / f"train_{opt}_{epochs}_{name}.py"
    text = textwrap.dedent(CONFIG_TEXT.format(opt=opt, epochs=epochs))
    if name is not None:
        text = text.replace('"nnue_vision_test"', f'"{name}"')
    path.write_text(text)
    return train_loop.load_config(path)


def _loaders(own_generator: bool):
    """6 x 16 + 7 seeded uint8 images with a learnable signal; the train loader augments and shuffles."""
    from nnue_hip.input_pipeline import GpuImageDataset
    g = torch.Generator().manual_seed(11)
    n = 6 * 16 + 7
    labels = torch.randint(0, 10, (n,), generator=g)
    images = (torch.randint(0, 160, (n, 32, 32, 3), generator=g) + labels.view(-1, 1, 1, 1) * 9).to(torch.uint8)
    train = GpuImageDataset(images, labels, augment="light", seed=3, num_classes=10)
    val = GpuImageDataset(images[:48], labels[:48], augment=False, num_classes=10)
    gen = torch.Generator().manual_seed(21) if own_generator else None
    if not own_generator:
        torch.cuda.manual_seed(77)
    return train.loader(16, shuffle=True, generator=gen), val.loader(16)


def _train(cfg, own_generator, ckpt_dir, **kw):
    train, val = _loaders(own_generator)
    torch.manual_seed(0)
    model = train_loop.build_model(cfg, DEV)
    res = train_loop.run_training(cfg, train, val, model=model, checkpoint_dir=ckpt_dir, log=lambda s: None, **kw)
    return res, {k: v.detach().clone() for k, v in model.state_dict().items()}, train


@pytest.mark.parametrize("own_generator", (True, False), ids=("loader_generator", "device_default_generator"))
def test_run_training_resumed_at_an_epoch_boundary_is_the_uninterrupted_run(tmp_path, own_generator):
    full, full_params, _ = _train(_config(tmp_path, 4), own_generator, tmp_path / "full", save_last=True)
    assert full.steps == 4 * 7 and len(full.history) == 4
    lrs = [row["train/lr"] for row in full.history]
    assert len(set(lrs)) == 4 and lrs[-1] < lrs[0], lrs  # the rate moved, per step: each row has its epoch's last value
    part, _, _ = _train(_config(tmp_path, 2), own_generator, tmp_path / "resumed", save_last=True)
    assert part.steps == 2 * 7 and part.history == full.history[:2]
    last = torch.load(tmp_path / "resumed" / "last.ckpt", weights_only=True)
    assert set(last) == {"epoch", "model_state_dict", "optimizer_state_dict", "metrics", "config_name", "run_state"}
    run = last["run_state"]
    assert run["epochs_done"] == 2 and run["steps"] == 14 and "optimizer" not in run["trainer"] and run["trainer"]["steps_done"] == 14
    assert run["trainer"]["lr_schedule"]["position"] == 14 and run["loader"]["dataset_step"] > 0
    assert (run["loader"]["generator"] is not None) == own_generator and (run["loader"]["device_rng"] is None) == own_generator
    assert last["metrics"] == {"val_f1": part.history[1]["val/f1"], "val_loss": part.history[1]["val/loss"]}
    resumed, resumed_params, _ = _train(_config(tmp_path, 4), own_generator, tmp_path / "resumed",
                                        resume_from=tmp_path / "resumed" / "last.ckpt", save_last=True)
    assert resumed.steps == full.steps and len(resumed.history) == 4
    assert resumed.history[2:] == full.history[2:], (resumed.history[2:], full.history[2:])
    assert resumed.history[:2] == full.history[:2]
    assert (resumed.best_val_f1, resumed.best_epoch) == (full.best_val_f1, full.best_epoch)
    for k, v in full_params.items():
        assert torch.equal(resumed_params[k], v), k
    # both runs end on the same last.ckpt contents; best-model.ckpt keeps exactly its five keys
    a, b = (torch.load(tmp_path / d / "last.ckpt", weights_only=True) for d in ("full", "resumed"))
    assert a["run_state"]["epochs_done"] == 4 == b["run_state"]["epochs_done"]
    assert all(torch.equal(a["model_state_dict"][k], b["model_state_dict"][k]) for k in a["model_state_dict"])
    assert not (tmp_path / "resumed" / "last.ckpt.tmp").exists()
    assert full.checkpoint_path is not None, "validation F1 never rose above 0 on the training images themselves"
    best = torch.load(full.checkpoint_path, weights_only=True)
    assert set(best) == {"epoch", "model_state_dict", "optimizer_state_dict", "metrics", "config_name"}


def test_resume_refuses_files_it_cannot_continue(tmp_path):
    cfg = _config(tmp_path, 1)
    res, _, _ = _train(cfg, True, tmp_path / "run", save_last=True)
    last = tmp_path / "run" / "last.ckpt"
    assert last.exists()
    if res.checkpoint_path is not None:
        with pytest.raises(ValueError, match="run state"):
            _train(_config(tmp_path, 2), True, tmp_path / "x", resume_from=res.checkpoint_path)
    bare = {k: v for k, v in torch.load(last, weights_only=True).items() if k != "run_state"}
    torch.save(bare, tmp_path / "bare.ckpt")
    with pytest.raises(ValueError, match="run state"):
        _train(_config(tmp_path, 2), True, tmp_path / "x", resume_from=tmp_path / "bare.ckpt")
    with pytest.raises(ValueError, match="config"):
        _train(_config(tmp_path, 2, name="another_config"), True, tmp_path / "x", resume_from=last)
    with pytest.raises(ValueError, match="optimizer type"):
        _train(_config(tmp_path, 2, opt="adam"), True, tmp_path / "x", resume_from=last)
    with pytest.raises(ValueError, match="checkpoint_dir"):
        _train(cfg, True, None, save_last=True)


def test_without_the_new_options_rows_and_files_are_as_before(tmp_path):
    cfg = _config(tmp_path, 1)
    cfg.lr_schedule = False
    res, _, _ = _train(cfg, True, tmp_path / "plain")
    assert set(res.history[0]) == {"epoch", "train/epoch_loss", "train/epoch_f1", "train/epoch_accuracy", "val/loss", "val/f1", "val/accuracy"}
    assert not (tmp_path / "plain" / "last.ckpt").exists()
