"""Soft targets through NnueTrainer, the GPU input pipeline and the training driver.  ``-m gpu``.

* One whole optimizer step with label_smoothing = 0.1 and a batch-constant lam = 0.3 is held to the float64 oracle through
  linearity: the backward is linear in d_logits, so the expected gradient (and loss) is
      0.9 * 0.3 * G(labels) + 0.9 * 0.7 * G(labels_b) + (0.1 / C) * sum_c G(all labels = c)
  with G = oracle.loss_and_grads_explicit on the same batch (C + 2 oracle calls), at tests/trainer_modes.py's bars
  (``compare_held``), in rows A, A_tail_in_dx (the SOFT arm inside the d_x launch) and A_k4_clip (bucketed stacks).
* Eager steps, graph steps and a step group are bitwise equal, as those rows promise.
* A trainer with the defaults makes today's calls: the plain entry points, and the same parameters as a second one.
* train_epoch on a mixing dataset with a short last batch, fed in place, equals copy feeding; without two_labels it raises.
* run_training from a config with the three attributes: two epochs, finite losses, val/loss is plain cross-entropy, and a run
  resumed after epoch 1 has the bits of the uninterrupted one.
"""
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from trainer_modes import BY_NAME, CallLog, compare_held, draw_batch, geometry, held_by, hyper, same, set_knobs, snapshot, trainer_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, LAM = 0.1, 0.3
ROWS = ("A", "A_tail_in_dx", "A_k4_clip")


def soft_batch(cfg, params64, gen):
    images, labels = draw_batch(cfg, params64, geometry(cfg)["stride"], gen, cfg["batch"])
    labels_b = torch.randint(0, cfg["classes"], labels.shape, generator=gen)
    return images, labels, labels_b, torch.full(labels.shape, LAM)


def oracle_soft_step(cfg, params64, images, labels, labels_b):
    """The expected step in float64, by linearity in the targets; compare_held's ``ref``."""
    import nnue_oracle as orc
    C, stride = cfg["classes"], geometry(cfg)["stride"]
    terms = [((1 - EPS) * LAM, labels), ((1 - EPS) * (1 - LAM), labels_b)] + [(EPS / C, torch.full_like(labels, c)) for c in range(C)]
    loss, grads, logits = 0.0, None, None
    for weight, y in terms:
        logits, l, g, _ = orc.loss_and_grads_explicit(params64, images.double(), y, stride, cfg["clip"])
        loss += weight * float(l)
        grads = {k: weight * v for k, v in g.items()} if grads is None else {k: grads[k] + weight * g[k] for k in grads}
    norm = float(torch.sqrt(sum((grads[k] ** 2).sum() for k in orc.TRAINABLE_KEYS)))
    p = {k: v.clone() for k, v in params64.items()}
    state, hp = {}, hyper(cfg)
    orc.sgd_step(p, grads, state, hp["lr"], hp["momentum"], hp["weight_decay"], 0.5 * norm)
    return dict(logits=logits, loss=loss, norm=norm, grads=grads, before=params64, after=p, state=state, max_grad_norm=0.5 * norm)


def feed(tr, batch, slot, max_grad_norm):
    images, labels, labels_b, lam = (t.to(DEV) for t in batch)
    tr.max_grad_norm = max_grad_norm
    return tr.step(images, labels, slot=slot, labels_b=labels_b, lam=lam)


@pytest.mark.parametrize("name", ROWS)
def test_a_soft_step_follows_the_oracle_and_graphs_and_groups_are_bitwise(name, monkeypatch):
    row = BY_NAME[name]
    cfg = row.config
    set_knobs(monkeypatch, row)
    soft = dict(label_smoothing=EPS, two_labels=True, input_slots=3)
    with trainer_for(cfg, use_graph=False, **soft) as (eager, params):
        p64 = {k: v.double() for k, v in params.items()}
        gen = torch.Generator().manual_seed(31)
        batches = [soft_batch(cfg, p64, gen) for _ in range(3)]
        ref = oracle_soft_step(cfg, p64, *batches[0][:3])
        was = {k: v.detach().clone() for k, v in eager.p.items()}
        with CallLog() as log:
            loss = feed(eager, batches[0], 0, ref["max_grad_norm"])
        torch.cuda.synchronize()
        entry = "nnue_classifier_train_step_soft_bucketed" if cfg["K"] > 1 else "nnue_classifier_train_step_soft"
        ran = [n for _, n, _ in log.entries if n.startswith("nnue_classifier_train_step")]
        assert ran and set(ran) == {entry}, ran
        assert eager.mode.phases == row.modes["phases"]
        ratios = {}
        fails = compare_held(dict(held_by(eager, was), logits=eager.logits, loss=loss, norm=eager.grad_norm), ref, eager.B, eager.B, None,
                             f"{name} soft step", ratios)
        print("SOFT_TRAINER", name, {k: round(v, 4) for k, v in ratios.items()})
        assert not fails, "; ".join(fails)
        assert set(ratios) >= {"logits", "loss", "norm", "grad", "parameters", "update", "momentum"}
        # ---- the same step and two more, then the three slots once more, as eager steps, graph steps and one step group
        losses, states = [loss.clone()], [snapshot(eager)]
        for s in (1, 2):
            losses.append(feed(eager, batches[s], s, ref["max_grad_norm"]).clone())
            states.append(snapshot(eager))
        with trainer_for(cfg, use_graph=True, **soft) as (single, _), trainer_for(cfg, use_graph=True, **soft) as (group, _):
            for s in (0, 1, 2):
                for tr in (single, group):
                    got = feed(tr, batches[s], s, ref["max_grad_norm"])
                    torch.cuda.synchronize()
                    assert torch.equal(got, losses[s]) and same(snapshot(tr), states[s]), f"{name} step {s}: the graph step is not the eager one"
            want = torch.stack([eager.step(slot=s).clone() for s in (0, 1, 2)])
            got_single = torch.stack([single.step(slot=s).clone() for s in (0, 1, 2)])
            got_group = group.step_many((0, 1, 2)).clone()
            torch.cuda.synchronize()
            assert torch.equal(got_single, want) and same(snapshot(single), snapshot(eager)), f"{name}: graph steps on the slots"
            assert torch.equal(got_group, want) and same(snapshot(group), snapshot(eager)), f"{name}: the step group"
            for s in (0, 1, 2):  # each slot kept its own second labels and weights
                assert torch.equal(group.soft_inputs[s][0].cpu(), batches[s][2]) and torch.equal(group.soft_inputs[s][1].cpu(), batches[s][3])
                assert len(group.inputs[s]) == 2


def test_label_smoothing_is_a_constant_of_the_local_plan_and_of_the_state(monkeypatch):
    row = BY_NAME["A"]
    cfg = row.config
    set_knobs(monkeypatch, row)
    gen = torch.Generator().manual_seed(5)
    images, labels = torch.rand(cfg["batch"], 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (cfg["batch"],), generator=gen).to(DEV)
    with trainer_for(cfg, label_smoothing=EPS) as (a, _), trainer_for(cfg) as (b, _):
        assert a.soft_inputs is None and a.label_smoothing == EPS and b.label_smoothing == 0.0
        a.step(images, labels)
        a.step(images, labels)
        assert a._g_local and a._plan_local is not None
        update_plan = a._plan_update
        a.label_smoothing = 0.0  # re-records the local plan, drops its graphs, keeps the update plan
        assert not a._g_local and a._plan_local is None and a._plan_update is update_plan
        with pytest.raises(ValueError, match="label_smoothing"):
            a.label_smoothing = 1.0
        with pytest.raises(ValueError, match="two_labels"):
            a.step(images, labels, labels_b=labels, lam=torch.ones(cfg["batch"], device=DEV))
        sd = a.state_dict()
        assert sd["label_smoothing"] == 0.0
        b.load_state_dict(sd)
        a.label_smoothing = EPS
        sd = a.state_dict()
        assert sd["label_smoothing"] == EPS
        before = snapshot(b)
        with pytest.raises(ValueError, match="label_smoothing"):
            b.load_state_dict(sd)
        assert same(snapshot(b), before)
        b.load_state_dict({k: v for k, v in sd.items() if k != "label_smoothing"})  # a state from before the key existed: 0


def test_a_default_trainer_makes_the_plain_calls(monkeypatch):
    for name in ("A", "A_k4_clip"):
        row = BY_NAME[name]
        cfg = row.config
        set_knobs(monkeypatch, row)
        gen = torch.Generator().manual_seed(9)
        data = [(torch.rand(cfg["batch"], 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (cfg["batch"],), generator=gen).to(DEV))
                for _ in range(3)]
        # two_labels with its initial -1 / 1 and no smoothing is one label per sample as well: the soft arm, the plain bits
        with trainer_for(cfg) as (a, _), trainer_for(cfg) as (b, _), trainer_for(cfg, two_labels=True) as (c, _):
            assert a.soft_inputs is None and a.labels_b is None and not a.two_labels and a.label_smoothing == 0.0
            assert all(len(slot) == 2 for slot in a.inputs + c.inputs)
            with CallLog() as log:
                for x, y in data:
                    a.step(x, y)
            ran = {n for _, n, _ in log.entries if n.startswith("nnue_classifier_train_step")}
            assert ran == {"nnue_classifier_train_step_bucketed" if cfg["K"] > 1 else "nnue_classifier_train_step"}, ran
            for x, y in data:
                b.step(x, y)
                c.step(x, y)
            torch.cuda.synchronize()
            assert same(snapshot(a), snapshot(b)), name
            assert same(snapshot(c), snapshot(a)), f"{name}: lam = 1 without smoothing is not the plain step"


def small_model():
    import nnue
    torch.manual_seed(0)
    return nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).cuda()


def test_mixing_epoch_in_place_equals_copy_feeding():
    """tests/test_gpu_augment_policy.py::test_medium_epoch_in_place_equals_copy_feeding with a dataset that mixes, at its bars."""
    from nnue_hip.input_pipeline import GpuImageDataset, train_epoch
    from nnue_hip.trainer import NnueTrainer
    rng = np.random.RandomState(10)
    images, labels = rng.randint(0, 256, size=(64 * 5 + 9, 24, 24, 3), dtype=np.uint8), rng.randint(0, 10, size=64 * 5 + 9)
    models, sums = [], []
    for mode in ("sequential", "in_place"):
        model = small_model()
        ds = GpuImageDataset(images, labels, augment="medium", out_hw=(32, 32), seed=5, mixup_alpha=0.4, cutmix_alpha=1.0)
        tr = NnueTrainer(model, 64, ds.output_hw, lr=0.01, momentum=0.9, input_slots=2, label_smoothing=EPS, two_labels=True)
        loader = ds.loader(64, shuffle=True, generator=torch.Generator().manual_seed(11))
        if mode == "sequential":
            losses = []
            for idx in loader.index_batches():
                x, y, y2, lam = ds.mixed_batch(idx)
                losses.append(float(tr.step(x, y, labels_b=y2, lam=lam)))
            total, n = sum(losses), len(losses)
            assert all(np.isfinite(losses))
        else:
            s, n = train_epoch(tr, loader)
            total = float(s)
            assert bool((tr.soft_inputs[0][1] < 1).any()) or bool((tr.soft_inputs[1][1] < 1).any())
        assert n == 6 and np.isfinite(total) and ds.step == 6
        models.append(model)
        sums.append(total)
    assert abs(sums[0] - sums[1]) <= 1e-4 * abs(sums[0])
    for (k, p), (_, q) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert float((p - q).detach().abs().max()) <= 1e-5 * max(1.0, float(q.detach().abs().max())), k


def test_train_epoch_refuses_a_mixing_dataset_without_two_labels():
    from nnue_hip.input_pipeline import GpuImageDataset, train_epoch
    from nnue_hip.trainer import NnueTrainer
    rng = np.random.RandomState(1)
    ds = GpuImageDataset(rng.randint(0, 256, size=(32, 32, 32, 3), dtype=np.uint8), rng.randint(0, 10, size=32), cutmix_alpha=1.0)
    tr = NnueTrainer(small_model(), 16, (32, 32), lr=0.01, label_smoothing=EPS)
    with pytest.raises(ValueError, match="two_labels"):
        train_epoch(tr, ds.loader(16))
    assert tr.steps_done == 0 and ds.step == 0


# ------------------------------------------------------------------------------------------------- the training driver
def _config(tmp_path, epochs):
    from nnue_hip import train_loop
    from test_train_loop import CONFIG_TEXT
    path = tmp_path / f"train_soft_{epochs}.py"
    path.write_text(textwrap.dedent(CONFIG_TEXT.format(opt="sgd", lr=0.02, epochs=epochs))
                    + "label_smoothing = 0.1\nmixup_alpha = 0.4\ncutmix_alpha = 1.0\nuse_augmentation = True\naugmentation_strength = 'light'\n")
    return train_loop.load_config(path)


def _train(cfg, ckpt_dir, **kw):
    from nnue_hip import train_loop
    from nnue_hip.input_pipeline import dataset_from_config
    g = torch.Generator().manual_seed(11)
    n = 6 * 16 + 7
    labels = torch.randint(0, 10, (n,), generator=g)
    images = (torch.randint(0, 160, (n, 32, 32, 3), generator=g) + labels.view(-1, 1, 1, 1) * 9).to(torch.uint8)
    train = dataset_from_config(cfg, images, labels, train=True, seed=3)
    val = dataset_from_config(cfg, images[:48], labels[:48], train=False)
    assert train.mixes and not val.mixes
    torch.manual_seed(0)
    model = train_loop.build_model(cfg, DEV)
    res = train_loop.run_training(cfg, train.loader(16, shuffle=True, generator=torch.Generator().manual_seed(21)), val.loader(16),
                                  model=model, checkpoint_dir=ckpt_dir, log=lambda s: None, **kw)
    return res, model, val


def test_run_training_with_the_three_attributes_and_a_resume(tmp_path):
    from nnue_hip import train_loop
    full, model, val = _train(_config(tmp_path, 2), tmp_path / "full", save_last=True)
    assert full.steps == 2 * 7 and len(full.history) == 2
    assert all(np.isfinite(row["train/epoch_loss"]) and np.isfinite(row["val/loss"]) for row in full.history)
    # val/loss is plain cross-entropy on the unmixed validation set: the mean of the per-batch means
    model.eval()
    with torch.no_grad():
        per_batch = [float(F.cross_entropy(model(x).double(), y)) for x, y in val.loader(16)]
    plain = sum(per_batch) / len(per_batch)
    assert abs(full.history[-1]["val/loss"] - plain) <= 1e-4 * max(1.0, abs(plain))
    last = torch.load(tmp_path / "full" / "last.ckpt", weights_only=True)
    assert last["run_state"]["trainer"]["label_smoothing"] == pytest.approx(0.1)
    # stop after epoch 1, resume: the bits of the uninterrupted run
    part, _, _ = _train(_config(tmp_path, 1), tmp_path / "resumed", save_last=True)
    assert part.history == full.history[:1]
    resumed, resumed_model, _ = _train(_config(tmp_path, 2), tmp_path / "resumed", save_last=True,
                                       resume_from=tmp_path / "resumed" / "last.ckpt")
    assert resumed.steps == full.steps and resumed.history == full.history
    for (k, v), (_, w) in zip(model.state_dict().items(), resumed_model.state_dict().items()):
        assert torch.equal(v, w), k
    # the alphas without a dataset that mixes are refused, not ignored
    cfg = _config(tmp_path, 1)
    from nnue_hip.input_pipeline import GpuImageDataset
    ds = GpuImageDataset(torch.zeros(16, 32, 32, 3, dtype=torch.uint8), torch.zeros(16, dtype=torch.int64))
    with pytest.raises(ValueError, match="does not mix"):
        train_loop.run_training(cfg, ds.loader(16), ds.loader(16), log=lambda s: None)
