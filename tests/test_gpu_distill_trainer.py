"""Distillation through NnueTrainer, the GPU input pipeline, the training driver and two data-parallel ranks.  ``-m gpu``.

* One whole optimizer step with label_smoothing = 0.1, distill_alpha = 0.7 and T = 2 is held to float64: the expected step is
  oracle.model_forward_loop on parameters that require grad, the loss of include/nnue_hip.h ("soft targets", the teacher arm)
  written in torch -- (1 - alpha) F.cross_entropy(label_smoothing) + alpha T^2 KL(softmax(u / T) || softmax(z / T)), batch mean --
  its autograd backward, then oracle.sgd_step (linearity in the targets does not reach this loss), at tests/trainer_modes.py's
  bars (``compare_held``), in rows A, A_tail_in_dx (the DISTILL arm inside the d_x launch) and A_k4_clip (bucketed stacks).
* Eager steps, graph steps and a step group are bitwise equal, and every slot keeps its own teacher logits.
* A trainer with the defaults makes today's calls and leaves the same parameters as a second one; the two values travel through
  state_dict / load_state_dict / rebuilt.
* train_epoch with a teacher and a short last batch, fed in place, equals copy feeding.
* run_training from a config with the two attributes and a drop-in NNUE teacher: two epochs, finite losses, val/loss is plain
  cross-entropy, and a run resumed after epoch 1 has the bits of the uninterrupted one.
* Two gloo ranks on one GPU (tests/test_gpu_weight_clip_dp.py's driver pattern), each on its half of the batch and of the teacher
  logits: every rank equals the single-rank step on the global batch at ``compare_held``'s bars, and the ranks are bitwise alike.
"""
import gc
import os
import socket
import textwrap
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trainer_modes as tm
from trainer_modes import BY_NAME, CallLog, compare_held, draw_batch, geometry, held_by, hyper, same, set_knobs, snapshot, trainer_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, ALPHA, T = 0.1, 0.7, 2.0
ROWS = ("A", "A_tail_in_dx", "A_k4_clip")
DISTILL = dict(label_smoothing=EPS, distill_alpha=ALPHA, distill_temperature=T)


@pytest.fixture(autouse=True)
def _collect_trainers():
    """(tests/test_gpu_weight_clip_dp.py) a failed test's trainers must not be collected inside the next test's graph capture."""
    yield
    gc.collect()


def distill_loss(logits, labels, teacher):
    """The definition, in torch: batch mean of (1 - alpha) L_soft + alpha T^2 KL(q || pT)."""
    kl = F.kl_div(torch.log_softmax(logits / T, dim=1), torch.log_softmax(teacher / T, dim=1), reduction="batchmean", log_target=True)
    return (1 - ALPHA) * F.cross_entropy(logits, labels, label_smoothing=EPS) + ALPHA * T * T * kl


def distill_batch(cfg, params64, gen):
    images, labels = draw_batch(cfg, params64, geometry(cfg)["stride"], gen, cfg["batch"])
    return images, labels, torch.randn(cfg["batch"], cfg["classes"], generator=gen) * 2


def oracle_distill_step(cfg, params64, images, labels, teacher):
    """The expected step in float64 through autograd on the loop form; compare_held's ``ref``."""
    import nnue_oracle as orc
    q = {k: v.detach().clone().requires_grad_(k in orc.TRAINABLE_KEYS) for k, v in params64.items()}
    logits = orc.model_forward_loop(q, images.double(), geometry(cfg)["stride"], None, cfg["clip"])
    loss = distill_loss(logits, labels, teacher.double())
    loss.backward()
    grads = {k: q[k].grad for k in orc.TRAINABLE_KEYS}
    norm = float(torch.sqrt(sum((grads[k] ** 2).sum() for k in orc.TRAINABLE_KEYS)))
    p = {k: v.clone() for k, v in params64.items()}
    state, hp = {}, hyper(cfg)
    orc.sgd_step(p, grads, state, hp["lr"], hp["momentum"], hp["weight_decay"], 0.5 * norm)
    return dict(logits=logits.detach(), loss=float(loss.detach()), norm=norm, grads=grads, before=params64, after=p, state=state, max_grad_norm=0.5 * norm)


def feed(tr, batch, slot, max_grad_norm):
    images, labels, teacher = (t.to(DEV) for t in batch)
    tr.max_grad_norm = max_grad_norm
    return tr.step(images, labels, slot=slot, teacher_logits=teacher)


@pytest.mark.parametrize("name", ROWS)
def test_a_distill_step_follows_the_oracle_and_graphs_and_groups_are_bitwise(name, monkeypatch):
    row = BY_NAME[name]
    cfg = row.config
    set_knobs(monkeypatch, row)
    kw = dict(DISTILL, input_slots=3)
    with trainer_for(cfg, use_graph=False, **kw) as (eager, params):
        p64 = {k: v.double() for k, v in params.items()}
        gen = torch.Generator().manual_seed(41)
        batches = [distill_batch(cfg, p64, gen) for _ in range(3)]
        ref = oracle_distill_step(cfg, p64, *batches[0])
        was = {k: v.detach().clone() for k, v in eager.p.items()}
        with CallLog() as log:
            loss = feed(eager, batches[0], 0, ref["max_grad_norm"])
        torch.cuda.synchronize()
        entry = "nnue_classifier_train_step_distill_bucketed" if cfg["K"] > 1 else "nnue_classifier_train_step_distill"
        ran = [n for _, n, _ in log.entries if n.startswith("nnue_classifier_train_step")]
        assert ran and set(ran) == {entry}, ran
        assert eager.mode.phases == row.modes["phases"]
        ratios = {}
        fails = compare_held(dict(held_by(eager, was), logits=eager.logits, loss=loss, norm=eager.grad_norm), ref, eager.B, eager.B, None,
                             f"{name} distill step", ratios)
        print("DISTILL_TRAINER", name, {k: round(v, 4) for k, v in ratios.items()})
        assert not fails, "; ".join(fails)
        assert set(ratios) >= {"logits", "loss", "norm", "grad", "parameters", "update", "momentum"}
        # ---- the same step and two more, then the three slots once more, as eager steps, graph steps and one step group
        losses, states = [loss.clone()], [snapshot(eager)]
        for s in (1, 2):
            losses.append(feed(eager, batches[s], s, ref["max_grad_norm"]).clone())
            states.append(snapshot(eager))
        with trainer_for(cfg, use_graph=True, **kw) as (single, _), trainer_for(cfg, use_graph=True, **kw) as (group, _):
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
            for s in (0, 1, 2):  # each slot kept its own teacher logits
                assert torch.equal(group.teacher_inputs[s].cpu(), batches[s][2]) and len(group.inputs[s]) == 2


def test_defaults_make_the_plain_calls_and_the_values_travel_with_the_state(monkeypatch):
    row = BY_NAME["A"]
    cfg = row.config
    set_knobs(monkeypatch, row)
    gen = torch.Generator().manual_seed(9)
    data = [(torch.rand(cfg["batch"], 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (cfg["batch"],), generator=gen).to(DEV))
            for _ in range(3)]
    teacher = torch.randn(cfg["batch"], cfg["classes"], generator=gen).to(DEV)
    # alpha == 0 with another temperature is the plain step as well: nothing is allocated, no call changes
    with trainer_for(cfg) as (a, _), trainer_for(cfg) as (b, _), trainer_for(cfg, distill_temperature=3.0) as (c, _):
        assert a.teacher_inputs is None and a.teacher is None and (a.distill_alpha, a.distill_temperature) == (0.0, 1.0)
        with CallLog() as log:
            for x, y in data:
                a.step(x, y)
        ran = {n for _, n, _ in log.entries if n.startswith("nnue_classifier_train_step")}
        assert ran == {"nnue_classifier_train_step"}, ran
        for x, y in data:
            b.step(x, y)
            c.step(x, y)
        torch.cuda.synchronize()
        assert same(snapshot(a), snapshot(b)) and same(snapshot(c), snapshot(a))
        with pytest.raises(ValueError, match="distill_alpha > 0"):
            a.step(*data[0], teacher_logits=teacher)
        old = {k: v for k, v in a.state_dict().items() if not k.startswith("distill")}
        assert a.state_dict()["distill_alpha"] == 0.0 and a.state_dict()["distill_temperature"] == 1.0
        b.load_state_dict(old)  # a state from before the keys existed: 0 and 1
        with trainer_for(cfg, **DISTILL) as (d, _), trainer_for(cfg, **DISTILL) as (e, _):
            with pytest.raises(ValueError, match="needs teacher_logits"):
                d.step(*data[0])
            with pytest.raises(ValueError, match="teacher_logits must be"):
                d.step(*data[0], teacher_logits=teacher[:, :5])
            d.step(*data[0], teacher_logits=teacher)
            sd = d.state_dict()
            assert (sd["distill_alpha"], sd["distill_temperature"]) == (ALPHA, T)
            e.load_state_dict(sd)
            e.model.load_state_dict(d.model.state_dict())
            before = snapshot(b)
            for state in (dict(sd, label_smoothing=0.0), dict(old, distill_alpha=ALPHA), dict(old, distill_temperature=T)):
                with pytest.raises(ValueError, match="distill_alpha"):
                    b.load_state_dict(state)
            assert same(snapshot(b), before)
            with pytest.raises(ValueError, match="distill_alpha"):
                d.load_state_dict(dict(old, label_smoothing=EPS))
            # the loaded twin and a rebuilt trainer go on as the original does
            la, lb = d.step(*data[1], teacher_logits=teacher), e.step(*data[1], teacher_logits=teacher)
            torch.cuda.synchronize()
            assert torch.equal(la, lb) and same(snapshot(d), snapshot(e))
            r = e.rebuilt("mfma")
            assert (r.distill_alpha, r.distill_temperature) == (ALPHA, T) and r.teacher_inputs is not None
            la, lb = d.step(*data[2], teacher_logits=teacher), r.step(*data[2], teacher_logits=teacher)
            torch.cuda.synchronize()
            assert torch.equal(la, lb) and same(snapshot(d), snapshot(r))


def small_model(seed=0):
    import nnue
    torch.manual_seed(seed)
    return nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).cuda()


def test_teacher_epoch_in_place_equals_copy_feeding():
    """tests/test_gpu_soft_trainer.py::test_mixing_epoch_in_place_equals_copy_feeding with a teacher, at its bars: a short last
    batch (9 of 64), the padded teacher rows behind labels of -1."""
    from nnue_hip.input_pipeline import GpuImageDataset, train_epoch
    from nnue_hip.trainer import NnueTrainer
    rng = np.random.RandomState(10)
    images, labels = rng.randint(0, 256, size=(64 * 5 + 9, 24, 24, 3), dtype=np.uint8), rng.randint(0, 10, size=64 * 5 + 9)
    teacher = small_model(seed=3).eval()
    calls = []

    def teach(x):
        calls.append(tuple(x.shape))
        return teacher(x)

    models, sums = [], []
    for mode in ("sequential", "in_place"):
        model = small_model()
        ds = GpuImageDataset(images, labels, augment="medium", out_hw=(32, 32), seed=5)
        tr = NnueTrainer(model, 64, ds.output_hw, lr=0.01, momentum=0.9, input_slots=2, **DISTILL)
        loader = ds.loader(64, shuffle=True, generator=torch.Generator().manual_seed(11))
        if mode == "sequential":
            losses = []
            for idx in loader.index_batches():
                x, y = ds.batch(idx)
                with torch.no_grad():
                    u = teacher(x)
                losses.append(float(tr.step(x, y, teacher_logits=u)))
            total, n = sum(losses), len(losses)
            assert all(np.isfinite(losses))
            with pytest.raises(ValueError, match="needs a teacher"):
                train_epoch(tr, loader)
        else:
            s, n = train_epoch(tr, loader, teacher=teach)
            total = float(s)
            assert calls == [(64, 3, 32, 32)] * 5 + [(9, 3, 32, 32)]
            assert bool(tr.teacher_inputs[0].any()) and bool(tr.teacher_inputs[1].any())
        assert n == 6 and np.isfinite(total) and ds.step == 6
        models.append(model)
        sums.append(total)
    assert abs(sums[0] - sums[1]) <= 1e-4 * abs(sums[0])
    for (k, p), (_, q) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert float((p - q).detach().abs().max()) <= 1e-5 * max(1.0, float(q.detach().abs().max())), k


# ------------------------------------------------------------------------------------------------- the training driver
def _config(tmp_path, epochs, distill=True):
    from nnue_hip import train_loop
    from test_train_loop import CONFIG_TEXT
    path = tmp_path / f"train_distill_{epochs}_{int(distill)}.py"
    path.write_text(textwrap.dedent(CONFIG_TEXT.format(opt="sgd", lr=0.02, epochs=epochs))
                    + (f"label_smoothing = {EPS}\ndistill_alpha = {ALPHA}\ndistill_temperature = {T}\n" if distill else ""))
    return train_loop.load_config(path)


def _train(cfg, ckpt_dir, teacher, **kw):
    from nnue_hip import train_loop
    from nnue_hip.input_pipeline import dataset_from_config
    g = torch.Generator().manual_seed(11)
    n = 6 * 16 + 7
    labels = torch.randint(0, 10, (n,), generator=g)
    images = (torch.randint(0, 160, (n, 32, 32, 3), generator=g) + labels.view(-1, 1, 1, 1) * 9).to(torch.uint8)
    train = dataset_from_config(cfg, images, labels, train=True, seed=3)
    val = dataset_from_config(cfg, images[:48], labels[:48], train=False)
    torch.manual_seed(0)
    model = train_loop.build_model(cfg, DEV)
    res = train_loop.run_training(cfg, train.loader(16, shuffle=True, generator=torch.Generator().manual_seed(21)), val.loader(16),
                                  model=model, checkpoint_dir=ckpt_dir, log=lambda s: None, teacher=teacher, **kw)
    return res, model, val


def test_run_training_with_a_teacher_and_a_resume(tmp_path):
    teacher = small_model(seed=7).eval()
    full, model, val = _train(_config(tmp_path, 2), tmp_path / "full", teacher, save_last=True)
    assert full.steps == 2 * 7 and len(full.history) == 2
    assert all(np.isfinite(row["train/epoch_loss"]) and np.isfinite(row["val/loss"]) for row in full.history)
    # val/loss is plain cross-entropy on the validation set: the mean of the per-batch means
    model.eval()
    with torch.no_grad():
        per_batch = [float(F.cross_entropy(model(x).double(), y)) for x, y in val.loader(16)]
    plain = sum(per_batch) / len(per_batch)
    assert abs(full.history[-1]["val/loss"] - plain) <= 1e-4 * max(1.0, abs(plain))
    last = torch.load(tmp_path / "full" / "last.ckpt", weights_only=True)
    assert last["run_state"]["trainer"]["distill_alpha"] == pytest.approx(ALPHA)
    assert last["run_state"]["trainer"]["distill_temperature"] == pytest.approx(T)
    # stop after epoch 1, resume: the bits of the uninterrupted run
    part, _, _ = _train(_config(tmp_path, 1), tmp_path / "resumed", teacher, save_last=True)
    assert part.history == full.history[:1]
    resumed, resumed_model, _ = _train(_config(tmp_path, 2), tmp_path / "resumed", teacher, save_last=True,
                                       resume_from=tmp_path / "resumed" / "last.ckpt")
    assert resumed.steps == full.steps and resumed.history == full.history
    for (k, v), (_, w) in zip(model.state_dict().items(), resumed_model.state_dict().items()):
        assert torch.equal(v, w), k
    # alpha 0 never calls a teacher; alpha > 0 without one is refused

    def never(x):
        raise AssertionError("the teacher was called with distill_alpha = 0")

    plain_run, _, _ = _train(_config(tmp_path, 1, distill=False), tmp_path / "plain", never)
    assert plain_run.steps == 7 and plain_run.history != full.history[:1]
    with pytest.raises(ValueError, match="needs a teacher"):
        _train(_config(tmp_path, 1), tmp_path / "none", None)


# ------------------------------------------------------------------------------------------------- two ranks
CFG = dict(tm.A, batch=12)
WORLD = 2


def _global_batch():
    """The global batch of the data-parallel row, clean of gate ties for the seed's parameters, and its teacher logits."""
    cfg = dict(CFG, batch=CFG["batch"] * WORLD)
    p64 = {k: v.detach().double() for k, v in tm.build_model(cfg).state_dict().items()}
    return distill_batch(cfg, p64, torch.Generator().manual_seed(51))


def _worker(rank: int, port: int, out_dir: str):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        for k in tm.KNOBS:
            os.environ.pop(k, None)
        images, labels, teacher = torch.load(Path(out_dir) / "batch.pt", weights_only=True)
        rows = slice(rank * CFG["batch"], (rank + 1) * CFG["batch"])
        with tm.trainer_for(CFG, **DISTILL) as (tr, _):
            assert tr.dp.world == WORLD and tr.teacher_inputs[0].shape == (CFG["batch"], CFG["classes"])
            was = {k: v.detach().cpu().clone() for k, v in tr.p.items()}
            loss = tr.step(images[rows].to(DEV), labels[rows].to(DEV), teacher_logits=teacher[rows].to(DEV))
            torch.cuda.synchronize()
            torch.save(dict(params={k: v.detach().cpu() for k, v in tr.p.items()}, was=was, logits=tr.logits.cpu(), loss=float(loss),
                            norm=float(tr.grad_norm), momentum={k: v.cpu() for k, v in tr.layout.views(tr.flat_momentum).items()}),
                       Path(out_dir) / f"rank_{rank}.pt")
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_two_ranks_equal_the_single_rank_step_on_the_global_batch(tmp_path, monkeypatch):
    import torch.multiprocessing as mp
    for k in tm.KNOBS:
        monkeypatch.delenv(k, raising=False)
    images, labels, teacher = batch = _global_batch()
    torch.save(batch, tmp_path / "batch.pt")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(port, str(tmp_path)), nprocs=WORLD, join=True)  # (a rank's failed assertion raises here)
    got = [torch.load(tmp_path / f"rank_{r}.pt", weights_only=True) for r in range(WORLD)]
    with trainer_for(dict(CFG, batch=CFG["batch"] * WORLD), **DISTILL) as (one, _):
        before = {k: v.detach().cpu().double() for k, v in one.p.items()}
        loss = one.step(images.to(DEV), labels.to(DEV), teacher_logits=teacher.to(DEV))
        torch.cuda.synchronize()
        ref = dict(before=before, after={k: v.detach().cpu().double() for k, v in one.p.items()}, norm=float(one.grad_norm),
                   state={k: v.cpu().double() for k, v in one.layout.views(one.flat_momentum).items()})
        sink = one.F - 1 if one.P > one.F else None
        logits, mean = one.logits.cpu().double(), float(loss)
    for r, held in enumerate(got):
        rows = slice(r * CFG["batch"], (r + 1) * CFG["batch"])
        ratios = {}
        fails = compare_held(dict(optimizer="sgd", sink=sink, params=held["params"], was=held["was"], momentum=held["momentum"],
                                  logits=held["logits"], norm=held["norm"]), dict(ref, logits=logits[rows]), CFG["batch"], CFG["batch"],
                             None, f"rank {r}", ratios)
        print("DISTILL_DP rank", r, {k: round(v, 4) for k, v in ratios.items()})
        assert not fails, "; ".join(fails)
        assert set(ratios) >= {"logits", "norm", "parameters", "update", "momentum"}
    assert abs(sum(h["loss"] for h in got) / WORLD - mean) <= 1e-4 * max(1.0, abs(mean))  # the ranks' local means average to the global one
    for k in got[0]["params"]:
        assert torch.equal(got[0]["params"][k], got[1]["params"][k]), f"the ranks' {k} differ"
