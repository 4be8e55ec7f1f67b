"""The fused trainer (flat buffers, recorded kernel plan, hipGraph replay, fused clip+SGD) against the
reference's SGD trajectory (golden step fixtures) and against the drop-in autograd path.  ``-m gpu``."""
import json

import pytest
import torch
import torch.nn.functional as F

import nnue
from conftest import assert_close_grad, load_npz
from nnue_hip.trainer import FlatLayout, NnueTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build(cfg, state):
    m = nnue.NNUE(nnue.GridFeatureSet(cfg["grid"], cfg["fps"]), cfg["l1"], cfg["l2"], cfg["l3"],
                  num_classes=cfg["classes"], input_size=cfg["input_size"])
    m.load_state_dict(state)
    return m.to(DEV)


@pytest.mark.parametrize("name", ("c1arch", "tiny96"))
@pytest.mark.parametrize("use_graph", (False, True))
def test_trainer_follows_reference_trajectory(name, use_graph):
    z = load_npz(f"step_{name}.npz")
    cfg = json.loads(str(z["cfg"]))
    state0 = {k[7:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state0/")}
    model = build(cfg, state0)
    images0 = torch.from_numpy(z["images0"])
    tr = NnueTrainer(model, images0.shape[0], tuple(images0.shape[2:]), lr=cfg["lr"], momentum=cfg["momentum"],
                     weight_decay=cfg["weight_decay"], max_grad_norm=cfg["max_grad_norm"], use_graph=use_graph)
    for s in range(3):
        loss = tr.step(torch.from_numpy(z[f"images{s}"]).to(DEV), torch.from_numpy(z[f"labels{s}"]).to(DEV).long())
        assert abs(float(loss) - float(z[f"loss{s}"])) <= 2e-4 * max(1.0, abs(float(z[f"loss{s}"])))
        assert abs(float(tr.grad_norm) - float(z[f"gradnorm{s}"])) <= 2e-4 * float(z[f"gradnorm{s}"])
        sd = model.state_dict()  # parameters are views of the flat buffer
        for k, v in sd.items():
            assert_close_grad(v, torch.from_numpy(z[f"state{s + 1}/{k}"]), f"step {s} {k}", rtol=2e-4)
    assert float(model.nnue2score) == 600.0


@pytest.mark.parametrize("path", ("bits", "list"))
def test_gather_paths_follow_the_trajectory_when_replayed(monkeypatch, path):
    """The gather kernel families under a replayed hipGraph (NNUE_FT_PATH): regression for zero fills that were
    memset nodes -- a memset captured ahead of a kernel scattering into the same buffer was not ordered before it."""
    monkeypatch.setenv("NNUE_FT_PATH", path)
    test_trainer_follows_reference_trajectory("c1arch", True)
    test_trainer_follows_reference_trajectory("tiny96", True)


def test_trainer_gradients_equal_autograd_path():
    torch.manual_seed(0)
    cfg = dict(grid=10, fps=8, l1=256, l2=32, l3=16, classes=10, input_size=32)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(DEV)
    twin = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(DEV)
    twin.load_state_dict(model.state_dict())
    images = torch.randn(64, 3, 32, 32, device=DEV)
    labels = torch.randint(0, 10, (64,), device=DEV)
    tr = NnueTrainer(model, 64, (32, 32), lr=0.0, use_graph=True)  # lr 0: parameters stay put, grads are exposed
    loss = tr.step(images, labels)
    ref_loss = F.cross_entropy(twin(images), labels)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
    for (k, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        if k != "nnue2score":
            assert_close_grad(p.grad, q.grad, k, rtol=1e-5)  # same kernels; d_logits comes from torch's CE there
    # replay is bitwise reproducible
    g1 = tr.flat_grads.clone()
    tr.step(images, labels)
    assert torch.equal(g1, tr.flat_grads)
    assert_close_grad(tr.evaluate(images), twin(images), "evaluate")


def test_flat_layout_alignment_and_roundtrip():
    model = nnue.NNUE(nnue.GridFeatureSet(5, 3), 24, 7, 5, num_classes=3, input_size=40)
    lay = FlatLayout.of(model)
    assert lay.names[0] == "visual_threshold" and "nnue2score" not in lay.names
    assert all(o % 4 == 0 for o in lay.offsets) and lay.count % 4 == 0
    state = {k: p.detach() for k, p in model.named_parameters() if k != "nnue2score"}
    flat = lay.pack(state)
    for k, v in lay.views(flat).items():
        assert torch.equal(v, state[k])


def test_c4_shaped_step_list_and_lds_paths_agree(monkeypatch):
    """One full training step at BASELINE config 4's architecture (224x224, 32x32x64 grid, 65 536 -> 1024/128/32 ->
    1000) with both FeatureTransformer kernel families: same loss, same gradients."""
    cfgs = {}
    for path in ("list", "bits"):
        monkeypatch.setenv("NNUE_FT_PATH", path)
        torch.manual_seed(0)
        model = nnue.NNUE(nnue.GridFeatureSet(32, 64), 1024, 128, 32, num_classes=1000, input_size=224).to(DEV)
        tr = NnueTrainer(model, 8, (224, 224), lr=0.0, use_graph=False)
        assert tr.use_bits == (path == "bits")
        gen = torch.Generator().manual_seed(1)
        images, labels = torch.randn(8, 3, 224, 224, generator=gen), torch.randint(0, 1000, (8,), generator=gen)
        loss = tr.step(images.to(DEV), labels.to(DEV))
        cfgs[path] = (float(loss), tr.flat_grads.clone(), tr.active_stats())
        del tr, model
    assert abs(cfgs["list"][0] - cfgs["bits"][0]) <= 1e-5 * max(1.0, abs(cfgs["list"][0]))
    assert cfgs["list"][2] == cfgs["bits"][2] and cfgs["list"][2][0] > 20000  # ~28k active features per image
    assert_close_grad(cfgs["bits"][1], cfgs["list"][1], "flat gradient")


def thresholds_for_density(model, images, density):
    """Per-channel thresholds that leave about `density` of the conv outputs above them (SURVEY 8d's sweep)."""
    with torch.no_grad():
        conv = F.conv2d(images, model.conv.weight.detach().to(images.device), stride=model.conv.stride, padding=1)
        per_channel = conv.transpose(0, 1).flatten(1)
        return torch.quantile(per_channel, 1.0 - density, dim=1)


@pytest.mark.parametrize("path", ("mfma", "bits", "list"))
@pytest.mark.parametrize("density", (0.01, 0.05, 0.25, 0.9))
def test_density_sweep_step_against_oracle(monkeypatch, density, path):
    """Whole-step gradients at about 1 %, 5 %, 25 % and 90 % active features (the sweep SURVEY 8d asks for, after the
    reference's tests/test_model.py:570-576), the shipped product form and both gather families, against the CPU oracle."""
    import nnue_oracle as orc
    monkeypatch.setenv("NNUE_FT_PATH", path)
    torch.manual_seed(2)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10)
    gen = torch.Generator().manual_seed(3)
    images, labels = torch.randn(48, 3, 32, 32, generator=gen), torch.randint(0, 10, (48,), generator=gen)
    with torch.no_grad():
        model.visual_threshold.copy_(thresholds_for_density(model, images, density))
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    tr = NnueTrainer(model, 48, (32, 32), lr=0.0, use_graph=False)
    assert tr.ft_path == path
    loss = tr.step(images.to(DEV), labels.to(DEV))
    _, ref_loss, ref_grads, keep = orc.loss_and_grads_explicit(params, images, labels, 3)
    n_mean, n_max = tr.active_stats()
    assert n_max == int(keep["n"].max()) and abs(n_mean - float(keep["n"].float().mean())) < 1e-3
    assert abs(n_mean / 968 - density) < 0.3 * density + 0.01  # the sweep point is what it says
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss)))
    grads = tr.layout.views(tr.flat_grads)
    for k, ref in ref_grads.items():
        assert_close_grad(grads[k], ref, f"{k} density={density}")


def test_first_step_on_another_slot_leaves_slot_zero_alone_and_lr_changes_take_effect():
    """recording the plan on the slot of the first step (not on a copy into slot 0); a changed learning rate
    re-records the update plan and the graphs built from it."""
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(DEV)
    twin = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(DEV)
    twin.load_state_dict(model.state_dict())
    gen = torch.Generator().manual_seed(4)
    data = [(torch.randn(32, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (32,), generator=gen).to(DEV)) for _ in range(3)]
    tr = NnueTrainer(model, 32, (32, 32), lr=0.05, momentum=0.9, input_slots=3, use_graph=True)
    for (im, lb), (ti, tl) in zip(data, tr.inputs):
        ti.copy_(im)
        tl.copy_(lb)
    tr.step(slot=2)  # first step ever, not on slot 0
    assert torch.equal(tr.inputs[0][0], data[0][0]) and torch.equal(tr.inputs[0][1], data[0][1])
    tr.step(slot=0)
    tr.step(slot=1)
    tr.lr = 0.5  # same as set_lr(0.5)
    tr.step(slot=2)
    tr.step(slot=0)
    ref = NnueTrainer(twin, 32, (32, 32), lr=0.05, momentum=0.9, use_graph=False)
    for i, slot in enumerate((2, 0, 1, 2, 0)):
        if i == 3:
            ref.set_lr(0.5)
        ref.step(*data[slot])
    assert_close_grad(tr.flat_params, ref.flat_params, "parameters after an lr change", rtol=1e-6)
    assert_close_grad(tr.evaluate(data[1][0]), ref.evaluate(data[1][0]), "evaluate after a plan recorded on slot 2", rtol=1e-6)


@pytest.mark.parametrize("shape", ("small", "buckets", "bigtable"))
def test_step_many_is_the_same_steps_in_one_graph(shape, monkeypatch):
    """step_many((s0, s1, ...)) replays the kernels of step(slot=s0), step(slot=s1), ... as one hipGraph: bitwise the same
    parameters, momentum and per-step losses; a learning-rate change keeps the captured graph (device scalar), a change of
    another hyper-parameter drops it.  "bigtable": a table the forward walks as a split-K product -- inside the group the
    table update of a step also forms the next step's FeatureTransformer forward (one pass over the table, two alternating
    maps), still bitwise the single steps."""
    kw = dict(num_ls_buckets=4, clip_activations=1.0) if shape == "buckets" else {}
    grid, hw, l1 = (nnue.GridFeatureSet(10, 8), 32, 256) if shape != "bigtable" else (nnue.GridFeatureSet(16, 32), 64, 256)
    if shape == "bigtable":
        monkeypatch.setenv("NNUE_FUSE_TABLE_UPDATE", "1")  # (auto: tables of 32 MB or more; this one has 8 MB)
        monkeypatch.setenv("NNUE_FUSE_NEXT_FORWARD", "1")
        kw = dict(input_size=64)
    torch.manual_seed(0)
    model = nnue.NNUE(grid, l1, 32, 16, num_classes=10, **kw).to(DEV)
    twin = nnue.NNUE(grid, l1, 32, 16, num_classes=10, **kw).to(DEV)
    twin.load_state_dict(model.state_dict())
    gen = torch.Generator().manual_seed(5)
    data = [(torch.randn(64, 3, hw, hw, generator=gen).to(DEV), torch.randint(0, 10, (64,), generator=gen).to(DEV)) for _ in range(3)]
    opt = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0, input_slots=3, use_graph=True)
    tr = NnueTrainer(model, 64, (hw, hw), **opt)
    if shape == "bigtable":
        import os
        if not tr.fuse_next_forward and os.environ.get("NNUE_FTM_BF16") == "0":
            pytest.skip("a developer knob took the forward off the bf16-split 64-deep tiles the fused pass is built on")
        assert tr.fuse_table_update and tr.fuse_next_forward
        monkeypatch.setenv("NNUE_FUSE_NEXT_FORWARD", "0")
    ref = NnueTrainer(twin, 64, (hw, hw), **opt)
    assert not ref.fuse_next_forward
    for t in (tr, ref):
        for (im, lb), (ti, tl) in zip(data, t.inputs):
            ti.copy_(im)
            tl.copy_(lb)
    order = (0, 1, 2, 1, 0)
    first = tr.step_many(order[:2])  # before anything is recorded: falls back to single steps
    want = [ref.step(slot=s).clone() for s in order[:2]]
    assert torch.equal(first, torch.stack(want))
    for rep in range(2):
        got = tr.step_many(order).clone()
        want = torch.stack([ref.step(slot=s).clone() for s in order])
        assert torch.equal(got, want), (rep, got, want)
    assert (order, "many") in tr._g_local and tr.steps_done == ref.steps_done == 12
    tr.lr = ref.lr = 0.2
    assert (order, "many") in tr._g_local  # the rate is read from a device scalar: nothing is re-recorded
    got = tr.step_many(order).clone()
    want = torch.stack([ref.step(slot=s).clone() for s in order])
    assert torch.equal(got, want)
    tr.weight_decay = ref.weight_decay = 3e-4  # a constant of the recorded update plan
    assert (order, "many") not in tr._g_local
    got = tr.step_many(order).clone()
    want = torch.stack([ref.step(slot=s).clone() for s in order])
    assert torch.equal(got, want)
    assert torch.equal(tr.flat_params, ref.flat_params)
    assert torch.equal(tr.flat_momentum, ref.flat_momentum)
    if shape == "bigtable":  # an even-length group ends on the second map; single steps and the statistics follow
        got = tr.step_many(order[:4]).clone()
        want = torch.stack([ref.step(slot=s).clone() for s in order[:4]])
        assert torch.equal(got, want) and tr._last_alt
        assert tr.active_stats() == ref.active_stats()
        assert torch.equal(tr.step(slot=2), ref.step(slot=2)) and torch.equal(tr.flat_params, ref.flat_params)
        timers = {"nnue_ftm_backward_weight_update_forward": [], "nnue_ftm_forward": []}
        got = tr.step_many(order, timers=timers).clone()  # the same launches eagerly, with events
        want = torch.stack([ref.step(slot=s).clone() for s in order])
        assert torch.equal(got, want) and torch.equal(tr.flat_params, ref.flat_params)
        assert len(timers["nnue_ftm_backward_weight_update_forward"]) == len(order) - 1 and len(timers["nnue_ftm_forward"]) == 1
    with pytest.raises(ValueError):
        tr.step_many((0, 3))


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
def test_learning_rate_schedule_without_recapture(optimizer):
    """A per-step learning-rate schedule (``trainer.lr = x`` before every step): the rate is a device scalar the optimizer
    kernels read, so the recorded plans and the captured graphs -- single steps and a step group -- stay as they are, and
    the trajectory equals the oracle's with the same schedule (train.py:457-471's optimizers with a scheduler on top)."""
    import nnue_oracle as orc
    z = load_npz("step_c1arch.npz")
    cfg = opt = json.loads(str(z["cfg"]))
    params = {k[7:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state0/")}
    images = [torch.from_numpy(z[f"images{s % 3}"]) for s in range(6)]
    labels = [torch.from_numpy(z[f"labels{s % 3}"]).long() for s in range(6)]
    lrs = [opt["lr"], opt["lr"] * 0.5, opt["lr"] * 2.0, opt["lr"] * 0.25, opt["lr"] * 1.5, opt["lr"] * 0.1]
    model = build(cfg, params)
    tr = NnueTrainer(model, images[0].shape[0], tuple(images[0].shape[2:]), lr=lrs[0], momentum=opt["momentum"],
                     weight_decay=opt["weight_decay"], max_grad_norm=opt["max_grad_norm"], use_graph=True, input_slots=2,
                     optimizer=optimizer)
    ref = {k: v.clone() for k, v in params.items()}
    state = {}
    graphs_after_warmup = None
    for s in range(4):  # single steps: plan, graphs, then replays with a new rate each time
        tr.lr = lrs[s]
        assert tr.lr == lrs[s] and float(tr.lr_dev) == pytest.approx(lrs[s])
        tr.step(images[s].to(DEV), labels[s].to(DEV), slot=s % 2)
        _, _, grads, _ = orc.loss_and_grads_explicit(ref, images[s], labels[s], cfg["stride"])
        if optimizer == "sgd":
            orc.sgd_step(ref, grads, state, lrs[s], opt["momentum"], opt["weight_decay"], opt["max_grad_norm"])
        else:
            orc.adam_step(ref, grads, state, lrs[s], weight_decay=opt["weight_decay"], max_grad_norm=opt["max_grad_norm"])
        if s == 2:
            graphs_after_warmup = set(tr._g_local)
    assert set(tr._g_local) == graphs_after_warmup, "changing the learning rate must not drop or add graphs"
    # a step group replayed twice with two different rates: the same graph object both times
    for s in (4, 5):
        tr.inputs[0][0].copy_(images[s]); tr.inputs[0][1].copy_(labels[s])
        tr.lr = lrs[s]
        tr.step_many((0,))
        _, _, grads, _ = orc.loss_and_grads_explicit(ref, images[s], labels[s], cfg["stride"])
        if optimizer == "sgd":
            orc.sgd_step(ref, grads, state, lrs[s], opt["momentum"], opt["weight_decay"], opt["max_grad_norm"])
        else:
            orc.adam_step(ref, grads, state, lrs[s], weight_decay=opt["weight_decay"], max_grad_norm=opt["max_grad_norm"])
    assert sum(1 for k in tr._g_local if k[1] == "many") == 1
    torch.cuda.synchronize()
    for k in orc.TRAINABLE_KEYS:
        assert_close_grad(tr.p[k], ref[k], f"{optimizer} {k} after six steps of a schedule", rtol=5e-4)
