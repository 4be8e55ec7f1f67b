"""The weight clip on the GPU (include/nnue_hip.h, "weight clip"; NnueTrainer(weight_clip=), nnue_hip.optim groups): a trainer
with ``weight_clip = c`` is, after every step and bit for bit, the plain trainer on which the four clipped tensors were
``clamp_``ed after that step -- in every step mode, in the table forms (the fused update + next-forward pass among them), with
the option off, on the module path, across a checkpoint, and up to the exported file.  tests/weight_clip_cases.py makes the clamp
bite and asserts that it did.  ``-m gpu``."""
import copy

import gc

import pytest
import torch

import nnue
import trainer_modes as tm
import weight_clip_cases as wc
from test_gpu_update_sequence import EXPECTED, OPTIMIZERS, _logged, _trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _collect_trainers():
    """A failed test's trainers live on in its traceback; their captured graphs must be destroyed here, between tests, and not by
    a garbage collection that happens to run inside the next test's graph capture (the runtime refuses that and aborts)."""
    yield
    gc.collect()
DEV = "cuda"

SIBLING = {name: name + "_clip" for name in (
    "nnue_sgd_step", "nnue_adam_step", "nnue_adam_step_ext", "nnue_ftm_backward_weight_update", "nnue_ftm_backward_weight_update_forward",
    "nnue_ftm_backward_weight_update_adam", "nnue_ftm_backward_weight_update_forward_adam")}


# ---------------------------------------------------------------------------------------------- 1. every step mode
# rows where the reference side's clamp_ stays below the bar from step 2 on at every learning rate and seed tried
# (tests/weight_clip_cases.py has the figures): several layer stacks, clipped activations, a last layer of 15 weights
RESPREAD = {"A_k4_clip", "A_k4_adam", "A_l2_7", "g5_bits_k3", "g5_list", "A_forced_list_k4", "g16_patches_k4", "t8192_ftu_k4"}


@pytest.mark.parametrize("name,c", [(n, 1.0) for n in tm.ROW_NAMES] + [("A", 0.25)])
def test_every_step_mode_clamps_as_clamp_does(monkeypatch, name, c):
    """Three single steps (first-step plan, steady plan, graph replay) of each row of trainer_modes.ROWS; row A at a second bound."""
    row = tm.BY_NAME[name]
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    batches = wc.fresh_batches(3, cfg["batch"], cfg["image"], cfg["classes"])
    with tm.trainer_for(cfg, weight_clip=c) as (clipped, _), tm.trainer_for(cfg) as (plain, _):
        assert clipped.mode == plain.mode  # (the option is no input of the mode; the row's mode is held by test_gpu_trainer_modes.py)
        feed = [lambda tr, b=b: tr.step(b[0].to(DEV), b[1].to(DEV)) for b in batches]
        wc.pair_steps(clipped, plain, c, feed, f"{name} c={c}", respread=name in RESPREAD)


# ---------------------------------------------------------------------------------------------- 2. the table forms
TABLE_CASES = [(o, f) for o in sorted(OPTIMIZERS) for f in ("1", "0")]


@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_table_forms_single_steps(monkeypatch, optimizer, fuse_next):
    clipped = _trainer(monkeypatch, fuse_next, weight_clip=1.0, **OPTIMIZERS[optimizer])
    plain = _trainer(monkeypatch, fuse_next, **OPTIMIZERS[optimizer])
    assert clipped.fuse_table_update and plain.fuse_table_update
    wc.pair_steps(clipped, plain, 1.0, [lambda tr, s=s: tr.step(slot=s) for s in (0, 1, 2)], f"table {optimizer} next={fuse_next}")


@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_a_step_group_is_three_single_steps(monkeypatch, optimizer, fuse_next):
    """step_many((0, 1, 2)) after two recording steps against five single steps: with the next forward fused, steps 2 and 3 of
    the group run on the FeatureTransformer output the previous update's pass formed -- from the clamped tiles, or this fails."""
    group = _trainer(monkeypatch, fuse_next, weight_clip=1.0, **OPTIMIZERS[optimizer])
    single = _trainer(monkeypatch, fuse_next, weight_clip=1.0, **OPTIMIZERS[optimizer])
    for tr in (group, single):
        wc.rescale(tr.p, 1.0)
        tr.max_grad_norm = wc.GRAD_NORM
        tr.step(slot=0)
        tr.step(slot=1)
    ring = group.step_many((0, 1, 2)).clone()
    losses = torch.stack([single.step(slot=s).clone() for s in (0, 1, 2)])
    torch.cuda.synchronize()
    assert group.steps_done == single.steps_done == 5
    assert torch.equal(ring, losses), (ring, losses)
    for a, b in zip(wc.state_of(group), wc.state_of(single)):
        assert torch.equal(a, b)
    # the clamp was at work in those steps: nothing lies beyond the bound, and the table -- the operand of the fused forward -- sits
    # on it in a good part of its elements
    assert all(float(group.p[k].abs().max()) <= 1.0 for k in wc.CLIPPED)
    assert float((group.p["input.weight"].abs() == 1.0).float().mean()) >= wc.BITE


@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_table_forms_launch_the_clamped_siblings(monkeypatch, optimizer, fuse_next):
    tr = _trainer(monkeypatch, fuse_next, weight_clip=1.0, **OPTIMIZERS[optimizer])
    single, group = _logged(monkeypatch, tr)
    want_single, want_group = EXPECTED[(optimizer, fuse_next)]
    assert single == [SIBLING.get(n, n) for n in want_single]
    assert group == [SIBLING.get(n, n) for n in want_group]
    assert any(n.endswith("_clip") for n in single) and len(single) == len(want_single) and len(group) == len(want_group)


# ---------------------------------------------------------------------------------------------- 3. off is plain
@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_off_is_plain(monkeypatch, optimizer, fuse_next):
    off = _trainer(monkeypatch, fuse_next, weight_clip=0.0, **OPTIMIZERS[optimizer])
    without = _trainer(monkeypatch, fuse_next, **OPTIMIZERS[optimizer])
    for tr in (off, without):
        wc.rescale(tr.p, 1.0)
    for s in (0, 1, 2):
        a, b = off.step(slot=s).clone(), without.step(slot=s).clone()
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    for a, b in zip(wc.state_of(off), wc.state_of(without)):
        assert torch.equal(a, b)
    assert float(off.p["input.weight"].abs().max()) > 1.0  # (nothing was clamped)
    fresh = _trainer(monkeypatch, fuse_next, weight_clip=0.0, **OPTIMIZERS[optimizer])
    assert _logged(monkeypatch, fresh) == tuple(list(x) for x in EXPECTED[(optimizer, fuse_next)])


# ---------------------------------------------------------------------------------------------- 5. the module path
def _module_run(opt_cls, groups_of, c_after, steps=3, **opt_kw):
    """`steps` steps of a small nnue.NNUE through backward() and the drop-in optimizer; c_after(model): what the caller does
    after each step (the reference side's clamp_).  Returns (parameters, optimizer state tensors, losses)."""
    from nnue_hip import optim
    torch.manual_seed(3)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(DEV)
    named = dict(model.named_parameters())
    wc.rescale({k: v.data for k, v in named.items()}, 1.0)
    opt = getattr(optim, opt_cls)(groups_of(named), max_grad_norm=wc.GRAD_NORM, **opt_kw)
    gen = torch.Generator().manual_seed(4)
    losses = []
    for i in range(steps):
        if i > 0:  # weight_clip_cases' respread, on both sides alike: at this batch of 16 the clamp would bite 1-2 % of the table
            with torch.no_grad():
                for k in wc.CLIPPED:
                    named[k].mul_(2.0)
        images, labels = torch.randn(16, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (16,), generator=gen).to(DEV)
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(images), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        c_after(named)
        losses.append(loss.detach().clone())
    state = [t.clone() for p in model.parameters() for k, t in sorted(opt.state.get(p, {}).items()) if torch.is_tensor(t) and t.is_cuda]
    return {k: v.detach().clone() for k, v in named.items()}, state, losses


@pytest.mark.parametrize("opt_cls,kw", (("SGD", dict(lr=0.05, momentum=0.9, weight_decay=2e-4)), ("Adam", dict(lr=1e-2, weight_decay=2e-4))))
def test_module_path_groups(opt_cls, kw):
    four = lambda named, c: [dict(params=[named[k] for k in wc.CLIPPED], weight_clip=c),  # noqa: E731
                             dict(params=[v for k, v in named.items() if k not in wc.CLIPPED and v.requires_grad and k != "nnue2score"])]
    shares = []
    got = _module_run(opt_cls, lambda n: four(n, 1.0), lambda n: None, **kw)
    ref = _module_run(opt_cls, lambda n: four(n, 0.0), lambda n: shares.append(wc.clamp_and_count({k: v.data for k, v in n.items()}, 1.0)), **kw)
    print(shares)
    assert all(min(s.values()) >= wc.BITE for s in shares), shares
    for k in got[0]:
        assert torch.equal(got[0][k], ref[0][k]), k
    assert len(got[1]) == len(ref[1]) > 0 and all(torch.equal(a, b) for a, b in zip(got[1], ref[1]))
    assert all(torch.equal(a, b) for a, b in zip(got[2], ref[2]))
    assert float(got[0]["conv.weight"].abs().max()) > 1.0  # its group does not clamp
    # one group with the option on every parameter clamps the conv weights too: the option means its group, nothing else
    every = lambda named, c: [dict(params=[v for k, v in named.items() if k != "nnue2score"], weight_clip=c)]  # noqa: E731

    def clamp_all(named):
        with torch.no_grad():
            for k, v in named.items():
                if k != "nnue2score":
                    v.clamp_(-1.0, 1.0)
    got = _module_run(opt_cls, lambda n: every(n, 1.0), lambda n: None, **kw)
    ref = _module_run(opt_cls, lambda n: every(n, 0.0), clamp_all, **kw)
    assert float(got[0]["conv.weight"].abs().max()) == 1.0
    for k in got[0]:
        assert torch.equal(got[0][k], ref[0][k]), k


# ---------------------------------------------------------------------------------------------- 6. the point of it
# measured at row A, ten steps from the default init with max_grad_norm 1: at 0.5 and 2.0 the table never reaches the bound; at
# 5.0 all four tensors do (shares on the bound 0.0002 / 0.031 / 0.19 / 0.21) and the plain run ends with as many beyond it
POINT_LR = 5.0


def _train_ten(weight_clip):
    from nnue_hip.trainer import NnueTrainer
    cfg = tm.BY_NAME["A"].config
    model = tm.build_model(cfg).to(DEV)  # default init, not rescaled
    tr = NnueTrainer(model, cfg["batch"], (cfg["image"], cfg["image"]), lr=POINT_LR, momentum=cfg["momentum"], weight_decay=2e-4,
                     max_grad_norm=1.0, weight_clip=weight_clip)
    for images, labels in wc.fresh_batches(10, cfg["batch"], cfg["image"], cfg["classes"], seed=21):
        tr.step(images.to(DEV), labels.to(DEV))
    torch.cuda.synchronize()
    return model


def test_the_exported_network_is_the_trained_one(monkeypatch, tmp_path):
    import serialize
    from nnue_hip.engine import EngineModel
    tm.set_knobs(monkeypatch, tm.BY_NAME["A"])
    model = _train_ten(1.0)
    at_bound = {k: float((dict(model.named_parameters())[k].abs() == 1.0).float().mean()) for k in wc.CLIPPED}
    print(f"share of each tensor on the bound after ten steps at lr {POINT_LR}: {at_bound}")
    assert min(at_bound.values()) > 0.0, "a tensor never reached the bound: raise POINT_LR"
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    twin = copy.deepcopy(model)
    serialize.serialize_model(model, tmp_path / "trained.nnue")
    after = model.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    twin._clip_weights()
    serialize.serialize_model(twin, tmp_path / "clipped.nnue")
    assert (tmp_path / "trained.nnue").read_bytes() == (tmp_path / "clipped.nnue").read_bytes()
    live, loaded = EngineModel.from_model(model), EngineModel.load(tmp_path / "trained.nnue", device=DEV)
    assert live.tensors.keys() == loaded.tensors.keys()
    for k in live.tensors:
        assert torch.equal(live.tensors[k].cpu(), loaded.tensors[k].cpu()), k
    # without the option the same run leaves weights outside the range, and serialising changes the live model
    plain = _train_ten(0.0)
    before = {k: v.detach().clone() for k, v in plain.state_dict().items()}
    serialize.serialize_model(plain, tmp_path / "plain.nnue")
    after = plain.state_dict()
    assert not all(torch.equal(before[k], after[k]) for k in before), "the plain run stayed inside the range: raise POINT_LR"


# ---------------------------------------------------------------------------------------------- 7. resume
@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
def test_resume_keeps_the_bound(monkeypatch, optimizer):
    row = tm.BY_NAME["A_adam" if optimizer == "adam" else "A"]
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    batches = [(i.to(DEV), l.to(DEV)) for i, l in wc.fresh_batches(3, cfg["batch"], cfg["image"], cfg["classes"])]
    with tm.trainer_for(cfg, weight_clip=1.0) as (whole, _), tm.trainer_for(cfg, weight_clip=1.0) as (resumed, _), \
            tm.trainer_for(cfg, weight_clip=0.5) as (other, _), tm.trainer_for(cfg) as (none, _):
        wc.rescale(whole.p, 1.0)
        for b in batches[:2]:
            whole.step(*b)
        torch.cuda.synchronize()
        sd = copy.deepcopy(whole.state_dict())
        assert sd["weight_clip"] == 1.0
        params = whole.flat_params.clone()
        for tr in (other, none):
            held = wc.state_of(tr)
            with pytest.raises(ValueError, match="weight_clip"):
                tr.load_state_dict(sd)
            assert tr.steps_done == 0 and all(torch.equal(a, b) for a, b in zip(held, wc.state_of(tr)))
        with pytest.raises(ValueError, match="weight_clip"):  # a state from before the key existed counts as 0
            whole.load_state_dict({k: v for k, v in sd.items() if k != "weight_clip"})
        resumed.flat_params.copy_(params)
        resumed.load_state_dict(sd)
        a, b = whole.step(*batches[2]).clone(), resumed.step(*batches[2]).clone()
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        for x, y in zip(wc.state_of(whole), wc.state_of(resumed)):
            assert torch.equal(x, y)
        assert float(whole.p["input.weight"].abs().max()) <= 1.0
        # the rebuilt trainer (the train loop's density switch) carries the bound over
        assert whole.rebuilt("mfma").weight_clip == 1.0
