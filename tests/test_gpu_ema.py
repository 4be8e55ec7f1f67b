"""The weight average on the GPU (include/nnue_hip.h, "weight average"; NnueTrainer(ema_decay=, ema_warmup=), nnue_hip.optim
groups): the stand-alone pass against float64, and a trainer with ``ema_decay`` held -- after every step and bit for bit -- to
the plain trainer on parameters, optimizer state and losses, and on ``flat_ema`` to the stand-alone pass applied to the previous
average and the plain trainer's new parameters: in every step mode, in the table forms, with the option off, under a warm-up,
through ``ema_weights()``, across a checkpoint and on the module path.  tests/ema_cases.py has the driver.  ``-m gpu``."""
import copy
import gc

import pytest
import torch

import ema_cases as ec
import nnue
import trainer_modes as tm
import weight_clip_cases as wc
from test_gpu_update_sequence import EXPECTED, OPTIMIZERS, _logged, _trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _collect_trainers():
    """A failed test's trainers live on in its traceback; their captured graphs must be destroyed here, between tests, and not by
    a garbage collection that happens to run inside the next test's graph capture (the runtime refuses that and aborts)."""
    yield
    gc.collect()


SIBLING = {name: name + "_ema" for name in (
    "nnue_sgd_step", "nnue_adam_step", "nnue_adam_step_ext", "nnue_ftm_backward_weight_update", "nnue_ftm_backward_weight_update_forward",
    "nnue_ftm_backward_weight_update_adam", "nnue_ftm_backward_weight_update_forward_adam")}


# ---------------------------------------------------------------------------------------------- 1. the stand-alone kernel
COUNTS = (1, 3, 4, 5, 1023, 4099)
TINY = 2.0 ** -126  # the smallest normal float32


def _inputs(count: int, seed: int):
    """(e, w): normal, denormal, +-0 and 1e30-sized values.  The bound below is two RELATIVE roundings, which float32 gives only
    where a result is normal: a denormal is therefore paired with a normal value (then the bound, 3 * 2^-24 * max >= 3 * 2^-150,
    also covers two absolute roundings of 2^-150 in the denormal range); two denormals, or a denormal and a zero, cannot meet a
    relative bound in float32 whatever the kernel does (their exact result lies between two denormals 2^-149 apart)."""
    gen = torch.Generator().manual_seed(seed)
    e, w = torch.randn(count, generator=gen), torch.randn(count, generator=gen)
    kind = torch.randint(0, 8, (count,), generator=gen)
    sign = torch.where(torch.rand(count, generator=gen) < 0.5, -1.0, 1.0)
    denormal = sign * torch.rand(count, generator=gen) * TINY * 0.5
    e = torch.where(kind == 1, denormal, e)          # a denormal average, a normal weight
    w = torch.where(kind == 2, denormal, w)          # ... and the other way round
    e = torch.where(kind == 3, 0.0 * sign, e)        # +-0
    w = torch.where(kind == 4, 0.0 * sign, w)
    e = torch.where(kind == 5, 1e30 * sign * (1.0 + torch.rand(count, generator=gen)), e)
    w = torch.where(kind == 6, -1e30 * sign * (1.0 + torch.rand(count, generator=gen)), w)
    both = kind == 7                                 # both 1e30-sized, opposite signs: the difference stays finite
    e, w = torch.where(both, 1e30 * sign, e), torch.where(both, -1.5e30 * sign, w)
    return e.to(torch.float32), w.to(torch.float32)


def _check(got, e, w, omd32, what):
    ref = e.double() + float(omd32) * (w.double() - e.double())
    err = (got.double() - ref).abs()
    bound = 3.0 * 2.0 ** -24 * torch.maximum(w.double().abs(), e.double().abs())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst |delta| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements beyond 3 * 2^-24 * max(|w|, |e|), worst ratio {worst}"


@pytest.mark.parametrize("count", COUNTS)
def test_the_stand_alone_pass_against_float64(count):
    from nnue_hip import lib
    for rate in (1e-3, 1.0):
        omd32 = torch.tensor(rate, dtype=torch.float32)
        for offset in (0, 1):  # 16-byte aligned buffers (the float4 form and its tail) and 4-byte-misaligned slices (the scalar form)
            for through_dev in (False, True):
                e, w = _inputs(count, seed=count + offset)
                e_dev = torch.zeros(count + 8, device=DEV)[offset:offset + count].copy_(e)
                w_dev = torch.zeros(count + 8, device=DEV)[offset:offset + count].copy_(w)
                assert e_dev.data_ptr() % 16 == 4 * offset
                omd_dev = omd32.to(DEV).view(1) if through_dev else None
                lib.ema_update(e_dev, w_dev, 0.5 if through_dev else float(omd32), omd_dev)  # (the device rate replaces the float)
                torch.cuda.synchronize()
                _check(e_dev.cpu(), e, w, omd32, f"count {count} omd {rate} offset {offset} dev {through_dev}")
    # two denormals under omd = 1: w - e and (w - e) + e are exact in float32, so the pass returns w itself
    gen = torch.Generator().manual_seed(count)
    e, w = (torch.rand(count, generator=gen) * TINY * 0.5).float(), (-torch.rand(count, generator=gen) * TINY * 0.5).float()
    e_dev, w_dev = e.to(DEV), w.to(DEV)
    lib.ema_update(e_dev, w_dev, 1.0)
    assert torch.equal(e_dev.cpu(), w) and bool((w != 0).any())


# ---------------------------------------------------------------------------------------------- 2. every step mode
@pytest.mark.parametrize("name", tm.ROW_NAMES)
def test_every_step_mode_averages_as_the_stand_alone_pass_does(monkeypatch, name):
    """Three single steps (first-step plan, steady plan, graph replay) of each row of trainer_modes.ROWS."""
    row = tm.BY_NAME[name]
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    batches = ec.fresh_batches(3, cfg["batch"], cfg["image"], cfg["classes"])
    with tm.trainer_for(cfg, ema_decay=ec.DECAY) as (averaged, _), tm.trainer_for(cfg) as (plain, _):
        assert averaged.mode == plain.mode  # (the option is no input of the mode; the row's mode is held by test_gpu_trainer_modes.py)
        feed = [lambda tr, b=b: tr.step(b[0].to(DEV), b[1].to(DEV)) for b in batches]
        ec.pair_steps(averaged, plain, feed, name)


def test_the_average_of_clamped_weights_stays_inside_the_bound(monkeypatch):
    """Row A with weight_clip = 1: the average is formed from the CLAMPED weights, so the four clipped tensors' averages lie in
    [-1, 1] although the un-clamped update leaves it (weight_clip_cases.rescale: half of each tensor starts on the bound)."""
    row = tm.BY_NAME["A"]
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    batches = ec.fresh_batches(3, cfg["batch"], cfg["image"], cfg["classes"])
    with tm.trainer_for(cfg, ema_decay=ec.DECAY, weight_clip=1.0) as (averaged, _), tm.trainer_for(cfg, weight_clip=1.0) as (plain, _):
        for tr in (averaged, plain):
            wc.rescale(tr.p, 1.0)
            for k in wc.CLIPPED:
                tr.p[k].clamp_(-1.0, 1.0)
            tr.max_grad_norm = wc.GRAD_NORM
        averaged.flat_ema.copy_(averaged.flat_params)  # (the average of a run that started from these weights)
        feed = [lambda tr, b=b: tr.step(b[0].to(DEV), b[1].to(DEV)) for b in batches]
        ec.pair_steps(averaged, plain, feed, "A weight_clip=1")
        ema = averaged.ema_state()
        for k in wc.CLIPPED:
            assert float(ema[k].abs().max()) <= 1.0, k
            on_bound = float((averaged.p[k].abs() == 1.0).float().mean())
            assert on_bound > 0.0, f"{k}: no weight sits on the bound -- the clamp was not at work"
        assert float(ema["conv.weight"].abs().max()) > 1.0  # (not a clipped tensor: its average follows it outside)


# ---------------------------------------------------------------------------------------------- 3. the table forms
TABLE_CASES = [(o, f) for o in sorted(OPTIMIZERS) for f in ("1", "0")]


@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_table_forms_single_steps(monkeypatch, optimizer, fuse_next):
    averaged = _trainer(monkeypatch, fuse_next, ema_decay=ec.DECAY, **OPTIMIZERS[optimizer])
    plain = _trainer(monkeypatch, fuse_next, **OPTIMIZERS[optimizer])
    assert averaged.fuse_table_update and plain.fuse_table_update
    start = averaged.ema_state()["input.weight"].clone()
    ec.pair_steps(averaged, plain, [lambda tr, s=s: tr.step(slot=s) for s in (0, 1, 2)], f"table {optimizer} next={fuse_next}")
    # bite: with weight decay and lr > 0 every table element moves in every step, and the average lags behind it
    table, ema = averaged.p["input.weight"], averaged.ema_state()["input.weight"]
    assert float((ema != table).float().mean()) >= 0.5 and float((ema != start).float().mean()) >= 0.5


@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_a_step_group_is_three_single_steps(monkeypatch, optimizer, fuse_next):
    """step_many((0, 1, 2)) after two recording steps against five single steps; with the next forward fused the average of the
    table rows is kept by the fused pass itself (the kEma forms of its kernel)."""
    group = _trainer(monkeypatch, fuse_next, ema_decay=ec.DECAY, **OPTIMIZERS[optimizer])
    single = _trainer(monkeypatch, fuse_next, ema_decay=ec.DECAY, **OPTIMIZERS[optimizer])
    for tr in (group, single):
        tr.step(slot=0)
        tr.step(slot=1)
    ring = group.step_many((0, 1, 2)).clone()
    losses = torch.stack([single.step(slot=s).clone() for s in (0, 1, 2)])
    torch.cuda.synchronize()
    assert group.steps_done == single.steps_done == 5
    assert torch.equal(ring, losses), (ring, losses)
    for a, b in zip(ec.state_of(group), ec.state_of(single)):
        assert torch.equal(a, b)
    assert torch.equal(group.flat_ema, single.flat_ema)
    assert float((group.flat_ema != group.flat_params).float().mean()) >= 0.5


@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_table_forms_launch_the_averaging_siblings(monkeypatch, optimizer, fuse_next):
    """The _ema siblings of EXPECTED and no further launch: the fused update + next-forward pass carries the average too."""
    tr = _trainer(monkeypatch, fuse_next, ema_decay=ec.DECAY, **OPTIMIZERS[optimizer])
    single, group = _logged(monkeypatch, tr)
    want_single, want_group = EXPECTED[(optimizer, fuse_next)]

    assert single == [SIBLING.get(n, n) for n in want_single]
    assert group == [SIBLING.get(n, n) for n in want_group]
    assert "nnue_ema_update" not in single + group and len(group) == len(want_group)
    assert any(n.endswith("_ema") for n in single)
    assert (fuse_next == "1") == any(n.startswith("nnue_ftm_backward_weight_update_forward") for n in group)


# ---------------------------------------------------------------------------------------------- 4. off is plain
@pytest.mark.parametrize("optimizer,fuse_next", TABLE_CASES)
def test_off_is_plain(monkeypatch, optimizer, fuse_next):
    off = _trainer(monkeypatch, fuse_next, ema_decay=0.0, **OPTIMIZERS[optimizer])
    without = _trainer(monkeypatch, fuse_next, **OPTIMIZERS[optimizer])
    assert off.flat_ema is None and off.ema_omd_dev is None
    for s in (0, 1, 2):
        a, b = off.step(slot=s).clone(), without.step(slot=s).clone()
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    for a, b in zip(ec.state_of(off), ec.state_of(without)):
        assert torch.equal(a, b)
    fresh = _trainer(monkeypatch, fuse_next, ema_decay=0.0, **OPTIMIZERS[optimizer])
    assert _logged(monkeypatch, fresh) == tuple(list(x) for x in EXPECTED[(optimizer, fuse_next)])
    with pytest.raises(ValueError, match="ema_decay"):
        off.ema_state()
    with pytest.raises(ValueError, match="switched"):
        off.ema_decay = 0.5


# ---------------------------------------------------------------------------------------------- 5. warm-up
@pytest.mark.parametrize("optimizer,fuse_next", (("sgd_momentum", "1"), ("adam", "0")))
def test_warm_up_in_single_steps_and_in_a_group(monkeypatch, optimizer, fuse_next):
    from nnue_hip import lib
    table = lib.ema_warmup_table(0.999)
    single = _trainer(monkeypatch, fuse_next, ema_decay=0.999, ema_warmup=True, **OPTIMIZERS[optimizer])
    group = _trainer(monkeypatch, fuse_next, ema_decay=0.999, ema_warmup=True, **OPTIMIZERS[optimizer])
    plain = _trainer(monkeypatch, fuse_next, **OPTIMIZERS[optimizer])
    slots = (0, 1, 2, 0, 1, 2, 0)
    # single steps against the stand-alone pass at the table's rates; the third step's rate is the table's third entry
    seen = []

    def step(tr, s):
        loss = tr.step(slot=s)
        if tr is single:
            seen.append(single.ema_omd_dev.clone())
        return loss
    ec.pair_steps(single, plain, [lambda tr, s=s: step(tr, s) for s in slots], f"warm-up {optimizer}",
                  omd_of_step=lambda i: float(table[i]))
    assert [float(x) for x in seen] == [float(table[i]) for i in range(7)] and float(seen[2]) == float(table[2])
    assert single.ema_position == 7 and int(single.ema_pos) == 7
    # two recording steps, then a group of FIVE replayed as one graph (five ticks of the in-graph position): the same seven steps
    group.step(slot=0)
    group.step(slot=1)
    group.step_many((2, 0, 1, 2, 0))
    torch.cuda.synchronize()
    assert ((2, 0, 1, 2, 0), "many") in group._g_local
    assert group.steps_done == 7 and group.ema_position == 7 and int(group.ema_pos) == 7
    assert torch.equal(group.flat_ema, single.flat_ema) and torch.equal(group.flat_params, single.flat_params)
    assert torch.equal(group.ema_omd_dev, single.ema_omd_dev)


def test_a_new_decay_is_one_fill(monkeypatch):
    """``trainer.ema_decay = x`` keeps plans and graphs: the next replayed step averages at the new rate."""
    from nnue_hip import lib
    averaged = _trainer(monkeypatch, "0", ema_decay=ec.DECAY, momentum=0.9)
    plain = _trainer(monkeypatch, "0", momentum=0.9)
    ec.pair_steps(averaged, plain, [lambda tr, s=s: tr.step(slot=s) for s in (0, 1, 2)], "before the change")
    graphs, plans = dict(averaged._g_local), averaged._plan_update
    averaged.ema_decay = 0.5
    assert averaged._g_local == graphs and averaged._plan_update is plans and float(averaged.ema_omd_dev) == 0.5
    ref = averaged.flat_ema.clone()
    averaged.step(slot=0)
    plain.step(slot=0)
    lib.ema_update(ref, plain.flat_params, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(averaged.flat_ema, ref) and torch.equal(averaged.flat_params, plain.flat_params)


# ---------------------------------------------------------------------------------------------- 6. ema_weights()
def _fresh_from(model, ema_state):
    fresh = copy.deepcopy(model)
    with torch.no_grad():
        named = dict(fresh.named_parameters())
        for k, v in ema_state.items():
            named[k].data = v.detach().clone()
    return fresh


def test_ema_weights_puts_the_average_into_the_live_model(monkeypatch, tmp_path):
    import serialize
    row = tm.BY_NAME["A"]
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    batches = [(i.to(DEV), l.to(DEV)) for i, l in ec.fresh_batches(4, cfg["batch"], cfg["image"], cfg["classes"])]
    with tm.trainer_for(cfg, ema_decay=ec.DECAY, weight_clip=1.0) as (tr, _), tm.trainer_for(cfg, ema_decay=ec.DECAY, weight_clip=1.0) as (twin, _):
        for t in (tr, twin):
            for b in batches[:3]:
                t.step(*b)
        torch.cuda.synchronize()
        model, images = tr.model, batches[3][0]
        before = tr.flat_params.clone()
        fresh = _fresh_from(model, tr.ema_state()).eval()
        assert not torch.equal(tr.flat_ema, tr.flat_params)
        model.eval()
        with torch.no_grad():
            want = fresh(images).clone()
            live = model(images).clone()
        from nnue_hip.trainer import NnueTrainer
        fresh_twin = copy.deepcopy(fresh)  # (a trainer re-binds its model's parameters: `fresh` itself stays as it is)
        want_eval = NnueTrainer(fresh_twin, cfg["batch"], (cfg["image"], cfg["image"]), max_grad_norm=1.0, **tm.hyper(cfg)).evaluate(images).clone()
        with tr.ema_weights() as inside:
            assert inside is tr and torch.equal(tr.flat_params, tr.flat_ema)
            with torch.no_grad():
                assert torch.equal(model(images), want)
            logits = tr.evaluate(images).clone()
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.step(*batches[3])
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.step_many((0,))
            serialize.serialize_model(model, tmp_path / "inside.nnue")
        model.train()
        assert not torch.equal(want, live)
        assert torch.equal(logits, want_eval)  # the trainer's own forward, against a fresh trainer on the fresh model
        assert torch.equal(tr.flat_params, before)  # the exact bits are back
        serialize.serialize_model(fresh, tmp_path / "fresh.nnue")
        assert (tmp_path / "inside.nnue").read_bytes() == (tmp_path / "fresh.nnue").read_bytes()
        # the next step is the step of the undisturbed twin
        a, b = tr.step(*batches[3]).clone(), twin.step(*batches[3]).clone()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(tr.flat_ema, twin.flat_ema)
        for x, y in zip(ec.state_of(tr), ec.state_of(twin)):
            assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------- 7. resume
@pytest.mark.parametrize("optimizer,warmup", (("sgd", False), ("adam", False), ("sgd", True)))
def test_a_resumed_run_continues_bitwise(monkeypatch, optimizer, warmup):
    row = tm.BY_NAME["A_adam" if optimizer == "adam" else "A"]
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    batches = [(i.to(DEV), l.to(DEV)) for i, l in ec.fresh_batches(4, cfg["batch"], cfg["image"], cfg["classes"])]
    kw = dict(ema_decay=0.99, ema_warmup=warmup)
    with tm.trainer_for(cfg, **kw) as (whole, _), tm.trainer_for(cfg, **kw) as (resumed, _), tm.trainer_for(cfg) as (none, _), \
            tm.trainer_for(cfg, ema_decay=0.5, ema_warmup=warmup) as (other, _), tm.trainer_for(cfg, ema_decay=0.99, ema_warmup=not warmup) as (flipped, _):
        for b in batches[:2]:
            whole.step(*b)
        torch.cuda.synchronize()
        sd = copy.deepcopy(whole.state_dict())
        assert sd["ema"]["decay"] == 0.99 and sd["ema"]["warmup"] == warmup and sd["ema"]["position"] == (2 if warmup else 0)
        params = whole.flat_params.clone()
        for tr in (none, other, flipped):  # no average, another decay, the warm-up the other way
            held = ec.state_of(tr)
            with pytest.raises(ValueError, match="weight average|ema_decay"):
                tr.load_state_dict(sd)
            assert tr.steps_done == 0 and all(torch.equal(a, b) for a, b in zip(held, ec.state_of(tr)))
        with pytest.raises(ValueError, match="weight average"):  # a state without the key loads only into a trainer without the average
            whole.load_state_dict({k: v for k, v in sd.items() if k != "ema"})
        none.load_state_dict({k: v for k, v in none.state_dict().items() if k != "ema"})
        resumed.flat_params.copy_(params)
        resumed.load_state_dict(sd)
        assert torch.equal(resumed.flat_ema, whole.flat_ema) and resumed.ema_position == whole.ema_position
        for b in batches[2:]:
            a, c = whole.step(*b).clone(), resumed.step(*b).clone()
            assert torch.equal(a, c)
        torch.cuda.synchronize()
        for x, y in zip(ec.state_of(whole), ec.state_of(resumed)):
            assert torch.equal(x, y)
        assert torch.equal(whole.flat_ema, resumed.flat_ema) and torch.equal(whole.ema_omd_dev, resumed.ema_omd_dev)
        # the rebuilt trainer (the train loop's density switch) carries the average over
        again = whole.rebuilt("mfma")
        assert again.ema_decay == 0.99 and again.ema_warmup == warmup and torch.equal(again.flat_ema, whole.flat_ema)
        assert again.ema_position == whole.ema_position and torch.equal(again.ema_omd_dev, whole.ema_omd_dev)


# ---------------------------------------------------------------------------------------------- 8. the module path
def _module_run(opt_cls, ema_decay, steps=3, **opt_kw):
    """`steps` steps of test_gpu_weight_clip._module_run's model through backward() and the drop-in optimizer.  Returns
    (parameters after every step, optimizer, losses)."""
    from nnue_hip import optim
    torch.manual_seed(3)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 256, 32, 16, num_classes=10).to(DEV)
    named = {k: v for k, v in model.named_parameters() if k != "nnue2score"}
    start = {k: v.detach().clone() for k, v in named.items()}
    table = [named[k] for k in wc.CLIPPED]
    rest = [v for k, v in named.items() if k not in wc.CLIPPED]
    opt = getattr(optim, opt_cls)([dict(params=table, ema_decay=ema_decay, weight_clip=1.0), dict(params=rest)], max_grad_norm=1.0, **opt_kw)
    gen = torch.Generator().manual_seed(4)
    history, losses = [], []
    for _ in range(steps):
        images, labels = torch.randn(16, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (16,), generator=gen).to(DEV)
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(images), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        history.append({k: v.detach().clone() for k, v in named.items()})
        losses.append(loss.detach().clone())
    return start, history, opt, named, losses


@pytest.mark.parametrize("opt_cls,kw", (("SGD", dict(lr=0.05, momentum=0.9, weight_decay=2e-4)), ("Adam", dict(lr=1e-2, weight_decay=2e-4))))
def test_module_path_groups(opt_cls, kw):
    from nnue_hip import lib
    start, got, opt, named, losses = _module_run(opt_cls, ec.DECAY, **kw)
    _, ref, plain_opt, _, ref_losses = _module_run(opt_cls, 0.0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses))
    for a, b in zip(got, ref):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert plain_opt.ema_state() == {}
    ema = opt.ema_state()
    assert set(ema) == {named[k] for k in wc.CLIPPED}  # the option means its group, nothing else
    for k in wc.CLIPPED:
        want = start[k].clone()
        for params in ref:
            lib.ema_update(want, params[k], lib.ema_omd(ec.DECAY))
        torch.cuda.synchronize()
        assert torch.equal(ema[named[k]], want), k
        assert float((want != start[k]).float().mean()) > 0.5 and not torch.equal(want, ref[-1][k])


# ---------------------------------------------------------------------------------------------- 8b. the multi-tensor kernels' other arms
def _views(sizes, offsets, fill):
    """One tensor per (size, offset): a slice of a buffer of its own that starts `offset` floats behind a 16-byte boundary."""
    out = []
    for n, off in zip(sizes, offsets):
        buf = torch.zeros(n + 8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + n]
        v.copy_(fill(n))
        out.append(v)
    return out


@pytest.mark.parametrize("opt_cls,kw", (("SGD", dict(lr=0.05, momentum=0.0, weight_decay=2e-4)), ("Adam", dict(lr=1e-2, weight_decay=2e-4))))
def test_multi_tensor_average_on_misaligned_views_and_long_lists(opt_cls, kw):
    """41 segments -- more than the 38 one launch of a list with averages holds -- of sizes around the units' edges, with every
    combination of offsets within 16 bytes: parameter and gradient alike (SGD without momentum: the vector unit with its head and
    tail; Adam, whose moments are aligned: the scalar unit) or apart (the scalar unit), and the average's offset equal to the
    parameter's or not (16-byte or 4-byte accesses to the average).  Two steps against the run without averages plus the
    stand-alone pass, bitwise."""
    from nnue_hip import lib, optim
    sizes = [1, 3, 4, 5, 7, 1023, 4096, 4099, 9001] * 5
    sizes = sizes[:41]
    p_off = [(i * 5) % 4 for i in range(41)]
    g_off = [(o if i % 3 else (o + 1) % 4) for i, o in enumerate(p_off)]
    e_off = [(o if i % 2 else (o + 2) % 4) for i, o in enumerate(p_off)]
    omd = lib.ema_omd(ec.DECAY)

    def run(decay):
        gen = torch.Generator().manual_seed(9)
        rnd = lambda n: torch.randn(n, generator=gen).to(DEV)  # noqa: E731
        params = [torch.nn.Parameter(v) for v in _views(sizes, p_off, rnd)]
        grads = [_views(sizes, g_off, rnd) for _ in range(2)]
        opt = getattr(optim, opt_cls)([dict(params=params[:30], ema_decay=decay), dict(params=params[30:])], max_grad_norm=1.0, **kw)
        start = [p.detach().clone() for p in params]
        if decay:
            for p, e in zip(params[:30], _views(sizes[:30], e_off[:30], lambda n: torch.zeros(n, device=DEV))):
                e.copy_(p.detach())
                opt.state[p]["ema"] = e  # a caller's own buffer: any 4-byte-aligned view
        history = []
        for step in range(2):
            for p, g in zip(params, grads[step]):
                p.grad = g
            opt.step()
            torch.cuda.synchronize()
            history.append([p.detach().clone() for p in params])
        return start, history, opt, params
    start, got, opt, params = run(ec.DECAY)
    _, ref, _, _ = run(0.0)
    for a, b in zip(got, ref):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    ema = opt.ema_state()
    assert len(ema) == 30
    for i, p in enumerate(params[:30]):
        want = start[i].clone()
        for step in ref:
            lib.ema_update(want, step[i], omd)
        torch.cuda.synchronize()
        assert ema[p].data_ptr() % 16 == 4 * e_off[i]
        assert torch.equal(ema[p], want), (i, sizes[i], p_off[i], g_off[i], e_off[i])
        assert not torch.equal(want, start[i])
