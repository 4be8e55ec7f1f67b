"""A per-step learning-rate schedule inside the step graphs (include/nnue_hip.h: nnue_lr_schedule_step;
NnueTrainer.set_lr_schedule): the reference's configs ask for one value per iteration (training_utils.py:283-336) and fix
the rate per optimizer (train.py:457-471).  The table is made on the host and only indexed on the device, so every check here
is bitwise: a scheduled step or step group against a twin trainer with no schedule, stepped singly with
``twin.lr = float(values[t])`` before each step.  ``-m gpu``."""
import pytest
import torch

from schedule_cases import (BIG_OPTS, DEV, RATES, big_pair, same_state, small_model, small_trainer)

pytestmark = pytest.mark.gpu
INT32_MAX = 2**31 - 1


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
def _run(table, position, calls):
    from nnue_hip import lib
    t = torch.tensor(table, dtype=torch.float32, device=DEV)
    pos = torch.tensor([position], dtype=torch.int32, device=DEV)
    out = torch.full((1,), float("nan"), device=DEV)
    got = []
    for _ in range(calls):
        lib.lr_schedule_step(t, pos, out)
        got.append(float(out))
    return got, int(pos), t.cpu().tolist()


def test_kernel_indexes_clamps_and_advances():
    got, pos, t = _run([0.5, 0.25, 0.125, 0.0625, 0.03125], 3, 4)
    assert got == [t[3], t[4], t[4], t[4]] and pos == 7
    got, pos, t = _run([0.1] * 4 + [0.7], 0, 5)
    assert got == t and pos == 5
    got, pos, t = _run([0.3], 0, 3)  # n = 1
    assert got == [t[0]] * 3 and pos == 3
    got, pos, t = _run([0.5, 0.25], -5, 2)  # a negative position reads the first value and counts up
    assert got == [t[0], t[0]] and pos == -3


def test_kernel_position_saturates_without_overflow():
    got, pos, t = _run([0.5, 0.25, 0.125], INT32_MAX - 1, 2)
    assert got == [t[2], t[2]] and pos == INT32_MAX
    got, pos, t = _run([0.5, 0.25, 0.125], INT32_MAX, 2)
    assert got == [t[2], t[2]] and pos == INT32_MAX


def test_wrapper_refuses_wrong_tensors():
    from nnue_hip import lib
    t, pos, out = torch.ones(4, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(TypeError):
        lib.lr_schedule_step(t, pos.long(), out)
    with pytest.raises(ValueError):
        lib.lr_schedule_step(t.view(2, 2), pos, out)
    with pytest.raises(ValueError):
        lib.lr_schedule_step(t[:0], pos, out)
    with pytest.raises(lib.NnueHipError):
        lib.lr_schedule_step(t.cpu(), pos, out)


# ---------------------------------------------------------------------------------------------- 2. small shape
def _twin_steps(twin, values, t0, slots):
    """Single steps of the schedule-less twin under the same values; step number t uses values[min(t, len - 1)]."""
    losses = []
    for i, s in enumerate(slots):
        twin.lr = float(values[min(t0 + i, len(values) - 1)])
        losses.append(twin.step(slot=s).clone())
    return torch.stack(losses)


def _agree(tr, twin, got, want, what):
    assert torch.equal(got, want), (what, got, want)
    assert torch.equal(tr.flat_params, twin.flat_params), what
    assert torch.equal(tr.flat_momentum, twin.flat_momentum), what
    assert int(tr.lr_pos) == tr.steps_done == tr.lr_position == twin.steps_done, what


@pytest.mark.parametrize("use_graph", (False, True))
def test_scheduled_steps_and_groups_are_the_single_steps_under_the_same_values(use_graph):
    model, twin_model = small_model(), small_model()
    tr, twin = small_trainer(model, use_graph), small_trainer(twin_model, use_graph)
    assert torch.equal(tr.flat_params, twin.flat_params)
    tr.set_lr_schedule(RATES)
    assert tr.lr == float(RATES[0]) and tr.lr_position == 0 and int(tr.lr_pos) == 0
    t = 0
    for s in (0, 1):
        got = tr.step(slot=s).clone().view(1)
        _agree(tr, twin, got, _twin_steps(twin, RATES, t, (s,)), f"step {t}")
        t += 1
        if s == 0:  # recording the plans executed two updates and put everything back
            assert int(tr.lr_pos) == 1 and float(tr.lr_dev) == float(RATES[0])
        assert tr.lr == float(RATES[t]) and tr.lr_last == float(RATES[t - 1])
    for group in ((0, 1, 2), (0, 1, 2, 1), (2,), (0, 1, 2), (1, 0)):  # the fourth crosses the end of the table
        got = tr.step_many(group).clone()
        _agree(tr, twin, got, _twin_steps(twin, RATES, t, group), f"group {group} from step {t}")
        t += len(group)
        if use_graph:
            assert (group, "many") in tr._g_local
    assert t == 15 > len(RATES)
    got = tr.step(slot=0).clone().view(1)  # a single step past the end: the last value holds
    _agree(tr, twin, got, _twin_steps(twin, RATES, t, (0,)), "past the end")
    assert float(tr.lr_dev) == float(RATES[-1]) == tr.lr == tr.lr_last
    timers = {"nnue_sgd_step": [], "nnue_lr_schedule_step": []}
    tr.set_lr_schedule(RATES, position=4)  # replaced: step numbers count from the given position
    got = tr.step(slot=1, timers=timers).clone().view(1)  # the eager, timed form
    want = _twin_steps(twin, RATES, 4, (1,))
    assert torch.equal(got, want) and torch.equal(tr.flat_params, twin.flat_params) and torch.equal(tr.flat_momentum, twin.flat_momentum)
    assert len(timers["nnue_lr_schedule_step"]) == 1 == len(timers["nnue_sgd_step"]) and int(tr.lr_pos) == 5 == tr.lr_position
    got = tr.step_many((0, 2), timers=timers).clone()  # the group's eager, timed form
    assert torch.equal(got, _twin_steps(twin, RATES, 5, (0, 2))) and torch.equal(tr.flat_params, twin.flat_params)
    assert len(timers["nnue_lr_schedule_step"]) == 3 and int(tr.lr_pos) == 7 == tr.lr_position
    # a padded short batch takes the eager update: the schedule's launch is in it as well
    images, labels = tr.inputs[0][0][:5].clone(), tr.inputs[0][1][:5].clone()
    twin.lr = float(RATES[7])
    assert torch.equal(tr.step(images, labels, slot=2), twin.step(images, labels, slot=2))
    assert torch.equal(tr.flat_params, twin.flat_params) and int(tr.lr_pos) == 8 == tr.lr_position


def test_lr_property_and_clearing():
    tr = small_trainer(small_model())
    with pytest.raises(ValueError):
        tr.set_lr_schedule(RATES, position=-1)
    with pytest.raises(ValueError):
        tr.set_lr_schedule([])
    with pytest.raises(ValueError):
        tr.set_lr_schedule(RATES.view(3, 4))
    assert tr.lr_table is None and tr.lr == 0.01
    tr.set_lr_schedule(RATES.tolist(), position=2)  # any 1-D sequence
    assert tr.lr_table.dtype == torch.float32 and tr.lr_pos.dtype == torch.int32 and tuple(tr.lr_pos.shape) == (1,)
    assert tr.lr == float(RATES[2])
    with pytest.raises(ValueError, match="clear the schedule first"):
        tr.lr = 0.5
    tr.step(slot=0)
    tr.step_many((1, 2))
    assert tr.lr == float(RATES[5]) and float(tr.lr_dev) == float(RATES[4])
    tr.clear_lr_schedule()
    assert tr.lr_table is None and tr.lr == float(RATES[4]) == float(tr.lr_dev)  # the rate stays at the last value used
    tr.lr = 0.002
    assert float(tr.lr_dev) == pytest.approx(0.002)
    before = tr.flat_params.clone()
    tr.step(slot=0)
    assert not torch.equal(before, tr.flat_params) and float(tr.lr_dev) == pytest.approx(0.002)


def test_rebuilt_carries_the_schedule_and_its_position():
    model, twin_model = small_model(), small_model()
    tr, twin = small_trainer(model), small_trainer(twin_model)
    tr.set_lr_schedule(RATES)
    tr.step(slot=0)
    tr.step_many((1, 2))
    _twin_steps(twin, RATES, 0, (0, 1, 2))
    data = [(im.clone(), lb.clone()) for im, lb in tr.inputs]
    new = tr.rebuilt("mfma")
    for (im, lb), (ti, tl) in zip(data, new.inputs):
        ti.copy_(im)
        tl.copy_(lb)
    assert new.lr_position == 3 == int(new.lr_pos) and torch.equal(new.lr_table, tr.lr_table) and new.lr == float(RATES[3])
    got = torch.stack([new.step(slot=0).clone(), new.step(slot=1).clone()])
    assert torch.equal(got, _twin_steps(twin, RATES, 3, (0, 1))) and torch.equal(new.flat_params, twin.flat_params)


# ---------------------------------------------------------------------------------------------- 3. the big-table modes
@pytest.mark.parametrize("kind", ("adam", "sgd"))
def test_scheduled_groups_at_the_big_table_are_the_single_steps(monkeypatch, kind):
    """Groups whose table update also forms the next step's forward (two alternating maps, the optimizer's two launches
    apart): one odd and one even group under a per-step schedule, bitwise the twin's single steps with the fused next forward
    off under the same values -- parameters, moments or momentum, losses."""
    values = RATES * 0.1 if kind == "adam" else RATES
    tr, twin = big_pair(monkeypatch, **BIG_OPTS[kind])
    tr.set_lr_schedule(values)
    got = tr.step(slot=0).clone().view(1)
    assert torch.equal(got, _twin_steps(twin, values, 0, (0,))) and same_state(tr, twin)
    t = 1
    for group in ((1, 2, 0), (1, 2, 0, 1)):
        got = tr.step_many(group).clone()
        want = _twin_steps(twin, values, t, group)
        t += len(group)
        assert torch.equal(got, want), (group, got, want)
        assert same_state(tr, twin), group
        assert (group, "many") in tr._g_local and int(tr.lr_pos) == t == tr.steps_done == tr.lr_position
    if kind == "adam":
        assert int(tr.adam_step_count) == t == int(twin.adam_step_count)
    assert float(tr.lr_dev) == float(values[t - 1])


# ---------------------------------------------------------------------------------------------- 4. graph bookkeeping
def _names(plan):
    return [c[0] for c in plan]


def test_no_schedule_no_new_call_and_only_update_graphs_are_dropped():
    a, b, c = (small_trainer(small_model()) for _ in range(3))
    c.set_lr_schedule(RATES)
    for tr in (a, b, c):
        tr.step(slot=0)
        tr.step(slot=0)
        tr.step_many((0, 1))
    for plan in ("_plan_update_first", "_plan_update"):
        assert "nnue_lr_schedule_step" not in _names(getattr(a, plan))
        assert _names(getattr(a, plan)) == _names(getattr(b, plan))
        # the scheduled trainer's plan is the same list behind ONE schedule call
        assert _names(getattr(c, plan)) == ["nnue_lr_schedule_step"] + _names(getattr(a, plan))
    assert "nnue_lr_schedule_step" not in _names(a._plan_local) and _names(a._plan_local) == _names(c._plan_local)
    before, plan_local, update_graph = set(a._g_local), a._plan_local, a._g_update
    with_update = {k for k in before if k[1] in ("full", "full_dp", "many")}
    assert with_update and before - with_update and update_graph is not None
    a.set_lr_schedule(RATES)
    assert set(a._g_local) == before - with_update, "attaching a schedule drops the graphs that contain an update, no others"
    assert a._g_update is None and a._plan_update is None and a._plan_local is plan_local
    a.step(slot=0)
    a.step_many((0, 1))
    assert _names(a._plan_update) == _names(c._plan_update) and set(a._g_local) == before
    # load_state_dict with a schedule of the same length copies in place: every graph stays
    graphs, update_graph, table = dict(a._g_local), a._g_update, a.lr_table.data_ptr()
    sd = c.state_dict()
    sd["lr_schedule"]["values"] = sd["lr_schedule"]["values"].flip(0)
    a.load_state_dict(sd)
    assert set(a._g_local) == set(graphs) and all(a._g_local[k] is graphs[k] for k in graphs) and a._g_update is update_graph
    assert a.lr_table.data_ptr() == table and torch.equal(a.lr_table.cpu(), RATES.flip(0)) and int(a.lr_pos) == c.lr_position
    # clearing drops them again
    a.clear_lr_schedule()
    assert set(a._g_local) == before - with_update and a._plan_update is None
