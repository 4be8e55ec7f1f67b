"""Every step mode of tests/trainer_modes.py's table on the GPU: the live trainer takes the mode the table says (flags, phase
mask, STE stages, launch list), three eager optimizer steps in that mode -- clip active, clip inactive, a short last batch --
follow the float64 oracle at the project's bars, and the same steps as graph replays and as one step group are bitwise the
eager ones.  One test per row, and one of the kernel family handed to ``rebuilt`` as an argument; ``-m gpu``.  Each row prints one ``TRAINER_MODE {json}`` line (mode, launches, worst error over
each bar): profiles/trainer_modes.md is that record."""
import json
import os

import pytest
import torch

from trainer_modes import A, BY_NAME, ROW_NAMES, CallLog, build_model, check_step, differences, flags_of, hyper, launches_of, modes_of, \
    oracle_steps, same, set_knobs, snapshot, trainer_for

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _feed(tr, ref, slot):
    tr.max_grad_norm = ref["max_grad_norm"]
    return tr.step(ref["images"].to(DEV), ref["labels"].to(DEV), slot=slot)


@pytest.mark.parametrize("name", ROW_NAMES)
def test_the_row_takes_its_mode_and_its_steps_follow_the_oracle(name, monkeypatch):
    row = BY_NAME[name]
    cfg = row.config
    set_knobs(monkeypatch, row)
    record = dict(row=name, ratios={})
    try:
        # ---- 1. the mode
        with trainer_for(cfg, use_graph=False, input_slots=3) as (eager, params):
            wrong = differences(flags_of(eager), {k: v for k, v in row.modes.items() if k not in ("phases", "ste_launch")})
            assert not wrong, f"{name}: " + "; ".join(wrong)
            # ---- 2. three eager steps against the oracle
            refs, states, losses, log = [], [], [], None
            for ref in oracle_steps(cfg, params):
                was = {k: v.detach().clone() for k, v in eager.p.items()}
                with CallLog() as seen:
                    loss = _feed(eager, ref, ref["step"])
                if ref["step"] == 1:
                    log = seen
                check_step(eager, ref, was, loss, f"{name} step {ref['step']}", record["ratios"])
                refs.append(ref)
                states.append(snapshot(eager))
                losses.append(loss.clone())
            mode, launches = modes_of(eager, log)
            record.update(mode=mode, launches=launches)
            wrong = differences(mode, row.modes)
            assert not wrong, f"{name}: " + "; ".join(wrong)
            assert launches == launches_of(row.modes), f"{name}: launches {launches}, the mode implies {launches_of(row.modes)}"
            # ---- 3. the same steps as graph replays, then the three slots once more singly and as one group
            with trainer_for(cfg, use_graph=True, input_slots=3) as (single, _), trainer_for(cfg, use_graph=True, input_slots=3) as (group, _):
                graph_ratios = {}
                for ref in refs:
                    for tr in (single, group):
                        was = {k: v.detach().clone() for k, v in tr.p.items()}
                        loss = _feed(tr, ref, ref["step"])
                        torch.cuda.synchronize()
                        if row.bitwise:
                            assert torch.equal(loss, losses[ref["step"]]) and same(snapshot(tr), states[ref["step"]]), \
                                f"{name} step {ref['step']}: the graph step is not bitwise the eager one"
                        else:
                            check_step(tr, ref, was, loss, f"{name} graph step {ref['step']}", graph_ratios)
                assert differences(flags_of(single), flags_of(eager)) == []
                want = [eager.step(slot=s).clone() for s in (0, 1, 2)]
                got_single = [single.step(slot=s).clone() for s in (0, 1, 2)]
                got_group = group.step_many((0, 1, 2)).clone()
                torch.cuda.synchronize()
                assert ((0, 1, 2), "many") in group._g_local and group.steps_done == single.steps_done == eager.steps_done == 6
                if row.bitwise:
                    assert torch.equal(torch.stack(got_single), torch.stack(want)) and same(snapshot(single), snapshot(eager)), \
                        f"{name}: single graph steps on the slots are not bitwise the eager ones"
                    assert torch.equal(got_group, torch.stack(got_single)) and same(snapshot(group), snapshot(single)), \
                        f"{name}: the step group is not bitwise the single graph steps"
                else:
                    from conftest import assert_close_grad
                    for tr, losses_ in ((single, torch.stack(got_single)), (group, got_group)):
                        assert_close_grad(losses_, torch.stack(want), f"{name}: losses on the slots")
                        for a, b in zip(snapshot(tr), snapshot(eager)):
                            assert_close_grad(a.float(), b.float(), f"{name}: state after the slots")
    finally:
        print("TRAINER_MODE " + json.dumps(record, sort_keys=True))


def test_rebuilt_takes_the_family_as_an_argument_and_the_flags_live_in_the_mode_alone(monkeypatch):
    """Configuration A at batch 40 (the smallest shape of the suite at which all three kernel families run): rebuilt(p) leaves
    the process environment alone and gives the trainer a fresh one gives under NNUE_FT_PATH=p -- the same mode, and bitwise the
    same first step; the mode's flags on the trainer are read-only views of ``trainer.mode``."""
    from nnue_hip.trainer import NnueTrainer
    cfg = dict(A, batch=40)
    set_knobs(monkeypatch, BY_NAME["A"])
    gen = torch.Generator().manual_seed(11)
    images = torch.rand((40, 3, 32, 32), generator=gen).to(DEV)
    labels = torch.randint(0, cfg["classes"], (40,), generator=gen).to(DEV)
    with trainer_for(cfg) as (tr, _):
        assert tr.ft_path == "mfma"
        snap = dict(os.environ)
        for path in ("bits", "list", "mfma"):
            tr2 = tr.rebuilt(path)
            assert dict(os.environ) == snap
            assert tr2.ft_path == path and tr2.steps_done == 0
            twin = build_model(cfg)
            twin.load_state_dict({k: v.detach().clone() for k, v in tr2.model.state_dict().items()})
            with monkeypatch.context() as forced:
                forced.setenv("NNUE_FT_PATH", path)
                fresh = NnueTrainer(twin.to(DEV), 40, (32, 32), max_grad_norm=1.0, **hyper(cfg))
            assert tr2.mode == fresh.mode, f"{tr2.mode.describe()} != {fresh.mode.describe()}"
            for t in (tr2, fresh):
                t.step(images, labels)
            torch.cuda.synchronize()
            assert torch.equal(tr2.flat_params, fresh.flat_params) and torch.equal(tr2.grad_norm, fresh.grad_norm), path
        with pytest.raises(AttributeError):
            tr.fuse_l1 = False
        assert tr.fuse_l1 is tr.mode.fuse_l1
