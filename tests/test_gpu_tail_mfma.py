"""The classifier's tile tail on the f32 MFMA (tail_dx_train_kernel: h2, logits, d_z2 and d_z1 of a 16-row tile as
v_mfma_f32_16x16x4_f32 tiles) at nnue_classifier_train_step.  ``-m gpu``.  Cases, launches, references:
tests/tail_mfma_cases.py.

Shapes: L2 = 128, L3 = 32 (the only widths the kernel is built for); L1 in {128, 256} (one and two column groups, 2 and 4
slabs); B in {1, 15, 16, 17, 33} (inside, at and past a row tile); C in {1, 2, 3, 10, 63, 64} (pad k of d_z2, pad columns of
logits, the kTdxMaxC edge); clip off and 1.0.  Every launch asserts that the fused predicate takes its shape.

  float64     every output against a float64 torch restatement from the launch's own inputs, stage by stage, at the
              element-wise bars of tests/test_gpu_classifier_train.py (imported).  Each case prints its worst
              max|got - ref| / max|ref| per output under ``pytest -s``; on the CPU a plain float32 restatement of h1, h2 and
              logits says what to expect (printed beside it).
  exact       operands on binary grids coarse enough that every partial sum is exact in float32: the four products EQUAL
              the float64 values.
  rows        permuting the batch rows permutes every per-row output bitwise; a row at B = 17 is bitwise that row alone.
  regimes     a NaN row stays in its row; labels -1 and C; logits near +-1e4 (every float64 case); W3 an interior view of a
              NaN-filled allocation and scratch NaN around d_logits / d_z2 / d_z1 (every float64 case).
  forms       phases 123 bitwise phases 59; a second launch bitwise the first; the C2 architecture at B = 160 for three
              optimizer steps eagerly, as per-step graphs and through step_many against the float64 oracle.
"""
import pytest
import torch

import tail_mfma_cases as tc
from test_gpu_classifier_train import assert_within, c64

pytestmark = pytest.mark.gpu
DEV = "cuda"

BS, CS = (1, 15, 16, 17, 33), (1, 2, 3, 10, 63, 64)
FORMS = ((128, 0.0), (256, 1.0))
FLOAT64_CASES = [(B, L1, C, clip, True) for B in BS for C in CS for L1, clip in FORMS]
# unit-scale logits (an unsaturated softmax: every class carries a gradient into d_z2) with the other (L1, clip) pairing
FLOAT64_CASES += [(B, L1, C, clip, False) for B in (17, 33) for C in CS for L1, clip in ((128, 1.0), (256, 0.0))]


def ratio(got, ref):
    got, ref = c64(got), c64(ref)
    fin = torch.isfinite(ref)
    den = float(ref[fin].abs().max()) if bool(fin.any()) else 0.0
    return float((got - ref)[fin].abs().max()) / den if den > 0 else 0.0


@pytest.mark.parametrize("B,L1,C,clip,big", FLOAT64_CASES)
def test_every_output_against_float64(B, L1, C, clip, big):
    c = tc.make_case(B, L1, C, seed=1000 * B + 10 * C + L1, big_logits=big)
    got, scratch, w3_whole = tc.launch(c, clip, 123, band_w3=True)
    ref = tc.reference(c, got, clip)
    cpu = tc.float32_restatement(c, clip)
    line = []
    for name in tc.NAMES:
        r, bound = ref[name]
        line.append(f"{name} {ratio(got[name], r):.2e}" + (f" (f32 on the CPU {ratio(cpu[name], r):.2e})" if name in cpu else ""))
    print(f"\nB={B} L1={L1} C={C} clip={clip} big={big}: " + ", ".join(line))
    for name in tc.NAMES:
        r, bound = ref[name]
        assert_within(got[name], r, bound, f"B={B} L1={L1} C={C} clip={clip} {name}")
    # labels outside [0, C): exact zeros
    bad = ~((c["labels"] >= 0) & (c["labels"] < C))
    assert bool(bad.any())
    assert bool((got["sample_loss"].cpu()[bad] == 0).all()) and bool((got["d_logits"].cpu()[bad] == 0).all())
    if big and C >= 2:
        assert float(got["logits"].abs().max()) > 5e3, "the saturated softmax regime"
    # the NaN around W3 and around the scratch outputs was neither read into a sum nor written over
    assert bool(torch.isnan(w3_whole[:tc.BAND]).all()) and bool(torch.isnan(w3_whole[-tc.BAND:]).all())
    assert tc.scratch_bands_untouched(c, got, scratch)


@pytest.mark.parametrize("B,L1,C", [(17, 128, 10), (33, 256, 64), (16, 128, 1), (15, 256, 3), (33, 128, 63), (1, 128, 2)])
def test_grid_operands_give_the_float64_products_exactly(B, L1, C):
    c = tc.make_grid_case(B, L1, C, seed=B + L1 + C)
    ref = tc.grid_reference(c)
    got, _, _ = tc.launch(c, 0.0, 123)
    for name in ("h1", "h2", "logits", "d_logits", "d_z2", "d_z1"):
        assert torch.equal(c64(got[name]), ref[name]), name
    if C > 1 and B > 1:
        assert float(got["d_z2"].abs().max()) > 0 and float(got["d_z1"].abs().max()) > 0, "the backward products are exercised"


@pytest.mark.parametrize("B,L1,C,clip", [(33, 128, 10, 0.0), (17, 256, 63, 1.0)])
def test_permuting_the_rows_permutes_the_outputs_bitwise(B, L1, C, clip):
    c = tc.make_case(B, L1, C, seed=5 * B + C)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    a, _, _ = tc.launch(c, clip, 123)
    b, _, _ = tc.launch(tc.permuted(c, perm), clip, 123)
    for name in tc.NAMES:
        assert torch.equal(tc.bits(b[name]), tc.bits(a[name][perm.to(DEV)])), name


@pytest.mark.parametrize("row", (0, 5, 16))
def test_a_row_of_b17_is_bitwise_that_row_alone(row):
    c = tc.make_case(17, 128, 10, seed=171, odd_labels=False)
    whole, _, _ = tc.launch(c, 1.0, 123)
    alone, _, _ = tc.launch(tc.rows_of(c, [row]), 1.0, 123)
    for name in tc.NAMES:
        assert torch.equal(tc.bits(alone[name][0]), tc.bits(whole[name][row])), name


@pytest.mark.parametrize("clip", (0.0, 1.0))
def test_a_nan_row_stays_in_its_row(clip):
    B, row = 33, 18
    c = tc.make_case(B, 128, 10, seed=33, odd_labels=False)
    clean, _, _ = tc.launch(c, clip, 123)
    bad = dict(c)
    bad["slabs"] = c["slabs"].clone()
    bad["slabs"][1, row] = float("nan")
    got, _, _ = tc.launch(bad, clip, 123)
    others = torch.arange(B) != row
    for name in tc.NAMES:
        assert torch.equal(tc.bits(got[name][others.to(DEV)]), tc.bits(clean[name][others.to(DEV)])), name
    for name in ("h1", "h2", "logits", "sample_loss", "d_logits"):
        assert bool(torch.isnan(got[name][row]).all()), name
    for name in ("d_z2", "d_z1", "d_x"):
        # torch's rule: clamp blocks the gradient at a NaN activation (an exact 0), relu passes it
        assert bool((got[name][row] == 0).all() if clip > 0 else torch.isnan(got[name][row]).all()), name


def test_phases_123_are_bitwise_phases_59_and_a_second_launch_the_first():
    c = tc.make_case(17, 128, 10, seed=59)
    ref, ref_scratch, _ = tc.launch(c, 1.0, 59)
    got, got_scratch, _ = tc.launch(c, 1.0, 123)
    again, again_scratch, _ = tc.launch(c, 1.0, 123)
    for name in tc.NAMES:
        assert bool(torch.isfinite(ref[name]).all()), name
        assert torch.equal(tc.bits(got[name]), tc.bits(ref[name])), name
        assert torch.equal(tc.bits(again[name]), tc.bits(got[name])), name
    assert torch.equal(got_scratch, ref_scratch) and torch.equal(again_scratch, got_scratch)


def test_three_trainer_steps_at_b160_follow_the_oracle_in_every_launch_form(monkeypatch):
    """The C2 architecture at batch 160 (ten row tiles, the fused tail + d_x launch): three optimizer steps eagerly, as per-step
    graphs and through step_many against the float64 oracle at trainer_modes.check_step's bars; the graph forms bitwise the
    eager one."""
    import trainer_modes as tm
    row = tm.Row("c2_b160", cfg=dict(l1=1024, l2=128, l3=32, batch=160))
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    with tm.trainer_for(cfg, use_graph=False, input_slots=3) as (eager, params):
        assert eager.fuse_tail_dx
        refs, states = [], []
        for ref in tm.oracle_steps(cfg, params):
            was = {k: v.detach().clone() for k, v in eager.p.items()}
            eager.max_grad_norm = ref["max_grad_norm"]
            loss = eager.step(ref["images"].to(DEV), ref["labels"].to(DEV), slot=ref["step"])
            tm.check_step(eager, ref, was, loss, f"eager step {ref['step']}", {})
            refs.append(ref)
            states.append(tm.snapshot(eager))
        with tm.trainer_for(cfg, use_graph=True, input_slots=3) as (single, _), tm.trainer_for(cfg, use_graph=True, input_slots=3) as (group, _):
            for ref in refs:
                for tr in (single, group):
                    was = {k: v.detach().clone() for k, v in tr.p.items()}
                    tr.max_grad_norm = ref["max_grad_norm"]
                    loss = tr.step(ref["images"].to(DEV), ref["labels"].to(DEV), slot=ref["step"])
                    tm.check_step(tr, ref, was, loss, f"graph step {ref['step']}", {})
                    assert tm.same(tm.snapshot(tr), states[ref["step"]]), f"graph step {ref['step']} is not bitwise the eager one"
            want = torch.stack([eager.step(slot=s).clone() for s in (0, 1, 2)])
            got_single = torch.stack([single.step(slot=s).clone() for s in (0, 1, 2)])
            got_group = group.step_many((0, 1, 2)).clone()
            torch.cuda.synchronize()
            assert torch.equal(got_single, want) and tm.same(tm.snapshot(single), tm.snapshot(eager))
            assert torch.equal(got_group, want) and tm.same(tm.snapshot(group), tm.snapshot(eager)), "step_many is not bitwise the eager steps"
