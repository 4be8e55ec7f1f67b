"""The merged FeatureTransformer backward's d_w1 rider as six bf16 plane products (gemm_tile_bf6t in every
ftm_backward_bf_kernel; NNUE_FTM_BF16=0, read per call, keeps ftm_backward_kernel's f32 rider, which the same cases hold too).
``-m gpu``.  Shapes, operands and references: tests/rider_planes_cases.py.

Every case is one launch of lib.ftm_backward(..., ft=, d_z1=, d_w1=).  d_w1 is an interior view of a NaN-filled buffer whose
bands must stay NaN; ft and d_z1 are interior views of NaN-surrounded buffers, so a read one row past B or past a bucket's end
shows as NaN in d_w1.

  unit   ft = k / 16, d_z1 = k / 64: d_w1 EQUALS the float64 product (the split of such operands is exact and every sum is
         exact in float32 in any order -- asserted on the reference, not assumed).
  randn  against float64 at the bar the f32 rider is held to, conftest.assert_close_grad's 1e-4 of the tensor's largest element.
         The ratio is printed under ``pytest -s``.  A CPU emulation of the split and the term order (exact plane products, one
         float32 rounding per 32-k MFMA) gives 0.9e-7 .. 3.8e-7 at exactly these operands and plain sequential float32
         summation 0.5e-7 .. 7.2e-7: a ratio far above that is a bug even inside the bar, so the six-plane form is also held to
         2e-6 -- 16 float32 roundings (2^-23) of the largest element, about three times what float32 summation itself loses here;
         the dropped terms (mid lo + lo mid + lo lo <= 2^-23 of a product) and the float32 pairwise product lie inside it.
"""
import pytest
import torch

import rider_planes_cases as rc
from conftest import assert_close_grad
from nnue_hip import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
KNOBS = ("default", "f32")
SIX_PLANE_BAR = 2e-6


@pytest.fixture(autouse=True)
def per_call_knobs(monkeypatch, request):
    for knob in ("NNUE_FTM_BF16", "NNUE_FTM_BF_WM", "NNUE_FTM_BF_BM", "NNUE_FTM_VAL_PLANES"):
        monkeypatch.delenv(knob, raising=False)
    if getattr(request.node, "callspec", None) is not None and request.node.callspec.params.get("knob") == "f32":
        monkeypatch.setenv("NNUE_FTM_BF16", "0")


def check_d_w1(got, ref, regime, knob, what, capsys=None):
    assert bool(torch.isfinite(got).all()), f"{what}: a NaN or Inf (a row past the operands' end was read, or an element was not stored)"
    if regime == "unit":
        wrong = got.cpu().double() != ref
        assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} of {ref.numel()} elements differ from float64, first at {wrong.nonzero()[0].tolist()}"
        return
    scale = max(float(ref.abs().max()), 1e-12)
    ratio = float((got.cpu().double() - ref).abs().max()) / scale
    if capsys is not None:
        with capsys.disabled():
            print(f"\n  {what} [{knob}]: max|got - ref| / max|ref| = {ratio:.2e} (bar 1e-04)", end="")
    assert_close_grad(got, ref, what)
    if knob == "default":
        assert ratio <= SIX_PLANE_BAR, f"{what}: {ratio:.2e} is inside the bar but far above the six-plane form's own error"


@pytest.mark.parametrize("regime", ("unit", "randn"))
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_d_w1_against_float64(shape, knob, regime, capsys):
    c = rc.case(shape, regime)
    b, f, p, l1, l2 = rc.geometry(shape)
    assert lib.ftm_backward_cw_supported(b, f, p, l1, l2) and lib.load().nnue_ftm_uses_bf16(2, b, f, p, l1) == int(knob == "default")
    plain = rc.launch(c, rider=False)
    got = rc.launch(c)
    check_d_w1(got["d_w1"], c["ref"], regime, knob, f"d_w1 {rc.shape_id(shape)}", capsys)
    # the launch's other outputs are bitwise those of the call without the rider; a second launch gives bitwise the first
    for k in ("d_w", "d_b", "d_v"):
        assert rc.same_bits(got[k], plain[k]), f"{k} differs from the call without the rider"
    again = rc.launch(c)
    for k in ("d_w1", "d_w", "d_b", "d_v"):
        assert rc.same_bits(again[k], got[k]), f"{k}: a second launch differs"


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("shape", [s for s in rc.SHAPES if s != rc.BIG][::3], ids=rc.shape_id)
def test_rider_beside_the_ste_partials_and_the_squared_norms(shape, knob):
    """sq_partial and ste= together: the partials and sq_partial are bitwise those of the call without the rider."""
    c = rc.case(shape, "randn")
    b, f, p, l1, l2 = rc.geometry(shape)
    # (the STE partials ride only beside the bf16 weight tiles: with NNUE_FTM_BF16=0 the launch has no STE form to compare)
    ste = knob == "default"
    assert ste or lib.ftm_backward_ste_chunks(b, f, p, l1, 3 * shape[2], 3 * shape[3], 3) == 0
    plain = rc.launch(c, rider=False, sq=True, ste=ste)
    got = rc.launch(c, sq=True, ste=ste)
    assert bool(torch.isfinite(plain["sq"]).all()) and (not ste or bool(torch.isfinite(plain["part"]).all()))
    for k in ("part", "sq", "d_w", "d_b", "d_v") if ste else ("sq", "d_w", "d_b", "d_v"):
        assert rc.same_bits(got[k], plain[k]), f"{k} differs from the call without the rider"
    check_d_w1(got["d_w1"], c["ref"], "randn", knob, f"d_w1 {rc.shape_id(shape)} beside the STE ride")
    assert rc.same_bits(got["d_w1"], rc.launch(c)["d_w1"]), "d_w1 differs from the launch without the STE ride"


@pytest.mark.parametrize("regime", ("unit", "randn"))
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("shape", rc.BUCKET_SHAPES, ids=rc.shape_id)
def test_bucketed_rider(shape, knob, regime, capsys):
    """K = 3 stacks over grouped rows 0 / 37 / 37 / 130 (no boundary a multiple of 4, the middle stack empty): d_w1[k] is the
    float64 product over stack k's rows only, d_w1[1] is exact zeros, and rows of the next stack or past the last one (NaN
    here, up to the grouped row count) are never read."""
    c = rc.case(shape, regime)
    b, f, p, l1, l2 = rc.geometry(shape)
    assert b == rc.SEG[-1]
    plan = lib.BucketPlan(b, 3, DEV)
    plan.seg.copy_(torch.tensor(rc.SEG, dtype=torch.int32))
    rows = plan.tiles * 16
    assert rows >= b + 16, "whole tiles of NaN rows lie past the last segment"
    band = rc.Banded()
    grouped = []
    for t in (c["ft"], c["d_z1"]):
        g = band(rows, t.shape[1], of=torch.full((rows, t.shape[1]), float("nan")))
        g[:b].copy_(t)
        grouped.append(g)
    plain = rc.launch(c, rider=False)
    got = rc.launch(c, ft=grouped[0], d_z1=grouped[1], buckets=plan, stacks=3)
    for k in ("d_w", "d_b", "d_v"):
        assert rc.same_bits(got[k], plain[k]), f"{k} differs from the call without the rider"
    for k in range(3):
        lo, hi = rc.SEG[k], rc.SEG[k + 1]
        ref = c["d_z1"][lo:hi].double().t() @ c["l0"][lo:hi]
        check_d_w1(got["d_w1"][k], ref, regime, knob, f"d_w1[{k}] {rc.shape_id(shape)}", capsys)
    assert rc.same_bits(got["d_w1"][1], torch.zeros_like(got["d_w1"][1])), "the empty stack's slab is exact (positive) zeros"
    again = rc.launch(c, ft=grouped[0], d_z1=grouped[1], buckets=plan, stacks=3)
    assert rc.same_bits(again["d_w1"], got["d_w1"])


# ------------------------------------------------------------------ the trainer
def test_three_trainer_steps_at_b160_follow_the_oracle_in_every_launch_form(monkeypatch):
    """The C2 architecture and map at batch 160 (the rider in ftm_backward_bf_kernel<64, 32, 64, 128, false, true, ...>): three
    optimizer steps eagerly, as per-step graphs and through step_many against the float64 oracle at the bars of
    tests/test_gpu_trainer_modes.py (trainer_modes.check_step: logits, loss, norm, gradients, parameters, updates, momentum)."""
    import trainer_modes as tm
    row = tm.Row("c2_b160", cfg=dict(l1=1024, l2=128, l3=32, batch=160))
    tm.set_knobs(monkeypatch, row)
    cfg = row.config
    with tm.trainer_for(cfg, use_graph=False, input_slots=3) as (eager, params):
        assert eager.ride_dw1 and eager.merge_backward
        refs, states = [], []
        for ref in tm.oracle_steps(cfg, params):
            was = {k: v.detach().clone() for k, v in eager.p.items()}
            eager.max_grad_norm = ref["max_grad_norm"]
            loss = eager.step(ref["images"].to(DEV), ref["labels"].to(DEV), slot=ref["step"])
            tm.check_step(eager, ref, was, loss, f"eager step {ref['step']}", {})
            refs.append(ref)
            states.append(tm.snapshot(eager))
        with tm.trainer_for(cfg, use_graph=True, input_slots=3) as (single, _), tm.trainer_for(cfg, use_graph=True, input_slots=3) as (group, _):
            for ref in refs:  # per-step graphs, each held to the oracle and bitwise the eager step
                for tr in (single, group):
                    was = {k: v.detach().clone() for k, v in tr.p.items()}
                    tr.max_grad_norm = ref["max_grad_norm"]
                    loss = tr.step(ref["images"].to(DEV), ref["labels"].to(DEV), slot=ref["step"])
                    tm.check_step(tr, ref, was, loss, f"graph step {ref['step']}", {})
                    assert tm.same(tm.snapshot(tr), states[ref["step"]]), f"graph step {ref['step']} is not bitwise the eager one"
            # the three slots once more: singly, and as one step group
            want = torch.stack([eager.step(slot=s).clone() for s in (0, 1, 2)])
            got_single = torch.stack([single.step(slot=s).clone() for s in (0, 1, 2)])
            got_group = group.step_many((0, 1, 2)).clone()
            torch.cuda.synchronize()
            assert torch.equal(got_single, want) and tm.same(tm.snapshot(single), tm.snapshot(eager))
            assert torch.equal(got_group, want) and tm.same(tm.snapshot(group), tm.snapshot(eager)), "step_many is not bitwise the eager steps"
