"""Adam on the big table without a materialised gradient (include/nnue_hip.h: nnue_adam_step_ext,
nnue_ftm_backward_weight_update_adam, nnue_ftm_backward_weight_update_forward_adam; NnueTrainer(optimizer="adam") with
``fuse_table_update`` / ``fuse_next_forward``): clip_grad_norm_ + torch.optim.Adam (train.py:363-366, :465-471) applied to
the table and its two moments in the epilogue of d_W = A^T d_out, and the same pass also forming the next step's
FeatureTransformer forward (nnue.py:686-710).  ``-m gpu``.

The per-element bound of the parameter checks (``adam_bounds``)
---------------------------------------------------------------
Adam's step is lr * m_hat / (sqrt(v_hat) + eps): where an element's gradient is within rounding of zero it can
legitimately differ by up to 2 lr, so a bar relative to the tensor's maximum is either blind or wrong.  The bound is the
one ``tests/test_gpu_multi_optim.py::Reference.check`` derives, with the constants of ``tests/test_gpu_optim.py``
(U = 2^-24 the float32 unit roundoff, K = 8 roundings per term, NORM_RTOL = 1e-5 on a clipped term whose coefficient was
formed from a float32 norm), fed the float32 state of the step before so that every bound covers one step:

    d       = wd |p_old| + t_g                       t_g = |coef * scale * d_W| in float64
    m_bound = K U (b1 |m_old| + (1 - b1) d) + clip_rtol (1 - b1) t_g + (1 - b1) dg
    v_bound = K U (b2 |v_old| + (1 - b2) d^2) + 2 clip_rtol (1 - b2) d t_g + (1 - b2) dg (2 d + dg)
    p_bound = K U (|p_old| + |p_ref - p_old|) + lr * dir_err(m_bound, v_bound)        (dir_err as in Reference.check)

with ONE allowance that reference does not need, because there the gradient is an input and here it is formed by the
kernel: dg = (B + K) U coef scale (A^T |d_out|), the float32 accumulation of the product over the batch -- B additions
of terms bounded by |d_out| plus the K roundings of the bf16 split and the scaling.  It enters m linearly and v through
|g'^2 - g^2| <= dg (2 |g| + dg).  Nothing here is fitted to an observed error, and no element is left out.
"""
import math
import os

import pytest
import torch

import nnue
import nnue_oracle as orc
from conftest import assert_close_grad
from test_gpu_optim import K, NORM_RTOL, U, assert_within, f32
from test_gpu_step_shapes import SHAPES as STEP_SHAPES, clean_batch
from test_gpu_update_forward import SHAPES, _map, require_fused_pass

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETAS, EPS = (0.9, 0.999), 1e-8


def adam_reference(p_old, m_old, v_old, g, lr, wd, t, betas=BETAS, eps=EPS):
    """float64 torch.optim.Adam arithmetic (L2 weight decay in the gradient, no amsgrad) with the float32 hyper-parameters
    the kernels get; g is the clipped and scaled gradient."""
    lr, wd, eps, (b1, b2) = f32(lr), f32(wd), f32(eps), (f32(betas[0]), f32(betas[1]))
    d = g + wd * p_old
    m = b1 * m_old + (1 - b1) * d
    v = b2 * v_old + (1 - b2) * d * d
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    p = p_old - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adam_bounds(p_old, m_old, v_old, t_g, dg, p_ref, m_ref, v_ref, lr, wd, t, clip_rtol, betas=BETAS, eps=EPS):
    """(m_bound, v_bound, p_bound) of this file's header; every argument float64, element by element."""
    lr, wd, eps, (b1, b2) = f32(lr), f32(wd), f32(eps), (f32(betas[0]), f32(betas[1]))
    d = wd * p_old.abs() + t_g
    m_bound = K * U * (b1 * m_old.abs() + (1 - b1) * d) + clip_rtol * (1 - b1) * t_g + (1 - b1) * dg
    v_bound = K * U * (b2 * v_old.abs() + (1 - b2) * d * d) + 2 * clip_rtol * (1 - b2) * d * t_g + (1 - b2) * dg * (2 * d + dg)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    denom = v_ref.sqrt() / math.sqrt(bc2) + eps
    sqrt_err = torch.where(v_bound > 0, 2 * v_bound / (v_ref.sqrt() + v_bound.sqrt()), torch.zeros_like(v_bound))
    dir_err = (m_bound / bc1 + (m_ref / bc1).abs() * (sqrt_err / math.sqrt(bc2) + K * U * denom) / denom) / denom
    p_bound = K * U * (p_old.abs() + (p_ref - p_old).abs()) + lr * dir_err
    return m_bound, v_bound, p_bound


def _state(gen, f, l1, later):
    """table, exp_avg, exp_avg_sq and the step number: zero moments at step 1, non-zero ones at step 3."""
    weight = (torch.randn(f, l1, generator=gen) * 0.1).to(DEV)
    if not later:
        return weight, torch.zeros(f, l1, device=DEV), torch.zeros(f, l1, device=DEV), 1
    return weight, (torch.randn(f, l1, generator=gen) * 1e-3).to(DEV), (torch.rand(f, l1, generator=gen) * 1e-5).to(DEV), 3


# ---------------------------------------------------------------------------------------------- 1. fused pass = its halves
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("later", [False, True])
@pytest.mark.parametrize("wd", [0.0, 2e-4])
def test_fused_pass_is_bitwise_its_two_halves(shape, later, wd):
    """nnue_ftm_backward_weight_update_forward_adam against nnue_ftm_backward_weight_update_adam + nnue_ftm_forward: table, both
    moments and the next forward bit for bit -- the contract the SGD pass has (tests/test_gpu_update_forward.py)."""
    from nnue_hip import lib
    lib.load()
    b, f, p, l1 = shape[:4]
    bn = shape[4] if len(shape) > 4 else b
    require_fused_pass(lib, b, f, p, l1, bn)
    gen = torch.Generator().manual_seed(b * 7 + f)
    fm, fm_next = _map(lib, gen, b, p, f, l1), _map(lib, gen, bn, p, f, l1, density=0.3)
    d_out = (torch.randn(b, l1, generator=gen) * 0.05).to(DEV)
    weight, m0, v0, t = _state(gen, f, l1, later)
    bias = torch.randn(l1, generator=gen).to(DEV)
    coef = torch.tensor([0.37], device=DEV)
    lr_dev = torch.tensor([2e-3], device=DEV)
    counter = torch.tensor([t], dtype=torch.int32, device=DEV)
    direct = min(f - 1, p)

    w_ref, m_ref, v_ref = weight.clone(), m0.clone(), v0.clone()
    lib.ftm_backward_weight_update_adam(d_out, fm, w_ref, m_ref[:direct], v_ref[:direct], coef, counter, 0.5, BETAS, EPS, wd, 1.0 / b,
                                        lr_dev=lr_dev)
    out_ref = lib.ftm_forward(w_ref, bias, fm_next)
    torch.cuda.synchronize()

    w_got, m_got, v_got = weight.clone(), m0.clone(), v0.clone()
    out_got = torch.full((bn, l1), float("nan"), device=DEV)
    fm_next.scratch.zero_()
    lib.ftm_backward_weight_update_forward_adam(d_out, fm, w_got, m_got[:direct], v_got[:direct], coef, counter, 0.5, BETAS, EPS, wd,
                                                1.0 / b, fm_next, bias, out_got, lr_dev=lr_dev)
    torch.cuda.synchronize()
    assert int(counter) == t, "the update reads the step counter, it does not advance it"
    assert torch.equal(w_got, w_ref), f"table differs: max |d| = {(w_got - w_ref).abs().max().item():.3e}"
    assert torch.equal(m_got, m_ref), "exp_avg differs"
    assert torch.equal(v_got, v_ref), "exp_avg_sq differs"
    assert torch.equal(out_got, out_ref), f"next forward differs: max |d| = {(out_got - out_ref).abs().max().item():.3e}"
    assert not torch.equal(w_got[:direct], weight[:direct])  # it did move
    # rows the product does not cover are nobody's here (the flat optimizer pass owns them)
    assert torch.equal(w_got[direct:], weight[direct:]) and torch.equal(m_got[direct:], m0[direct:]) and torch.equal(v_got[direct:], v0[direct:])


# ---------------------------------------------------------------------------------------------- 2. epilogue against float64
def test_epilogue_against_float64():
    """One call with non-zero moments at step 3 against float64 g = coef scale A^T d_out + wd w and torch's Adam formulas:
    moments at the project's gradient bar, the table element by element within ``adam_bounds``."""
    from nnue_hip import lib
    lib.load()
    b, f, p, l1 = 128, 8192, 8192, 256
    gen = torch.Generator().manual_seed(11)
    fm = _map(lib, gen, b, p, f, l1)
    d_out = (torch.randn(b, l1, generator=gen) * 0.05).to(DEV)
    weight, m, v, t = _state(gen, f, l1, later=True)
    coef, lr, wd, scale = 0.8, 1e-3, 2e-4, 1.0 / b
    direct = f - 1
    p_old, m_old, v_old = (x[:direct].cpu().double() for x in (weight, m, v))
    A = fm.bits.cpu().double()[:, :direct]
    cs = float(f32(coef)) * float(f32(scale))
    g = cs * (A.T @ d_out.cpu().double())
    dg = (b + K) * U * cs * (A.T @ d_out.cpu().double().abs())
    p_ref, m_ref, v_ref = adam_reference(p_old, m_old, v_old, g, lr, wd, t)
    tail = [x[direct:].clone() for x in (weight, m, v)]
    lib.ftm_backward_weight_update_adam(d_out, fm, weight, m[:direct], v[:direct], torch.tensor([coef], device=DEV),
                                        torch.tensor([t], dtype=torch.int32, device=DEV), lr, BETAS, EPS, wd, scale)
    torch.cuda.synchronize()
    assert_close_grad(m[:direct], m_ref.float(), "exp_avg")
    assert_close_grad(v[:direct], v_ref.float(), "exp_avg_sq")
    m_bound, v_bound, p_bound = adam_bounds(p_old, m_old, v_old, g.abs(), dg, p_ref, m_ref, v_ref, lr, wd, t, clip_rtol=0.0)
    err = (weight[:direct].cpu().double() - p_ref).abs()
    print(f"table: max err {float(err.max()):.3e}, max err / bound {float((err / p_bound).max()):.3f}, "
          f"largest bound {float(p_bound.max()):.3e} (lr {lr:g})")
    assert_within(weight[:direct], p_ref, p_bound, "table")
    assert_within(m[:direct], m_ref, m_bound, "exp_avg (element by element)")
    assert_within(v[:direct], v_ref, v_bound, "exp_avg_sq (element by element)")
    for got, was in zip((weight, m, v), tail):
        assert torch.equal(got[direct:], was), "a row the product does not cover was touched"


# ---------------------------------------------------------------------------------------------- 3. trainer: fused vs materialised
def test_trainer_fused_update_against_the_materialised_path(monkeypatch):
    """tests/test_gpu_ftm.py::test_table_update_in_the_product_epilogue_equals_the_materialised_path with optimizer="adam":
    three steps, clip active, weight decay on.  The two trainers start every step from the materialised trainer's state, so
    each step's update is checked on its own: norms within 2e-6 of each other, moments at the 1e-5 bar, and every parameter
    within ``adam_bounds`` of float64 Adam on the MATERIALISED gradient (clip_rtol = NORM_RTOL: the clip is active).  That
    gradient is itself a float32 product over the batch, so the table's allowance dg is taken twice: once for the product
    inside the fused epilogue, once for the one the reference is computed from."""
    if os.environ.get("NNUE_FT_PATH", "auto") not in ("auto", "mfma"):
        pytest.skip("another FeatureTransformer kernel family is forced (NNUE_FT_PATH)")
    from nnue_hip.trainer import NnueTrainer
    B, lr, wd, max_norm = 96, 0.05, 1e-3, 0.5
    trs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("NNUE_FUSE_TABLE_UPDATE", mode)
        torch.manual_seed(4)
        model = nnue.NNUE(nnue.GridFeatureSet(16, 16), 256, 32, 16, num_classes=10, input_size=64).to(DEV)
        tr = NnueTrainer(model, B, (64, 64), lr=lr, weight_decay=wd, max_grad_norm=max_norm, use_graph=True, optimizer="adam")
        assert tr.fuse_table_update == (mode == "1") and tr.grads_materialised == (mode == "0")
        trs[mode] = tr
    fused, mat = trs["1"], trs["0"]
    lo, hi = fused.sq_range
    gen = torch.Generator().manual_seed(8)
    for s in range(3):
        for dst, src in ((fused.flat_params, mat.flat_params), (fused.flat_exp_avg, mat.flat_exp_avg),
                         (fused.flat_exp_avg_sq, mat.flat_exp_avg_sq), (fused.adam_step_count, mat.adam_step_count)):
            dst.copy_(src)
        p_old, m_old, v_old = (x.cpu().double() for x in (mat.flat_params, mat.flat_exp_avg, mat.flat_exp_avg_sq))
        images, labels = torch.randn(B, 3, 64, 64, generator=gen).to(DEV), torch.randint(0, 10, (B,), generator=gen).to(DEV)
        fused.step(images, labels)
        mat.step(images, labels)
        torch.cuda.synchronize()
        a, b_ = float(fused.grad_norm), float(mat.grad_norm)
        assert abs(a - b_) <= 2e-6 * b_ and b_ > max_norm, (s, a, b_)  # the clip is active
        assert int(fused.adam_step_count) == int(mat.adam_step_count) == s + 1
        g_mat = mat.flat_grads.cpu().double()
        norm = float(torch.linalg.vector_norm(g_mat))
        assert abs(b_ - norm) <= NORM_RTOL * norm
        coef = min(max_norm / (norm + 1e-6), 1.0)
        p_ref, m_ref, v_ref = adam_reference(p_old, m_old, v_old, coef * g_mat, lr, wd, s + 1)
        dg = torch.zeros_like(p_old)
        A = fused.fm.bits.cpu().double()[:, :(hi - lo) // fused.L1]
        dg[lo:hi] = (2 * (B + K) * U * coef * (A.T @ fused.d_ft.cpu().double().abs())).reshape(-1)
        m_bound, v_bound, p_bound = adam_bounds(p_old, m_old, v_old, (coef * g_mat).abs(), dg, p_ref, m_ref, v_ref, lr, wd, s + 1,
                                                clip_rtol=NORM_RTOL)
        assert_within(fused.flat_params, p_ref, p_bound, f"step {s}: parameters of the fused path")
        assert_within(mat.flat_params, p_ref, p_bound, f"step {s}: parameters of the materialised path")
        assert_close_grad(fused.flat_exp_avg, mat.flat_exp_avg, f"step {s}: exp_avg", rtol=1e-5)
        assert_close_grad(fused.flat_exp_avg_sq, mat.flat_exp_avg_sq, f"step {s}: exp_avg_sq", rtol=1e-5)
        assert not torch.equal(fused.flat_params[lo:hi], p_old[lo:hi].float().to(DEV))  # the table did move
        assert float(fused.flat_grads[lo:hi].abs().max()) == 0.0  # ... and its gradient was never written


# ---------------------------------------------------------------------------------------------- 4. step group = single steps
def _bigtable_pair(monkeypatch, **opt):
    from nnue_hip.trainer import NnueTrainer
    monkeypatch.setenv("NNUE_FUSE_TABLE_UPDATE", "1")  # (auto: tables of 32 MB or more; this one has 8 MB)
    monkeypatch.setenv("NNUE_FUSE_NEXT_FORWARD", "1")
    grid, hw, l1 = nnue.GridFeatureSet(16, 32), 64, 256
    torch.manual_seed(0)
    model = nnue.NNUE(grid, l1, 32, 16, num_classes=10, input_size=64).to(DEV)
    twin = nnue.NNUE(grid, l1, 32, 16, num_classes=10, input_size=64).to(DEV)
    twin.load_state_dict(model.state_dict())
    tr = NnueTrainer(model, 64, (hw, hw), **opt)
    if not tr.fuse_next_forward and os.environ.get("NNUE_FTM_BF16") == "0":
        pytest.skip("a developer knob took the forward off the bf16-split 64-deep tiles the fused pass is built on")
    assert tr.fuse_table_update and tr.fuse_next_forward and not tr.grads_materialised
    monkeypatch.setenv("NNUE_FUSE_NEXT_FORWARD", "0")
    ref = NnueTrainer(twin, 64, (hw, hw), **opt)
    assert ref.fuse_table_update and not ref.fuse_next_forward
    gen = torch.Generator().manual_seed(5)
    data = [(torch.randn(64, 3, hw, hw, generator=gen).to(DEV), torch.randint(0, 10, (64,), generator=gen).to(DEV)) for _ in range(3)]
    for t in (tr, ref):
        for (im, lb), (ti, tl) in zip(data, t.inputs):
            ti.copy_(im)
            tl.copy_(lb)
    return tr, ref


def _same_state(tr, ref):
    return (torch.equal(tr.flat_params, ref.flat_params) and torch.equal(tr.flat_exp_avg, ref.flat_exp_avg)
            and torch.equal(tr.flat_exp_avg_sq, ref.flat_exp_avg_sq))


def test_step_group_at_the_big_table_is_the_single_steps(monkeypatch):
    """The "bigtable" case of tests/test_gpu_trainer.py::test_step_many_is_the_same_steps_in_one_graph for Adam: inside a
    group the table update also forms the next forward (two alternating maps), bitwise the same steps taken singly with
    NNUE_FUSE_NEXT_FORWARD=0 -- parameters, both moments, losses -- over an odd and an even group, and run to run."""
    opt = dict(lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, input_slots=3, use_graph=True, optimizer="adam")
    runs = []
    for rep in range(2):
        tr, ref = _bigtable_pair(monkeypatch, **opt)
        order = (0, 1, 2, 1, 0)
        first = tr.step_many(order[:2])  # before anything is recorded: falls back to single steps
        want = [ref.step(slot=s).clone() for s in order[:2]]
        assert torch.equal(first, torch.stack(want))
        steps = 2
        for group in (order, order[:4], order):  # odd, even (ends on the second map), odd again
            got = tr.step_many(group).clone()
            want = torch.stack([ref.step(slot=s).clone() for s in group])
            steps += len(group)
            assert torch.equal(got, want), (group, got, want)
            assert _same_state(tr, ref), group
            assert int(tr.adam_step_count) == int(ref.adam_step_count) == steps == tr.steps_done
        assert (order, "many") in tr._g_local and (order[:4], "many") in tr._g_local
        assert tr.active_stats() == ref.active_stats()
        assert torch.equal(tr.step(slot=2), ref.step(slot=2)) and _same_state(tr, ref)  # a single step after an even group
        timers = {"nnue_ftm_backward_weight_update_forward_adam": [], "nnue_ftm_backward_weight_update_adam": [], "nnue_ftm_forward": []}
        got = tr.step_many(order, timers=timers).clone()  # the same launches eagerly, with events
        want = torch.stack([ref.step(slot=s).clone() for s in order])
        assert torch.equal(got, want) and _same_state(tr, ref)
        assert len(timers["nnue_ftm_backward_weight_update_forward_adam"]) == len(order) - 1
        assert len(timers["nnue_ftm_backward_weight_update_adam"]) == 1 and len(timers["nnue_ftm_forward"]) == 1
        runs.append((tr.flat_params.clone(), tr.flat_exp_avg.clone(), tr.flat_exp_avg_sq.clone(), got))
        del tr, ref
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_), "not reproducible run to run"


# ---------------------------------------------------------------------------------------------- 5. against the oracle at C4
def test_a_step_group_at_the_224_shape_follows_the_oracle_with_adam():
    """BASELINE configs[3]'s shape with the reference's other optimizer (config/train_nnue_test.py: Adam): one single step
    (records the plans), then a group of three replayed as one graph, against oracle.loss_and_grads_explicit +
    oracle.adam_step; batches by tests/test_gpu_step_shapes.py::clean_batch (samples near a discontinuity are redrawn, the
    batch keeps its 128 rows); parameters on the update scale, as tests/test_oracle_golden.py::test_adam_steps_match_reference."""
    from nnue_hip.trainer import NnueTrainer
    cfg = STEP_SHAPES["c4"]
    opt = dict(lr=1e-3, weight_decay=2e-4, max_grad_norm=1.0)
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(cfg["grid"], cfg["fps"]), cfg["l1"], cfg["l2"], cfg["l3"], num_classes=cfg["classes"],
                      input_size=cfg["image"])
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    stride = orc.conv_stride(cfg["image"], cfg["grid"])
    tr = NnueTrainer(model.to(DEV), cfg["batch"], (cfg["image"], cfg["image"]), use_graph=True, input_slots=3, optimizer="adam", **opt)
    if not tr.fuse_next_forward:
        assert os.environ.get("NNUE_FUSE_NEXT_FORWARD") == "0" or os.environ.get("NNUE_FUSE_TABLE_UPDATE") == "0" \
            or os.environ.get("NNUE_FT_PATH", "auto") not in ("auto", "mfma") or os.environ.get("NNUE_FTM_BF16") == "0", \
            "the 224x224 shape must take the fused pass by default"
        pytest.skip("a knob switched the fused update + next forward off")
    assert tr.fuse_table_update and not tr.grads_materialised
    gen = torch.Generator().manual_seed(79)
    state, ref_losses, ref_norms = {}, [], []
    for s in range(4):
        images, labels = clean_batch(cfg, params, stride, gen)
        assert images.shape[0] == cfg["batch"]
        _, ref_loss, ref_grads, keep = orc.loss_and_grads_explicit(params, images, labels, stride, None)
        ref_norms.append(float(orc.adam_step(params, ref_grads, state, opt["lr"], opt["weight_decay"], opt["max_grad_norm"])))
        ref_losses.append(float(ref_loss))
        if s == 0:
            first = tr.step(images.to(DEV), labels.to(DEV), slot=0)
            assert abs(float(first) - ref_losses[0]) <= 1e-4 * max(1.0, abs(ref_losses[0]))
            assert abs(float(tr.grad_norm) - ref_norms[0]) <= 1e-4 * ref_norms[0]
            for k in orc.TRAINABLE_KEYS:
                err = float((tr.p[k].cpu() - params[k]).abs().max())
                assert err <= 2e-5 + 1e-4 * float(params[k].abs().max()), f"first step {k}: {err:.3e}"
        else:
            tr.inputs[s - 1][0].copy_(images)
            tr.inputs[s - 1][1].copy_(labels)
    losses = tr.step_many((0, 1, 2))
    torch.cuda.synchronize()
    assert (((0, 1, 2), "many") in tr._g_local) and tr.steps_done == 4 and int(tr.adam_step_count) == 4
    for s in range(3):
        assert abs(float(losses[s]) - ref_losses[s + 1]) <= 1e-4 * max(1.0, abs(ref_losses[s + 1])), (s, float(losses[s]), ref_losses[s + 1])
    assert abs(float(tr.grad_norm) - ref_norms[3]) <= 1e-4 * ref_norms[3]
    n_mean, n_max = tr.active_stats()
    assert n_max == int(keep["n"].max()) and abs(n_mean - float(keep["n"].float().mean())) < 1e-2
    for k in orc.TRAINABLE_KEYS:
        # Adam divides by sqrt(v): an element whose gradient is ~0 amplifies rounding, so compare on the update scale
        err = float((tr.p[k].cpu() - params[k]).abs().max())
        print(f"{k}: max err {err:.3e} (bar {2e-5 + 1e-4 * float(params[k].abs().max()):.3e})")
        assert err <= 2e-5 + 1e-4 * float(params[k].abs().max()), f"after the group: {k}: {err:.3e}"
        views = tr.layout.views(tr.flat_exp_avg)[k], tr.layout.views(tr.flat_exp_avg_sq)[k]
        assert_close_grad(views[0], state[k]["m"], f"exp_avg of {k}")
        assert_close_grad(views[1], state[k]["v"], f"exp_avg_sq of {k}")


# ---------------------------------------------------------------------------------------------- 6. state hand-over, schedule
def test_state_hand_over_and_learning_rate_schedule(monkeypatch):
    """optimizer_state_dict() of the fused trainer loads into torch.optim.Adam with the table's step / exp_avg / exp_avg_sq equal
    to the flat buffers; ``trainer.lr = x`` between replays changes the update without adding or dropping a graph."""
    opt = dict(lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, input_slots=3, use_graph=True, optimizer="adam")
    tr, ref = _bigtable_pair(monkeypatch, **opt)
    tr.step(slot=0), ref.step(slot=0)
    group = (1, 2, 0)
    tr.step_many(group)
    for s in group:
        ref.step(slot=s)
    assert _same_state(tr, ref)
    graphs = set(tr._g_local)
    before = tr.flat_params.clone()
    tr.step_many(group)
    d_small = (tr.flat_params - before).abs().mean()
    tr.lr = 8e-3
    assert float(tr.lr_dev) == pytest.approx(8e-3)
    before = tr.flat_params.clone()
    tr.step_many(group)
    d_big = (tr.flat_params - before).abs().mean()
    assert set(tr._g_local) == graphs, "changing the learning rate must not drop or add graphs"
    for i, s in enumerate(group * 2):
        ref.lr = 1e-3 if i < 3 else 8e-3
        ref.step(slot=s)
    assert _same_state(tr, ref), "the group under a schedule is not the single steps under the same schedule"
    assert float(d_big) > 4 * float(d_small), (float(d_big), float(d_small))  # Adam's step scales with the rate: 8x here
    torch.cuda.synchronize()
    sd = tr.optimizer_state_dict()
    torch_opt = torch.optim.Adam(tr.model.parameters(), lr=tr.lr, betas=tr.betas, eps=tr.eps, weight_decay=tr.weight_decay)
    torch_opt.load_state_dict(sd)
    st = torch_opt.state[tr.model.input.weight]
    assert float(st["step"]) == tr.steps_done == int(tr.adam_step_count) == 10
    assert torch.equal(st["exp_avg"], tr.layout.views(tr.flat_exp_avg)["input.weight"])
    assert torch.equal(st["exp_avg_sq"], tr.layout.views(tr.flat_exp_avg_sq)["input.weight"])
    assert float(st["exp_avg_sq"].min()) >= 0.0 and float(st["exp_avg"].abs().max()) > 0.0
    for k, prm in tr.model.named_parameters():
        if k != "nnue2score":
            assert torch.equal(torch_opt.state[prm]["exp_avg"], tr.layout.views(tr.flat_exp_avg)[k]), k
