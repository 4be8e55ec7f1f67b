"""The loss, metric and optimizer kernels (optim_kernels.hip) at every launch form, against float64 torch on the CPU fed
exactly the float32 inputs each kernel got: clip_grad_norm_ + torch.optim.SGD / torch.optim.Adam, F.cross_entropy, and
numpy.argmax for the confusion matrix.  Torch's own optimizers, not the oracle, so that the two cannot share a mistake.
``-m gpu``.

Chained steps feed every reference step the kernel's own state (parameters, momentum, moments) of the step before, so
each bound covers one step's rounding and errors never compound.

Bounds, element by element (never against a tensor's maximum, so a skipped or doubly applied element fails even where its
update is tiny).  U is the float32 unit roundoff.
* An updated element goes through a handful of float32 roundings (g * clip * scale, the weight-decay fma, the momentum fma,
  lr * d, the subtraction; for Adam the moment fmas, sqrt, the bias-correction products and the division): K = 8 of
  them bound each term it is formed from, taken in absolute value, so a cancellation between terms cannot tighten the
  bound below what rounding the terms themselves allows.
  - SGD: m_new within K U (|momentum m_old| + |wd p_old| + |coef s g|); p_new within K U |p_old| + lr * (that bound);
    the update p_new - p_old within 2 U |p_ref| (the one rounding of the stored parameter) + lr * (that bound).
  - Adam: m within K U (|beta1 m_old| + |(1 - beta1) d|), v within K U (|beta2 v_old| + |(1 - beta2) d^2|), with
    d = |wd p_old| + |coef s g|; the parameter and its update by the same route, through the error those moments carry
    into m_hat / (sqrt(v_hat) + eps).
* NORM_RTOL: the norm against float64.  The kernels sum squares in float32 per partial (at most ~100 sequential
  additions per thread at these shapes, then a wave and a block reduction) and the partials in double: 1e-5 relative,
  the bar the rest of the suite uses.  Where clipping is active, the coefficient max_norm / norm carries the same relative
  error into every clipped gradient term, so that term gets NORM_RTOL on top of K U.
* Cross-entropy: the per-sample loss and the mean within 1e-5 * max(1, |ref|) (the existing bar); each d_logits element
  within 1e-5 * (softmax + onehot) * grad_scale / B: the exponent's rounding (|z - max| <= 88 where a term is not
  underflowed), expf, and the sum of up to 64 terms per lane plus the wave reduction; plus 2^-126 absolute, below which
  float32 has no normal numbers.
* The confusion matrix is compared exactly.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nnue_hip import lib as hip

pytestmark = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
K = 8
NORM_RTOL = 1e-5
CE_RTOL = 1e-5
CE_FLOOR = 2.0 ** -126  # float32's smallest normal: below it a probability or gradient may be denormal or flushed


def f32(x: float) -> float:
    return float(np.float32(x))


def dev_buf(src: torch.Tensor, offset: int = 0) -> torch.Tensor:
    """A device copy of src that starts `offset` floats into its own allocation (offset 1: 4-byte aligned only)."""
    base = torch.zeros(src.numel() + offset, device=DEV)
    out = base[offset:]
    out.copy_(src.reshape(-1))
    return out.view(src.shape)


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound element by element; NaNs must sit exactly where the reference has them, infinities must equal."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).cpu()
    bound = bound.reshape(-1) if bound.numel() == ref.numel() else bound.expand_as(ref)
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(nan_g, nan_r), f"{what}: NaN pattern differs at {int((nan_g != nan_r).sum())} of {ref.numel()} elements"
    err = (got - ref).abs()
    bad = ~nan_r & (got != ref) & ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements outside the bound; first at {i}: "
                             f"got {float(got[i])!r} ref {float(ref[i])!r} bound {float(bound[i]):.3e}")


def assert_norm(got, ref, what="norm"):
    if math.isnan(ref):
        assert math.isnan(got), f"{what}: {got} where the reference is NaN"
    elif math.isinf(ref):
        assert got == ref, f"{what}: {got} vs {ref}"
    else:
        assert abs(got - ref) <= NORM_RTOL * ref, f"{what}: {got} vs float64 {ref}"


# ------------------------------------------------------------------------------------------------- references
def clip_reference(p, max_norm):
    """torch.nn.utils.clip_grad_norm_ on p.grad (float64) -> (norm, coefficient torch applied: 1 without clipping)."""
    norm = torch.linalg.vector_norm(p.grad)
    if max_norm > 0:
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        torch.nn.utils.clip_grad_norm_([p], max_norm, foreach=False)
    else:
        coef = torch.ones((), dtype=torch.float64)
    return float(norm), float(coef)


def torch_sgd(p_old, g, m_old, lr, momentum, wd, max_norm, scale, first):
    """clip_grad_norm_ + torch.optim.SGD(momentum, weight_decay) in float64 on the kernel's float32 inputs; with the
    per-element bounds of the header."""
    lr, momentum, wd, max_norm, scale = f32(lr), f32(momentum), f32(wd), f32(max_norm), f32(scale)
    p_old = p_old.cpu().double()
    p = torch.nn.Parameter(p_old.clone())
    p.grad = g.cpu().double() * scale
    norm, coef = clip_reference(p, max_norm)
    t_g = p.grad.abs()
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=wd, foreach=False)
    has_buf = momentum != 0.0 and not first
    t_rest = wd * p_old.abs()
    if has_buf:
        m_old = m_old.cpu().double()
        opt.state[p]["momentum_buffer"] = m_old.clone()
        t_rest = t_rest + momentum * m_old.abs()
    opt.step()
    buf = opt.state[p].get("momentum_buffer") if momentum != 0.0 else None
    clip_rtol = NORM_RTOL if coef < 1.0 else 0.0
    m_bound = K * U * (t_rest + t_g) + clip_rtol * t_g
    p_new = p.detach()
    return dict(p=p_new, m=buf, norm=norm, coef=coef, m_bound=m_bound, p_bound=K * U * p_old.abs() + lr * m_bound,
                upd_bound=2 * U * p_new.abs() + lr * m_bound, p_old=p_old)


def check_sgd(what, p, m, r, m_old=None, sel=slice(None)):
    """p, m: the kernel's results; r: torch_sgd's; sel: the elements this launch updates."""
    p = p.detach().cpu().double()[sel]
    assert_within(p, r["p"][sel], r["p_bound"][sel], f"{what}: parameters")
    assert_within(p - r["p_old"][sel], r["p"][sel] - r["p_old"][sel], r["upd_bound"][sel], f"{what}: update")
    if r["m"] is not None:
        assert_within(m.detach().cpu()[sel], r["m"][sel], r["m_bound"][sel], f"{what}: momentum")
    elif m is not None:  # momentum 0: the buffer is not the kernel's to touch
        assert torch.equal(m.detach().cpu(), m_old.cpu()), f"{what}: momentum buffer written with momentum 0"


def sgd_gpu(p, g, m, lr, momentum, wd, max_norm, scale, first, want_norm=True, **kw):
    scratch = torch.empty((hip.sgd_scratch_bytes(p.numel()),), dtype=torch.uint8, device=DEV)
    norm = torch.full((), float("nan"), device=DEV) if want_norm else None
    hip.sgd_step(p, g, m, lr, momentum, wd, max_norm, scale, first, norm, scratch, **kw)
    torch.cuda.synchronize()
    return None if norm is None else float(norm)


def grads_of(count, amp, gen):
    """randn gradient of norm ~amp (element 0 set to amp: the norm is at least amp whatever the draw)."""
    g = torch.randn(count, generator=gen) * (amp / math.sqrt(count))
    g[0] = amp
    return g


# ------------------------------------------------------------------------------------------------- SGD
# (count, offset floats into the allocation); the launch form by nnue_sgd_step's rule: the float4 kernel when count % 4 == 0,
# the pointers are 16-byte aligned and live <= 16M elements; otherwise the scalar kernel.  nb = norm workgroups.
SGD_SHAPES = [
    (4, 0),         # vector: one float4, nb = 64
    (64, 0),        # vector
    (262144, 0),    # vector: the last count with nb = 64
    (262148, 0),    # vector: nb = 65
    (4194304, 0),   # vector: nb = 1024 reached
    (4194308, 0),   # vector: nb = 1024 (clamped); the apply grid clamped at 2048, passes beyond the prefetched two
    (1, 0),         # scalar: count % 4 != 0
    (3, 0),         # scalar
    (4097, 0),      # scalar
    (4096, 1),      # scalar: count % 4 == 0 but the slice starts one float in (misaligned)
    (16777220, 0),  # scalar: live > 16M on size alone (count % 4 == 0, aligned); grid-stride beyond the prefetch
]
# (first_step, gradient amplitude, max_norm, norm requested, grad_scale) of the chained steps
SGD_STEPS = (
    (True, 50.0, 1.0, True, 1.0),     # clip active; momentum buffer started
    (False, 1e-3, 1.0, True, 0.5),    # clip inactive; grad_scale
    (False, 1.0, 0.0, False, 1.0),    # max_norm == 0 and no norm requested: no norm launch
    (True, 50.0, 2.0, True, 0.3),     # momentum restarted; clip active; a grad_scale that is not a power of two
)


def _sgd_cases():
    for count, off in SGD_SHAPES:
        for momentum in (0.0, 0.9):
            for wd in (0.0, 2e-4):
                if count > 4194308 and (momentum, wd) != (0.9, 2e-4):
                    continue  # the 16.8M buffer once: host memory and time
                yield count, off, momentum, wd


@pytest.mark.parametrize("count,off,momentum,wd", list(_sgd_cases()))
def test_sgd_step_chain(count, off, momentum, wd):
    gen = torch.Generator().manual_seed(count + off)
    p = dev_buf(torch.randn(count, generator=gen), off)
    m = dev_buf(torch.randn(count, generator=gen), off)  # momentum 0: passed anyway, must stay untouched
    lr = 0.05
    for s, (first, amp, max_norm, want_norm, scale) in enumerate(SGD_STEPS):
        g = grads_of(count, amp, gen)
        p_old, m_old = p.cpu(), m.cpu()
        r = torch_sgd(p_old, g, m_old, lr, momentum, wd, max_norm, scale, first)
        if max_norm > 0:
            assert (r["coef"] < 1.0) == (amp > 1.0), "the step does not reach the clip state it is meant to test"
        norm = sgd_gpu(p, dev_buf(g, off), m, lr, momentum, wd, max_norm, scale, first, want_norm)
        if want_norm:
            assert_norm(norm, r["norm"], f"step {s} norm")
        check_sgd(f"step {s}", p, m, r, m_old)
        del r


@pytest.mark.parametrize("count,off", [(4096, 0), (4097, 0), (4096, 1)])  # vector / scalar / scalar (misaligned)
def test_sgd_learning_rate_on_device(count, off):
    gen = torch.Generator().manual_seed(7 + count)
    p = dev_buf(torch.randn(count, generator=gen), off)
    m = dev_buf(torch.randn(count, generator=gen), off)
    g = grads_of(count, 5.0, gen)
    lr_dev = torch.tensor([0.0123], device=DEV)
    r = torch_sgd(p.cpu(), g, m.cpu(), 0.0123, 0.9, 1e-3, 1.0, 1.0, False)
    sgd_gpu(p, dev_buf(g, off), m, 0.5, 0.9, 1e-3, 1.0, 1.0, False, lr_dev=lr_dev)  # the device value wins over lr = 0.5
    check_sgd("lr_dev", p, m, r)


# ext = (partials, lo, hi): a producer's sums of squares of grads[lo:hi], built as the trainer does (nnue_sqnorm_partials)
@pytest.mark.parametrize("count,lo,hi", [
    (10000, 0, 4000), (10000, 4000, 8000), (10000, 8000, 10000),   # vector apply
    (10002, 0, 4000), (10002, 4000, 8000), (10002, 8000, 10002),   # scalar apply; hi == count with count % 4 != 0
])
def test_sgd_producer_partials(count, lo, hi):
    gen = torch.Generator().manual_seed(count + lo)
    p, m = dev_buf(torch.randn(count, generator=gen)), dev_buf(torch.randn(count, generator=gen))
    g = grads_of(count, 20.0, gen)
    gd = dev_buf(g)
    partial = torch.full((37,), float("nan"), device=DEV)
    hip.sqnorm_partials(gd[lo:hi], partial)
    r = torch_sgd(p.cpu(), g, m.cpu(), 0.05, 0.9, 2e-4, 1.0, 0.5, False)
    assert r["coef"] < 1.0
    norm = sgd_gpu(p, gd, m, 0.05, 0.9, 2e-4, 1.0, 0.5, False, ext=(partial, lo, hi))
    assert_norm(norm, r["norm"])
    check_sgd(f"ext [{lo}, {hi})", p, m, r)


def _hole_step(count, lo, hi, g, gen):
    """ext_applied_elsewhere: the producer applies [lo, hi) itself with coef_out; this launch updates the rest."""
    p, m = dev_buf(torch.randn(count, generator=gen)), dev_buf(torch.randn(count, generator=gen))
    p_old, m_old = p.cpu(), m.cpu()
    gd = dev_buf(g)
    partial = torch.full((16,), float("nan"), device=DEV)
    hip.sqnorm_partials(gd[lo:hi], partial)
    coef = torch.full((), float("nan"), device=DEV)
    norm = sgd_gpu(p, gd, m, 0.05, 0.9, 2e-4, 1.0, 0.5, False, ext=(partial, lo, hi), coef_out=coef, ext_applied_elsewhere=True)
    r = torch_sgd(p_old, g, m_old, 0.05, 0.9, 2e-4, 1.0, 0.5, False)
    # the hole keeps its bits
    assert torch.equal(p.cpu()[lo:hi].view(torch.int32), p_old[lo:hi].view(torch.int32)), "parameters in the hole changed"
    assert torch.equal(m.cpu()[lo:hi].view(torch.int32), m_old[lo:hi].view(torch.int32)), "momentum in the hole changed"
    return p, m, r, norm, float(coef)


@pytest.mark.parametrize("count,lo,hi", [
    (10000, 0, 4000), (10000, 4000, 8000), (10000, 8000, 10000), (10000, 0, 10000),   # vector apply; the last: live == 0
    (10002, 0, 4000), (10002, 4000, 8000), (10002, 8000, 10002), (10002, 0, 10002),   # scalar apply; the last: live == 0
])
def test_sgd_hole_applied_elsewhere(count, lo, hi):
    gen = torch.Generator().manual_seed(count + lo + hi)
    g = grads_of(count, 20.0, gen)
    p, m, r, norm, coef = _hole_step(count, lo, hi, g, gen)
    assert r["coef"] < 1.0
    assert_norm(norm, r["norm"])
    assert abs(coef - r["coef"]) <= (NORM_RTOL + K * U) * r["coef"], f"coef_out {coef} vs torch {r['coef']}"
    live = torch.ones(count, dtype=torch.bool)
    live[lo:hi] = False
    check_sgd(f"hole [{lo}, {hi})", p, m, r, sel=live)


def test_sgd_ste_ride_with_producer_partials():
    """The deferred STE second stage riding in the norm launch (ste=) together with a producer's partials (ext=) behind it:
    the combination the trainer forms; against float64 SGD on the gradients the plain STE backward writes."""
    b, h, w, fps, stride = 7, 40, 40, 3, 4
    gen = torch.Generator().manual_seed(99)
    images = dev_buf(torch.randn(b, 3, h, w, generator=gen))
    gh, gw = hip.conv_out_hw(h, w, stride)
    conv_out = dev_buf(torch.randn(b, fps, gh, gw, generator=gen))
    thr = dev_buf(torch.randn(fps, generator=gen) * 0.1)
    d_conv = dev_buf(torch.randn(b, fps, gh, gw, generator=gen) / b)
    n_thr, n_w = (fps + 3) // 4 * 4, (fps * 27 + 3) // 4 * 4
    count = n_thr + n_w + 4096 + 4
    lo, hi = n_thr + n_w, n_thr + n_w + 4096
    base = torch.zeros(count)
    base[lo:] = torch.randn(count - lo, generator=gen)
    p0, m0 = torch.randn(count, generator=gen), torch.randn(count, generator=gen)
    chunks = hip.ste_conv_backward_chunks(b, fps, gh, gw)
    scratch_bytes = max(16, hip.load().nnue_ste_conv_backward_scratch(b, fps, gh, gw))

    def heads(grads):
        return grads[:fps], grads[n_thr:n_thr + fps * 27].view(fps, 3, 3, 3)

    plain = dev_buf(base)
    d_thr, d_w = heads(plain)
    hip.ste_conv_backward(images, conv_out, thr, d_conv, stride, d_thr=d_thr, d_weight=d_w,
                          scratch=torch.empty((scratch_bytes,), dtype=torch.uint8, device=DEV), stages=3)
    grads = dev_buf(base)
    d_thr, d_w = heads(grads)
    scratch = torch.empty((scratch_bytes,), dtype=torch.uint8, device=DEV)
    hip.ste_conv_backward(images, conv_out, thr, d_conv, stride, d_thr=d_thr, d_weight=d_w, scratch=scratch, stages=1)
    partial = torch.full((8,), float("nan"), device=DEV)
    hip.sqnorm_partials(grads[lo:hi], partial)
    p, m = dev_buf(p0), dev_buf(m0)
    norm = sgd_gpu(p, grads, m, 0.05, 0.9, 1e-4, 1.0, 0.5, False, ste=(scratch, chunks, fps, d_thr, d_w), ext=(partial, lo, hi))
    assert torch.equal(grads.cpu(), plain.cpu()), "the ride's d_thr / d_weight differ from the plain STE backward"
    r = torch_sgd(p0, plain.cpu(), m0, 0.05, 0.9, 1e-4, 1.0, 0.5, False)
    assert r["coef"] < 1.0
    assert_norm(norm, r["norm"])
    check_sgd("ste + ext", p, m, r)


@pytest.mark.parametrize("world", (2, 3, 4))
def test_sgd_sharded_update_on_one_gpu(world):
    """The sharded update's arithmetic (trainer.py: reduce-scatter -> per-shard partials -> all-gathered rank-major partials
    -> per-shard nnue_sgd_step(ext=(all_partials, 0, shard_len))), every shard on the one GPU: concatenated, the float64
    step of the whole buffer; every shard forms the identical norm."""
    real, padded = 23998, 24000  # the flat buffer padded to a multiple of the world size with zeros (FlatLayout pad_to)
    gen = torch.Generator().manual_seed(world)
    g = torch.zeros(padded)
    g[:real] = grads_of(real, 20.0, gen)
    p0, m0 = torch.zeros(padded), torch.zeros(padded)
    p0[:real], m0[:real] = torch.randn(real, generator=gen), torch.randn(real, generator=gen)
    p, m, gd = dev_buf(p0), dev_buf(m0), dev_buf(g)
    per, nparts = padded // world, 64
    all_partials = torch.full((world * nparts,), float("nan"), device=DEV)
    for rank in range(world):
        hip.sqnorm_partials(gd[rank * per:(rank + 1) * per], all_partials[rank * nparts:(rank + 1) * nparts])
    norms = []
    for rank in range(world):
        sl = slice(rank * per, (rank + 1) * per)
        norms.append(sgd_gpu(p[sl], gd[sl], m[sl], 0.05, 0.9, 2e-4, 1.0, 0.5, False, ext=(all_partials, 0, per)))
    assert len({struct_bits(n) for n in norms}) == 1, f"the shards formed different norms: {norms}"
    r = torch_sgd(p0, g, m0, 0.05, 0.9, 2e-4, 1.0, 0.5, False)
    assert r["coef"] < 1.0
    assert_norm(norms[0], r["norm"])
    check_sgd(f"{world} shards", p, m, r)


def struct_bits(x: float) -> int:
    return int(np.float32(x).view(np.int32))


# ------------------------------------------------------------------------------------------------- Adam
def torch_adam(p_old, g, m_old, v_old, t, lr, betas, eps, wd, max_norm, scale):
    """clip_grad_norm_ + torch.optim.Adam in float64 on the kernel's float32 inputs, from step t - 1's moments."""
    lr, b1, b2, eps, wd, max_norm, scale = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(wd), f32(max_norm), f32(scale)
    p_old, m_old, v_old = p_old.cpu().double(), m_old.cpu().double(), v_old.cpu().double()
    p = torch.nn.Parameter(p_old.clone())
    p.grad = g.cpu().double() * scale
    norm, coef = clip_reference(p, max_norm)
    t_g = p.grad.abs()
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m_old.clone(), "exp_avg_sq": v_old.clone()}
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == t
    m_ref, v_ref, p_ref = st["exp_avg"], st["exp_avg_sq"], p.detach()
    # the header's bounds
    clip_rtol = NORM_RTOL if coef < 1.0 else 0.0
    d = wd * p_old.abs() + t_g
    m_bound = K * U * (b1 * m_old.abs() + (1 - b1) * d) + clip_rtol * (1 - b1) * t_g
    v_bound = K * U * (b2 * v_old.abs() + (1 - b2) * d * d) + 2 * clip_rtol * (1 - b2) * d * t_g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    denom = v_ref.sqrt() / math.sqrt(bc2) + eps
    sqrt_err = torch.where(v_bound > 0, 2 * v_bound / (v_ref.sqrt() + v_bound.sqrt()), torch.zeros_like(v_bound))
    dir_err = (m_bound / bc1 + (m_ref / bc1).abs() * (sqrt_err / math.sqrt(bc2) + K * U * denom) / denom) / denom
    step = (p_ref - p_old).abs()
    return dict(p=p_ref, m=m_ref, v=v_ref, norm=norm, coef=coef, p_old=p_old, m_bound=m_bound, v_bound=v_bound,
                p_bound=K * U * (p_old.abs() + step) + lr * dir_err, upd_bound=2 * U * p_ref.abs() + K * U * step + lr * dir_err)


def check_adam(what, p, m, v, r):
    p = p.detach().cpu().double()
    assert_within(p, r["p"], r["p_bound"], f"{what}: parameters")
    assert_within(p - r["p_old"], r["p"] - r["p_old"], r["upd_bound"], f"{what}: update")
    assert_within(m.cpu(), r["m"], r["m_bound"], f"{what}: exp_avg")
    assert_within(v.cpu(), r["v"], r["v_bound"], f"{what}: exp_avg_sq")


def adam_gpu(p, g, m, v, counter, lr, betas, eps, wd, max_norm, scale, want_norm=True, lr_dev=None):
    norm = torch.full((), float("nan"), device=DEV) if want_norm else None
    hip.adam_step(p, g, m, v, counter, lr, betas, eps, wd, max_norm, scale, norm_out=norm, lr_dev=lr_dev)
    torch.cuda.synchronize()
    return None if norm is None else float(norm)


# (gradient amplitude, max_norm, norm requested, grad_scale) by step % 3
ADAM_STEPS = ((50.0, 1.0, True, 1.0), (1e-3, 1.0, True, 0.5), (1.0, 0.0, False, 1.0))


@pytest.mark.parametrize("count,off", [(1, 0), (5, 0), (64, 0), (1048573, 0), (4096, 1)])  # the last: a misaligned slice
@pytest.mark.parametrize("wd", (0.0, 1e-2))
def test_adam_chain(count, off, wd):
    """20 chained steps (bias correction from t = 1 to well past it); a quarter of the elements get an exactly zero gradient
    for the first 8 steps (the rows the map cannot reach) and a non-zero one afterwards."""
    gen = torch.Generator().manual_seed(count + off + int(wd * 100))
    p = dev_buf(torch.randn(count, generator=gen), off)
    m, v = dev_buf(torch.zeros(count), off), dev_buf(torch.zeros(count), off)
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    cold = torch.arange(count) % 4 == 3
    for s in range(20):
        amp, max_norm, want_norm, scale = ADAM_STEPS[s % 3]
        g = grads_of(count, amp, gen)
        if s < 8:
            g[cold] = 0.0
        r = torch_adam(p.cpu(), g, m.cpu(), v.cpu(), s + 1, 1e-2, (0.9, 0.999), 1e-8, wd, max_norm, scale)
        norm = adam_gpu(p, dev_buf(g, off), m, v, counter, 1e-2, (0.9, 0.999), 1e-8, wd, max_norm, scale, want_norm)
        assert int(counter.item()) == s + 1, "the step counter must advance by one per call"
        if want_norm:
            assert_norm(norm, r["norm"], f"step {s + 1} norm")
        check_adam(f"step {s + 1}", p, m, v, r)
        if s < 8 and wd == 0.0 and bool(cold.any()):
            assert torch.equal(p.cpu()[cold], r["p_old"][cold].float()), "a zero-gradient element moved without weight decay"


@pytest.mark.parametrize("betas,eps,use_lr_dev", [((0.0, 0.999), 1e-8, False), ((0.9, 0.0), 1e-8, False),
                                                  ((0.9, 0.999), 1e-3, False), ((0.9, 0.999), 1e-8, True)])
def test_adam_betas_eps_and_device_lr(betas, eps, use_lr_dev):
    count = 4099
    gen = torch.Generator().manual_seed(17)
    p = dev_buf(torch.randn(count, generator=gen))
    m, v = dev_buf(torch.zeros(count)), dev_buf(torch.zeros(count))
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    lr = 2e-3
    lr_dev = torch.tensor([lr], device=DEV) if use_lr_dev else None
    for s in range(5):
        amp, max_norm, want_norm, scale = ADAM_STEPS[s % 3]
        g = grads_of(count, amp, gen)
        r = torch_adam(p.cpu(), g, m.cpu(), v.cpu(), s + 1, lr, betas, eps, 1e-3, max_norm, scale)
        norm = adam_gpu(p, dev_buf(g), m, v, counter, 0.7 if use_lr_dev else lr, betas, eps, 1e-3, max_norm, scale, want_norm,
                        lr_dev=lr_dev)
        assert int(counter.item()) == s + 1
        if want_norm:
            assert_norm(norm, r["norm"])
        check_adam(f"step {s + 1}", p, m, v, r)


# ------------------------------------------------------------------------------------------------- non-finite gradients
@pytest.mark.parametrize("count", (4096, 4097))  # vector / scalar apply
@pytest.mark.parametrize("bad", ("nan", "inf"))
@pytest.mark.parametrize("max_norm", (1.0, 0.0))
def test_sgd_non_finite_gradient(count, bad, max_norm):
    """torch: a NaN norm makes the clip coefficient NaN and every gradient NaN; an Inf norm makes it 0 (the Inf element
    becomes NaN, the others 0).  Without clipping only the element itself is non-finite."""
    gen = torch.Generator().manual_seed(count)
    p, m = dev_buf(torch.randn(count, generator=gen)), dev_buf(torch.randn(count, generator=gen))
    g = grads_of(count, 0.5, gen)
    g[1234] = float(bad)
    r = torch_sgd(p.cpu(), g, m.cpu(), 0.05, 0.9, 2e-4, max_norm, 1.0, False)
    norm = sgd_gpu(p, dev_buf(g), m, 0.05, 0.9, 2e-4, max_norm, 1.0, False)
    assert_norm(norm, r["norm"])
    check_sgd(f"{bad} gradient", p, m, r)


@pytest.mark.parametrize("count,lo,hi", [(4096, 1024, 2048), (4098, 1024, 2048)])  # vector / scalar apply
def test_sgd_hole_nan_gradient(count, lo, hi):
    """A NaN inside the producer's range: the norm, coef_out and every element this launch updates are NaN, as torch's
    whole-buffer clip makes them; the hole keeps its bits."""
    gen = torch.Generator().manual_seed(count + 5)
    g = grads_of(count, 0.5, gen)
    g[1500] = float("nan")
    p, m, r, norm, coef = _hole_step(count, lo, hi, g, gen)
    assert math.isnan(r["coef"]) and math.isnan(coef), f"coef_out {coef}, torch {r['coef']}"
    assert_norm(norm, r["norm"])
    live = torch.ones(count, dtype=torch.bool)
    live[lo:hi] = False
    check_sgd("hole, NaN gradient", p, m, r, sel=live)


@pytest.mark.parametrize("bad", ("nan", "inf"))
@pytest.mark.parametrize("max_norm", (1.0, 0.0))
def test_adam_non_finite_gradient(bad, max_norm):
    count = 4097
    gen = torch.Generator().manual_seed(3)
    p, m, v = dev_buf(torch.randn(count, generator=gen)), dev_buf(torch.randn(count, generator=gen)), dev_buf(torch.rand(count, generator=gen))
    counter = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    g = grads_of(count, 0.5, gen)
    g[77] = float(bad)
    r = torch_adam(p.cpu(), g, m.cpu(), v.cpu(), 5, 1e-2, (0.9, 0.999), 1e-8, 1e-3, max_norm, 1.0)
    norm = adam_gpu(p, dev_buf(g), m, v, counter, 1e-2, (0.9, 0.999), 1e-8, 1e-3, max_norm, 1.0)
    assert_norm(norm, r["norm"])
    check_adam(f"{bad} gradient", p, m, v, r)


# ------------------------------------------------------------------------------------------------- cross-entropy
def ce_reference(logits, labels, grad_scale):
    z = logits.double().requires_grad_(True)
    loss = F.cross_entropy(z, labels, reduction="none")
    b = logits.shape[0]
    (loss.sum() * (grad_scale / b)).backward()
    sm = torch.softmax(z.detach(), dim=1)
    onehot = F.one_hot(labels, logits.shape[1]).double()
    d_bound = CE_RTOL * (sm.abs() + onehot) * (grad_scale / b) + CE_FLOOR
    return loss.detach(), z.grad, d_bound


def ce_logits(b, c, spread, gen):
    logits = (torch.rand(b, c, generator=gen) * 2 - 1) * spread
    labels = torch.randint(0, c, (b,), generator=gen)
    labels[0], labels[-1] = 0, c - 1  # the first and the last class
    return logits, labels


def check_ce(logits, labels, grad_scale=0.5):
    sample, loss, d = hip.cross_entropy(dev_buf(logits), labels.to(DEV), grad_scale)
    torch.cuda.synchronize()
    ref, ref_d, d_bound = ce_reference(logits, labels, grad_scale)
    assert_within(sample.cpu(), ref, CE_RTOL * ref.abs().clamp(min=1.0), "per-sample loss")
    ref_mean = float(ref.mean())
    assert abs(float(loss) - ref_mean) <= CE_RTOL * max(1.0, abs(ref_mean)), (float(loss), ref_mean)
    assert_within(d.cpu(), ref_d, d_bound, "d_logits")


@pytest.mark.parametrize("spread", (3.0, 80.0, 1e4))
@pytest.mark.parametrize("c", (1, 2, 63, 64, 65, 4096))  # lanes stride by 64
@pytest.mark.parametrize("b", (1, 3, 255, 256, 257))     # the mean is one 256-thread block
def test_cross_entropy_shapes(b, c, spread):
    gen = torch.Generator().manual_seed(b * 7919 + c)
    check_ce(*ce_logits(b, c, spread, gen))


@pytest.mark.parametrize("c,spread", [(10, 3.0), (65, 80.0)])
def test_cross_entropy_large_batch(c, spread):
    gen = torch.Generator().manual_seed(c)
    check_ce(*ce_logits(70000, c, spread, gen))


@pytest.mark.parametrize("c", (2, 10, 65, 200))
def test_cross_entropy_non_finite_rows(c):
    """NaN, +Inf and -Inf logits: the per-sample loss is finite exactly where torch's float64 loss is (-Inf on a class that
    is not the label), and the mean is non-finite whenever torch's is."""
    gen = torch.Generator().manual_seed(c)
    b = 64
    logits, labels = ce_logits(b, c, 3.0, gen)
    other = (labels + 1) % c
    nan, inf = float("nan"), float("inf")
    rows = [(nan, "label"), (nan, "other"), (inf, "other"), (inf, "label"), (-inf, "other"), (-inf, "label")]
    for i, (val, where) in enumerate(rows):
        logits[i, labels[i] if where == "label" else other[i]] = val
    logits[6] = -inf               # every class -Inf
    logits[7, other[7]] = inf      # +Inf and -Inf in one row
    logits[7, labels[7]] = -inf
    logits[8, other[8]] = -inf     # two -Inf, neither the label
    if c > 2:
        logits[8, (labels[8] + 2) % c] = -inf
    sample, loss, d = hip.cross_entropy(dev_buf(logits), labels.to(DEV), 0.5)
    torch.cuda.synchronize()
    ref, ref_d, d_bound = ce_reference(logits, labels, 0.5)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(sample.cpu()), fin), (sample.cpu()[:10], ref[:10])
    assert bool(fin[4]) and bool(fin[8]) and not bool(fin[:4].any())
    assert_within(sample.cpu()[fin], ref[fin], CE_RTOL * ref[fin].abs().clamp(min=1.0), "finite per-sample losses")
    assert_within(d.cpu()[fin], ref_d[fin], d_bound[fin], "d_logits of the finite rows")
    assert not math.isfinite(float(loss)) and not math.isfinite(float(ref.mean()))
    # the finite rows alone (a -Inf on another class included): a finite mean within the bar
    keep = torch.nonzero(fin).flatten()
    check_ce(logits[keep].contiguous(), labels[keep].contiguous())


# ------------------------------------------------------------------------------------------------- confusion
def confusion_reference(logits, labels):
    z, y = logits.numpy(), labels.numpy()
    c = z.shape[1]
    if c == 1:
        pred, truth = (z[:, 0] > 0.5).astype(np.int64), (y > 0.5).astype(np.int64)
        k = 2
    else:
        pred, truth, k = np.argmax(z, axis=1), y, c
    conf = np.zeros((k, k), dtype=np.int64)
    ok = (truth >= 0) & (truth < k)
    np.add.at(conf, (truth[ok], pred[ok]), 1)
    return conf


@pytest.mark.parametrize("c", (2, 10, 100))
def test_confusion_ties_nan_and_labels(c):
    """Exact ties (the first maximum wins), NaN rows (the first NaN wins, as numpy.argmax), out-of-range labels (not
    counted), B over several 256-sample blocks, accumulated over three calls into one matrix."""
    gen = torch.Generator().manual_seed(c)
    b = 1000
    logits = torch.randint(0, 3, (b, c), generator=gen).float()
    labels = torch.randint(0, c, (b,), generator=gen)
    for i in range(0, 60):
        logits[i, int(torch.randint(0, c, (1,), generator=gen))] = float("nan")
    for i in range(40, 60):  # a second NaN
        logits[i, int(torch.randint(0, c, (1,), generator=gen))] = float("nan")
    logits[60:64] = float("nan")
    logits[64:70, 0] = float("nan")
    logits[70:74, -1] = float("nan")
    logits[74:80] = -float("inf")
    labels[100:104] = -1
    labels[104:108] = c
    labels[108:110] = c + 7
    conf = None
    for lo, hi in ((0, 300), (300, 700), (700, b)):
        conf = hip.confusion_accumulate(logits[lo:hi].to(DEV), labels[lo:hi].to(DEV), conf)
    got = conf.cpu().numpy()
    want = confusion_reference(logits, labels)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert int(got.sum()) == b - 10


def test_confusion_single_output():
    """C == 1: the reference's binary rule, output > 0.5 against target > 0.5 (integer labels: >= 1)."""
    gen = torch.Generator().manual_seed(1)
    b = 600
    logits = torch.rand(b, 1, generator=gen)
    logits[:20] = 0.5
    logits[20:30] = float("nan")
    labels = torch.randint(0, 2, (b,), generator=gen)
    labels[30:35] = 2
    conf = hip.confusion_accumulate(logits.to(DEV), labels.to(DEV))
    conf = hip.confusion_accumulate(logits[:100].to(DEV), labels[:100].to(DEV), conf)
    want = confusion_reference(logits, labels) + confusion_reference(logits[:100], labels[:100])
    assert np.array_equal(conf.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------- reproducibility
def test_every_entry_point_is_bitwise_reproducible():
    """optim_kernels.hip's promise: staged sums, so the same inputs give the same bits."""
    gen = torch.Generator().manual_seed(5)

    def sgd(count, off, **kw):
        g = grads_of(count, 20.0, torch.Generator().manual_seed(count))
        p0, m0 = torch.randn(count, generator=torch.Generator().manual_seed(1)), torch.randn(count, generator=torch.Generator().manual_seed(2))
        outs = []
        for _ in range(2):
            p, m, gd = dev_buf(p0, off), dev_buf(m0, off), dev_buf(g, off)
            extra = {}
            if kw.get("hole"):
                part, coef = torch.zeros((16,), device=DEV), torch.zeros((), device=DEV)
                hip.sqnorm_partials(gd[1024:2048], part)
                extra = dict(ext=(part, 1024, 2048), coef_out=coef, ext_applied_elsewhere=True)
            norm = sgd_gpu(p, gd, m, 0.05, 0.9, 2e-4, 1.0, 0.5, False, **extra)
            outs.append((p.cpu(), m.cpu(), struct_bits(norm)))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2], (count, off, kw)

    sgd(1 << 20, 0)
    sgd(1 << 20, 1)
    sgd(8192, 0, hole=True)
    sgd(8194, 0, hole=True)
    count = 100003
    p0, g = torch.randn(count, generator=gen), grads_of(count, 20.0, gen)
    outs = []
    for _ in range(2):
        p, m, v = dev_buf(p0), dev_buf(torch.zeros(count)), dev_buf(torch.zeros(count))
        counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
        norm = adam_gpu(p, dev_buf(g), m, v, counter, 1e-2, (0.9, 0.999), 1e-8, 1e-3, 1.0, 1.0)
        outs.append((p.cpu(), m.cpu(), v.cpu(), struct_bits(norm)))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3]
    logits, labels = ce_logits(70000, 65, 80.0, gen)
    runs = [hip.cross_entropy(logits.to(DEV), labels.to(DEV), 0.5) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.cpu(), b.cpu())
    confs = [hip.confusion_accumulate(logits.to(DEV), labels.to(DEV)).cpu() for _ in range(2)]
    assert torch.equal(confs[0], confs[1])
