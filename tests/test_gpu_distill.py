"""Distillation (the teacher arm of include/nnue_hip.h, "soft targets") in the classifier's training step --
nnue_classifier_train_step_distill[_bucketed], the DISTILL arm of both tail kernels -- and in the stand-alone loss
nnue_cross_entropy_distill, through the C ABI against float64 torch on the CPU.  ``-m gpu``.  Built on
tests/test_gpu_soft_targets.py (``CASES``, ``run_step``'s layout, ``soft_reference``) and tests/test_gpu_classifier_train.py's
bounds.

Per sample, beside the soft target t (labels a, a2, weight lam, smoothing eps): teacher logits u, one alpha in [0, 1] and one
T > 0 per call.  With q = softmax(u / T), pT = softmax(z / T), p = softmax(z):
    loss = (1-alpha) L_soft + alpha T^2 KL(q || pT),   d_logits = ((1-alpha) (p - t) + alpha T (pT - q)) grad_scale / B
The float64 reference is formed from the kernel's own logits with both logs from ``log_softmax`` (never the log of a rounded
probability): KL = sum_c q_c (log q_c - log pT_c), CE(q, pT) = -sum_c q_c log pT_c, H(q) = -sum_c q_c log q_c.

Bars, element by element (U = 2^-24, gamma_n = n U / (1 - n U), CE_RTOL = 1e-5 of test_gpu_classifier_train.py):
* h1, h2, logits: bitwise the plain call's (they do not depend on the loss).
* sample_loss: CE_RTOL max(1, (1-alpha) L_soft + alpha T^2 (CE(q, pT) + H(q)))      -- relative to the two non-negative sums the
  KL term is the difference of, not to the difference
  + (1-alpha) gamma_{C+4} (eps/C) sum_c (mx - z_c)                                   -- the soft loss's smoothing sum, as there,
  scaled as the kernel scales it
  + gamma_{C+4} alpha T sum_c q_c (|mx - z_c| + |mu - u_c|)                           -- the C-term KL sum: alpha T^2 (1/T) sum ...
  Every T of the table below is a power of two, so the divisions by T in the exponents and in (ksum / sU) / T are exact and
  need no term of their own; expf / logf are a few ulp, inside CE_RTOL (168 ulp).
  Mean loss: the mean of the per-sample bars + gamma_{B+2} of the mean of the |per-sample losses|.
* d_logits: CE_RTOL ((1-alpha) (p + t) + alpha T (pT + q)) grad_scale / B + 2^-126.
* d_z1, the gradients and d_x: test_gpu_classifier_train.py's propagated bounds, each stage from the kernel's own previous one.
* exact: alpha = 0 with a NaN-filled teacher gives the soft call's bits; a row that does not count has loss 0 and a zero
  gradient row whatever its teacher row holds (the test puts NaN there); phases 123 and 59 agree bitwise; the forward-only
  stand-alone call has the bits of the one with gradient; a refused call leaves NaN-filled outputs untouched.

Teacher regimes: ``randn3`` (randn * 3), ``tie`` (near 1e4, the runner-up 3 below the maximum; the student's logits are then in
their own tie regime), ``same`` (the plain call's logits: KL ~ 0, the loss a difference of two nearly equal sums), ``peaked``
(one class 90 T above the rest: q underflows elsewhere).  Every case meets every (T, alpha) pair and every regime once.
"""
import ctypes
import functools

import pytest
import torch

from nnue_hip import lib as hip
from test_gpu_classifier_train import (CE_RTOL, CLIP, DEV, GRAD_SCALE, TINY, Stacks, assert_within, c64, gamma, gate64, l0_of,
                                       read_dz1, scratch_for, to_dev)
from test_gpu_soft_targets import CASES, bits, inputs_of, make_targets, soft_reference

pytestmark = pytest.mark.gpu

PAIRS = ((1.0, 1.0), (2.0, 0.5), (4.0, 0.9), (0.5, 0.3))  # (T, alpha)
TEACHERS = ("randn3", "tie", "same", "peaked")
KINDS = ("plain", "smooth_mix", "edges")
E_ARG = -1
# every case meets every pair and every teacher regime once, and every soft kind at least once
COMBOS = [(name, PAIRS[j], TEACHERS[(i + j) % 4], KINDS[(i + j) % 3]) for i, name in enumerate(CASES) for j in range(4)]


def make_teacher(regime, B, C, T, same, seed):
    """Teacher logits float32 [B, C] on the CPU; ``same``: the logits to return in that regime."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(B, C, generator=gen) * 3
    if regime == "tie":
        u = u * 1e-3 - 5e3 - torch.arange(C, dtype=torch.float32)
        u[:, 0] += 1.5e4
        if C > 1:
            u[:, 1] += 1.5e4 - 2
    elif regime == "same":
        u = same.detach().float().cpu().clone()
    elif regime == "peaked":
        k = torch.randint(0, C, (B,), generator=gen)
        u[torch.arange(B), k] = u.max(dim=1).values + 90.0 * T
    return u


def distill_reference(lgk, a, a2, lam, eps, u, alpha, T):
    """float64, from the kernel's own logits lgk and the teacher's u: per-sample loss and bar, d_logits / scale and its bar /
    scale, and the mask of the rows that count (module header)."""
    B, C = lgk.shape
    per_s, _, sm, t, counts = soft_reference(lgk, a, a2, lam, eps)
    zero = torch.zeros((), dtype=torch.float64)
    u = torch.where(counts.unsqueeze(1), u.double(), zero)  # (rows that do not count may hold NaN: they are masked below)
    logq, logp = torch.log_softmax(u / T, dim=1), torch.log_softmax(lgk / T, dim=1)
    q, pT = logq.exp(), logp.exp()
    kl = (q * (logq - logp)).sum(1)
    ce_q, h_q = -(q * logp).sum(1), -(q * logq).sum(1)
    mx, mu = lgk.max(dim=1, keepdim=True).values, u.max(dim=1, keepdim=True).values
    per = (1 - alpha) * per_s + alpha * T * T * kl
    bound = (CE_RTOL * ((1 - alpha) * per_s + alpha * T * T * (ce_q + h_q)).clamp(min=1.0)
             + (1 - alpha) * gamma(C + 4) * (eps / C) * (mx - lgk).sum(1)
             + gamma(C + 4) * alpha * T * (q * ((mx - lgk).abs() + (mu - u).abs())).sum(1))
    per, bound = torch.where(counts, per, zero), torch.where(counts, bound, zero)
    m = counts.unsqueeze(1)
    dl = torch.where(m, (1 - alpha) * (sm - t) + alpha * T * (pT - q), zero)
    dl_b = torch.where(m, CE_RTOL * ((1 - alpha) * (sm + t) + alpha * T * (pT + q)), zero)
    return per, bound, dl, dl_b, counts


def step_buffers(name, regime, labels):
    shape, phases, K = CASES[name]
    B, L1, L2, L3, C = shape
    x, w, _, bucket, slabs = inputs_of(name, regime)
    xd, wd, yd = to_dev(x, w, labels)
    plan = hip.bucket_group(bucket.to(DEV, torch.int32), 0, K) if K > 1 else None
    scratch = scratch_for(B, L1, L2, L3, C, K)
    scratch.fill_(0x7F)
    if slabs is not None:
        scratch[:slabs.numel() * 4].view(torch.float32).copy_(slabs.reshape(-1).to(DEV))
    lead = (K,) if K > 1 else ()
    grads = [torch.full(lead + s, float("nan"), device=DEV) for s in ((L2, L1), (L2,), (L3, L2), (L3,), (C, L3), (C,))]
    return xd, wd, yd, plan, scratch, grads


def run_step(name, regime, clip, labels, soft, distill):
    """test_gpu_soft_targets.run_step with the ``distill`` argument: one call at the case's phases, the named outputs."""
    shape, phases, K = CASES[name]
    B, L1, L2, L3, C = shape
    xd, wd, yd, plan, scratch, grads = step_buffers(name, regime, labels)
    dev = lambda v: v.to(DEV) if torch.is_tensor(v) else v  # noqa: E731
    soft = None if soft is None else tuple(dev(v) for v in soft)
    distill = None if distill is None else tuple(dev(v) for v in distill)
    res = hip.classifier_train_step(xd, True, *wd, yd, GRAD_SCALE, clip, scratch=scratch, phases=phases, buckets=plan, grads=grads,
                                    soft=soft, distill=distill)
    torch.cuda.synchronize()
    (h1, h2, logits), (sample_loss, loss), d_x, grads = res
    out = {"h1": h1, "h2": h2, "logits": logits, "sample_loss": sample_loss, "loss": loss, "d_x": d_x, "grads": grads}
    if K == 1:
        off = hip.classifier_train_dz1_offset(B, L1, L2, L3, C, True)
        r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
        o_dl = off + r4(B * L2) * 4 + r4(B * L3) * 4
        out["d_z1"] = read_dz1(scratch, B, L1, L2, L3, C, True)
        out["d_logits"] = scratch[o_dl:o_dl + B * C * 4].view(torch.float32).view(B, C)
    else:  # grouped rows: d_z1 back in sample order
        rows = plan.rows.cpu().long()
        dz_off, _ = hip.classifier_train_grouped_offsets(B, L1, L2, L3, C, K)
        d_z1_g = scratch[dz_off:dz_off + rows.numel() * L2 * 4].view(torch.float32).view(-1, L2).cpu()
        d_z1 = torch.empty(B, L2)
        d_z1[rows[rows >= 0]] = d_z1_g[rows >= 0]
        out["d_z1"] = d_z1
    return out


@functools.lru_cache(maxsize=None)
def plain_step(name, regime, clip):
    """The plain call of a case (its labels), kept: the bits h1, h2 and logits must have, and the ``same`` teacher."""
    return run_step(name, regime, clip, inputs_of(name, regime)[2], None, None)


@pytest.mark.parametrize("name,pair,teacher,kind", COMBOS, ids=[f"{n}-T{p[0]}-a{p[1]}-{t}-{k}" for n, p, t, k in COMBOS])
def test_distill_train_step_against_float64(name, pair, teacher, kind):
    shape, phases, K = CASES[name]
    B, L1, L2, L3, C = shape
    T, alpha = pair
    regime = "tie" if teacher == "tie" else "randn"
    clip = CLIP if (sum(shape) + KINDS.index(kind)) % 2 else 0.0
    x, w, labels, bucket, _ = inputs_of(name, regime)
    a, a2, lam, eps = make_targets(kind, labels, C, seed=sum(shape) + KINDS.index(kind))
    plain = plain_step(name, regime, clip)
    u = make_teacher(teacher, B, C, T, plain["logits"], seed=sum(shape) + TEACHERS.index(teacher))
    counts = soft_reference(c64(plain["logits"]), a, a2, lam, eps)[4]
    u[~counts] = float("nan")  # the padding rule: a row that does not count is not read into any result
    got = run_step(name, regime, clip, a, (a2, lam, eps), (u, alpha, T))
    tag = f"{name} T={T} alpha={alpha} {teacher} {kind}"
    for nm in ("h1", "h2", "logits"):
        assert torch.equal(bits(got[nm]), bits(plain[nm])), f"{tag} {nm}: not the plain call's bits"

    st = Stacks(B, K, bucket)
    w1, b1, w2, b2, w3, b3 = (c64(t) for t in w)
    h1k, h2k, lgk, dz1k = c64(got["h1"]), c64(got["h2"]), c64(got["logits"]), c64(got["d_z1"])
    per, per_bound, dl, dl_b, counts = distill_reference(lgk, a, a2, lam, eps, u, alpha, T)
    print(f"{tag}: max |loss err| / bar = {float(((c64(got['sample_loss']) - per).abs() / per_bound.clamp(min=1e-300)).max()):.3g}")
    assert_within(got["sample_loss"], per, per_bound, f"{tag} sample loss")
    assert not bool(got["sample_loss"].cpu()[~counts].any()), f"{tag}: an excluded row has a loss"
    scale = GRAD_SCALE / B
    dl, dl_b = dl * scale, torch.where(counts.unsqueeze(1), dl_b * scale + TINY, torch.zeros((), dtype=torch.float64))
    if K == 1:
        print(f"{tag}: max |d_logits err| / bar = {float(((c64(got['d_logits']) - dl).abs() / dl_b.clamp(min=1e-300)).max()):.3g}")
        assert_within(got["d_logits"], dl, dl_b, f"{tag} d_logits")
        assert not bool(got["d_logits"].cpu()[~counts].any()), f"{tag}: an excluded row has a gradient"
    # from here on test_gpu_classifier_train.check_step's propagated bounds, with dl / dl_b as formed above
    nC, nB, nL3, nL2 = C + 8, B + 8, L3 + 4, L2 + 4
    dz2 = gate64(st.bwd(dl, w3), h2k, clip)
    dz2_b = gate64(st.bwd(dl_b, w3.abs()) + gamma(nC) * st.bwd(dl.abs() + dl_b, w3.abs()) + nC * TINY, h2k, clip)
    dz1 = gate64(st.bwd(dz2, w2), h1k, clip)
    dz1_b = gate64(st.bwd(dz2_b, w2.abs()) + gamma(nL3) * st.bwd(dz2.abs() + dz2_b, w2.abs()) + nL3 * TINY, h1k, clip)
    assert_within(got["d_z1"], dz1, dz1_b, f"{tag} d_z1")
    if not phases & hip.CLS_SMALL_RIDE:  # (with bit 32 the small gradients and the mean loss are left to nnue_ftm_backward's launch)
        assert_within(got["loss"].reshape(1), per.mean().reshape(1), per_bound.mean() + gamma(B + 2) * per.abs().mean(), f"{tag} mean loss")

        def batch_bound(d, d_b, inp):
            return st.wgrad(d_b, inp.abs()) + gamma(nB) * st.wgrad(d.abs() + d_b, inp.abs()) + nB * TINY

        def bias_bound(d, d_b):
            return st.bgrad(d_b) + gamma(nB) * st.bgrad(d.abs() + d_b) + nB * TINY

        d_w1, d_b1, d_w2, d_b2, d_w3, d_b3 = got["grads"]
        assert_within(d_w3, st.wgrad(dl, h2k), batch_bound(dl, dl_b, h2k), f"{tag} d_w3")
        assert_within(d_b3, st.bgrad(dl), bias_bound(dl, dl_b), f"{tag} d_b3")
        assert_within(d_w2, st.wgrad(dz2, h1k), batch_bound(dz2, dz2_b, h1k), f"{tag} d_w2")
        assert_within(d_b2, st.bgrad(dz2), bias_bound(dz2, dz2_b), f"{tag} d_b2")
        assert_within(d_b1, st.bgrad(dz1k), gamma(nB) * st.bgrad(dz1k.abs()) + nB * TINY, f"{tag} d_b1")
        if not phases & hip.CLS_DW1_RIDES:
            nW1 = B + B // 16 + 8
            l0 = l0_of(c64(x), True)
            assert_within(d_w1, st.wgrad(dz1k, l0), gamma(nW1) * st.wgrad(dz1k.abs(), l0.abs()) + nW1 * TINY, f"{tag} d_w1")
    x64 = c64(x)
    d_l0, a_l0 = st.bwd(dz1k, w1), st.bwd(dz1k.abs(), w1.abs())
    h = L1 // 2
    xa, xb = x64[:, :h], x64[:, h:]
    ref_dx = torch.cat([d_l0[:, :h] * xb + d_l0[:, h:], d_l0[:, :h] * xa], dim=1)
    a_dx = torch.cat([a_l0[:, :h] * xb.abs() + a_l0[:, h:], a_l0[:, :h] * xa.abs()], dim=1)
    assert_within(got["d_x"], ref_dx, gamma(nL2) * a_dx + nL2 * TINY, f"{tag} d_x")


@pytest.mark.parametrize("name", list(CASES))
def test_alpha_zero_is_the_soft_call_and_does_not_read_the_teacher(name):
    shape, phases, K = CASES[name]
    B, C = shape[0], shape[4]
    labels = inputs_of(name, "randn")[2]
    a, a2, lam, eps = make_targets("edges", labels, C, seed=B + C)
    soft = run_step(name, "randn", CLIP, a, (a2, lam, eps), None)
    for teacher in (torch.full((B, C), float("nan")), None):
        got = run_step(name, "randn", CLIP, a, (a2, lam, eps), (teacher, 0.0, 3.0))
        for nm in ("h1", "h2", "logits", "sample_loss", "d_z1", "d_x") + (("d_logits",) if K == 1 else ()):
            assert torch.equal(bits(got[nm]), bits(soft[nm])), (name, nm, teacher is None)
        if not phases & hip.CLS_SMALL_RIDE:
            assert torch.equal(bits(got["loss"].reshape(1)), bits(soft["loss"].reshape(1))), name


def test_fused_tail_with_and_without_dx_tiles_agree_bitwise():
    """phases 123 (the DISTILL arm inside the d_x launch) against 59 (the tile tail alone, then the d_x launch)."""
    for (on_name, off_name), (T, alpha) in zip((("tile10dx", "tile10"), ("tile64dx", "tile64")), ((2.0, 0.5), (0.5, 0.3))):
        B, C = CASES[on_name][0][0], CASES[on_name][0][4]
        labels = inputs_of(on_name, "randn")[2]
        a, a2, lam, eps = make_targets("edges", labels, C, seed=3)
        u = make_teacher("randn3", B, C, T, None, seed=5)
        on = run_step(on_name, "randn", CLIP, a, (a2, lam, eps), (u, alpha, T))
        off = run_step(off_name, "randn", CLIP, a, (a2, lam, eps), (u, alpha, T))
        for nm in ("h1", "h2", "logits", "sample_loss", "d_logits", "d_z1", "d_x"):
            assert torch.equal(bits(on[nm]), bits(off[nm])), (on_name, nm)


# ------------------------------------------------------------------------------------------------- the stand-alone loss
CE_COMBOS = [(C, TEACHERS[j], PAIRS[(i + j) % 4], KINDS[(i + j) % 3]) for i, C in enumerate((1, 2, 64, 65, 1000)) for j in range(4)]


@pytest.mark.parametrize("C,teacher,pair,kind", CE_COMBOS, ids=[f"C{c}-{t}-T{p[0]}-a{p[1]}-{k}" for c, t, p, k in CE_COMBOS])
def test_cross_entropy_distill_against_float64(C, teacher, pair, kind):
    B = 37
    T, alpha = pair
    gen = torch.Generator().manual_seed(C + KINDS.index(kind))
    logits = torch.randn(B, C, generator=gen) * 3
    labels = torch.randint(0, C, (B,), generator=gen)
    if teacher == "tie":  # the student in its own tie regime: logits near 1e4, the runner-up 3 below the maximum
        logits = logits * 1e-3 - 5e3 - torch.arange(C, dtype=torch.float32)
        logits[:, 0] += 1.5e4
        if C > 1:
            logits[:, 1] += 1.5e4 - 2
        logits = logits.flip(1).contiguous()  # (not the teacher's order)
    a, a2, lam, eps = make_targets(kind, labels, C, seed=C + 11)
    u = make_teacher(teacher, B, C, T, logits, seed=C + 17)
    counts = soft_reference(logits.double(), a, a2, lam, eps)[4]
    u[~counts] = float("nan")
    dev = lambda v: v.to(DEV) if torch.is_tensor(v) else v  # noqa: E731
    sample_loss, loss, d_logits = hip.cross_entropy_distill(dev(logits), dev(a), dev(u), alpha, T, dev(a2), dev(lam), eps,
                                                            grad_scale=GRAD_SCALE)
    fwd_only = hip.cross_entropy_distill(dev(logits), dev(a), dev(u), alpha, T, dev(a2), dev(lam), eps, grad_scale=GRAD_SCALE,
                                         want_grad=False)
    torch.cuda.synchronize()
    tag = f"C={C} {teacher} T={T} alpha={alpha} {kind}"
    per, per_bound, dl, dl_b, counts = distill_reference(logits.double(), a, a2, lam, eps, u, alpha, T)
    print(f"{tag}: max |loss err| / bar = {float(((c64(sample_loss) - per).abs() / per_bound.clamp(min=1e-300)).max()):.3g}")
    assert_within(sample_loss, per, per_bound, f"{tag} sample loss")
    assert_within(loss.reshape(1), per.mean().reshape(1), per_bound.mean() + gamma(B + 2) * per.abs().mean(), f"{tag} mean loss")
    scale = GRAD_SCALE / B
    dl_b = torch.where(counts.unsqueeze(1), dl_b * scale + TINY, torch.zeros((), dtype=torch.float64))
    assert_within(d_logits, dl * scale, dl_b, f"{tag} d_logits")
    assert not bool(sample_loss.cpu()[~counts].any()) and not bool(d_logits.cpu()[~counts].any()), f"{tag}: an excluded row is not zero"
    assert fwd_only[2] is None
    assert torch.equal(bits(fwd_only[0]), bits(sample_loss)) and torch.equal(bits(fwd_only[1].reshape(1)), bits(loss.reshape(1)))


def test_cross_entropy_distill_alpha_zero_is_the_soft_call():
    B, C = 37, 65
    gen = torch.Generator().manual_seed(1)
    logits, labels = (torch.randn(B, C, generator=gen) * 3).to(DEV), torch.randint(0, C, (B,), generator=gen)
    a, a2, lam, eps = (v.to(DEV) if torch.is_tensor(v) else v for v in make_targets("edges", labels, C, seed=2))
    soft = hip.cross_entropy_soft(logits, a, a2, lam, eps, grad_scale=GRAD_SCALE)
    for teacher in (torch.full((B, C), float("nan"), device=DEV), None):
        got = hip.cross_entropy_distill(logits, a, teacher, 0.0, 2.0, a2, lam, eps, grad_scale=GRAD_SCALE)
        assert all(torch.equal(bits(g.reshape(-1)), bits(s.reshape(-1))) for g, s in zip(got, soft))


# ------------------------------------------------------------------------------------------------- refusals
REFUSALS = {  # the five: what to change in an accepted call
    "alpha above 1": dict(alpha=1.5), "alpha NaN": dict(alpha=float("nan")), "alpha negative": dict(alpha=-0.1),
    "T zero": dict(T=0.0), "T negative": dict(T=-1.0), "T infinite": dict(T=float("inf")), "T NaN": dict(T=float("nan")),
    "no teacher": dict(teacher=None),
    "eps": dict(eps=1.0),
    "labels_b without lam": dict(lam=None),
}


@pytest.mark.parametrize("what", list(REFUSALS))
@pytest.mark.parametrize("bucketed", (False, True))
def test_train_step_distill_refusals_launch_nothing(what, bucketed):
    name = "cls2"
    shape, phases, _ = CASES[name]
    B, L1, L2, L3, C = shape
    labels = inputs_of(name, "randn")[2]
    xd, wd, yd, _, scratch, grads = step_buffers(name, "randn", labels)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    outs = [nan(B, L2), nan(B, L3), nan(B, C), nan(B), nan(1), nan(B, L1)]
    kw = dict(alpha=0.5, T=2.0, teacher=torch.zeros(B, C, device=DEV), eps=0.1, labels_b=yd.clone(), lam=torch.ones(B, device=DEV))
    kw.update(REFUSALS[what])
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    args = [p(xd), 1, *[p(t) for t in wd], 0.0, p(yd), GRAD_SCALE, B, L1, L2, L3, C, *[p(t) for t in outs[:5]], p(outs[5]),
            *[p(g) for g in grads], p(scratch), scratch.numel(), phases, p(kw["labels_b"]), p(kw["lam"]), kw["eps"], p(kw["teacher"]),
            kw["alpha"], kw["T"]]
    L = hip.load()
    before = [bits(t).clone() for t in outs + grads] + [scratch.clone()]
    rc = (L.nnue_classifier_train_step_distill_bucketed(*args, None, None) if bucketed
          else L.nnue_classifier_train_step_distill(*args, None))
    torch.cuda.synchronize()
    assert rc == E_ARG, (what, rc)
    after = [bits(t) for t in outs + grads] + [scratch]
    assert all(torch.equal(x, y) for x, y in zip(before, after)), f"{what}: a refused call wrote something"


@pytest.mark.parametrize("what", list(REFUSALS))
def test_cross_entropy_distill_refusals_launch_nothing(what):
    B, C = 8, 5
    logits, labels = torch.randn(B, C, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    outs = [nan(B), nan(1), nan(B, C)]
    kw = dict(alpha=0.5, T=2.0, teacher=torch.zeros(B, C, device=DEV), eps=0.1, labels_b=labels.clone(), lam=torch.ones(B, device=DEV))
    kw.update(REFUSALS[what])
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    rc = hip.load().nnue_cross_entropy_distill(p(logits), p(labels), p(kw["labels_b"]), p(kw["lam"]), kw["eps"], B, C, 1.0, p(outs[0]),
                                               p(outs[1]), p(outs[2]), p(kw["teacher"]), kw["alpha"], kw["T"], None)
    torch.cuda.synchronize()
    assert rc == E_ARG, (what, rc)
    assert all(bool(torch.isnan(t).all()) for t in outs), f"{what}: a refused call wrote something"
