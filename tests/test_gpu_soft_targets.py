"""Soft targets (label smoothing, mixup / CutMix weights; include/nnue_hip.h "soft targets") in the classifier's training step
-- nnue_classifier_train_step_soft[_bucketed], the SOFT arm of both tail kernels -- and in the stand-alone loss
nnue_cross_entropy_soft, against float64 torch on the CPU.  ``-m gpu``.  Built on tests/test_gpu_classifier_train.py: its
input builders, ``Stacks``, ``assert_within`` and bounds.

Per sample: labels a, a2, a weight lam, one eps per call;
    t_c = (1-eps) (lam [c == a] + (1-lam) [c == a2]) + eps/C,  loss = sum_c t_c (lse - z_c),  d_logits = (softmax - t) grad_scale / B
= lam CE(z, a) + (1-lam) CE(z, a2) with label_smoothing = eps.  A sample counts iff a is a class and (lam == 1 or a2 is one);
an excluded row has loss 0 and a zero gradient row, exactly.

Bars, element by element (U = 2^-24, gamma_n = n U / (1 - n U)):
* h1, h2, logits: bitwise those of the plain entry point on the same inputs (they do not depend on the loss).
* sample_loss: 1e-5 max(1, |ref|) + gamma_{C+4} (eps/C) sum_c (mx - z_c) -- that file's CE_RTOL bar plus the rounding of the
  C-term sum; the reference is formed from the kernel's own logits.  Mean loss: the mean of the per-sample bars + gamma_B of
  the sum.
* d_logits: 1e-5 (softmax + t) grad_scale / B + 2^-126.
* d_z1, the gradients and d_x: that file's propagated bounds, each stage from the kernel's own previous one.
* eps = 0, lam = 1, labels_b = labels: sample_loss and d_logits bitwise the plain call's (1 x + 0 y and p - 1 are exact).
"""
import functools

import pytest
import torch

from nnue_hip import lib as hip
from test_gpu_classifier_train import (CE_RTOL, CLIP, DEV, GRAD_SCALE, TINY, Stacks, assert_within, c64, gamma, gate64, l0_of,
                                       make_inputs, read_dz1, scratch_for, to_dev)

pytestmark = pytest.mark.gpu

# name: (B, L1, L2, L3, C), phases, K
CASES = {
    "cls1": ((20, 64, 32, 8, 1), 3, 1),
    "cls2": ((20, 64, 32, 8, 2), 3, 1),
    "cls64": ((64, 96, 48, 36, 64), 3, 1),        # wave reduction at its limit
    "cls65": ((64, 96, 48, 36, 65), 3, 1),        # block reduction
    "cls257": ((40, 320, 160, 40, 257), 3, 1),    # NT = 512
    "B37": ((37, 256, 48, 16, 7), 3, 1),          # ragged B, not VEC
    "tile10dx": ((37, 128, 128, 32, 10), 123, 1),  # the fused tail at a ragged row tile, with its d_x tiles
    "tile10": ((37, 128, 128, 32, 10), 59, 1),     # ... and alone (the d_x launch follows)
    "tile64dx": ((37, 128, 128, 32, 64), 123, 1),
    "tile64": ((37, 128, 128, 32, 64), 59, 1),
    "grouped": ((48, 128, 64, 16, 10), 19, 3),    # bucketed stacks, the per-sample kernel once per grouped row
    "C2": ((512, 1024, 128, 32, 10), 123, 1),
}
REGIMES = ("randn", "tie")
TARGETS = ("plain", "smooth", "mix", "smooth_mix", "edges")


def make_targets(kind, labels, C, seed):
    """(labels a, labels_b a2 or None, lam or None, eps) on the CPU.  ``edges``: lam in {0, 1} exactly, a2 == a on some rows,
    a = -1 on some rows, a2 = -1 once with lam = 1 (the row counts) and once with lam < 1 (it does not)."""
    B = labels.numel()
    gen = torch.Generator().manual_seed(seed)
    a = labels.clone()
    a2 = torch.randint(0, C, (B,), generator=gen)
    lam = torch.rand(B, generator=gen)
    if kind == "plain":
        return a, a.clone(), torch.ones(B), 0.0
    if kind == "smooth":
        return a, None, None, 0.1
    if kind == "mix":
        return a, a2, lam, 0.0
    if kind == "smooth_mix":
        return a, a2, lam, 0.1
    lam = (torch.rand(B, generator=gen) < 0.5).float()
    a2[2], a2[3] = a[2], a[3]
    a[4], a[5] = -1, -1
    lam[4], lam[5] = 1.0, 0.0
    a2[6], lam[6] = -1, 1.0
    a2[7], lam[7] = -1, 0.25
    lam[8] = 0.5
    return a, a2, lam, 0.1


def soft_reference(lgk, a, a2, lam, eps):
    """float64, from the kernel's own logits: per-sample loss and its bar, softmax, t, and the mask of the rows that count."""
    B, C = lgk.shape
    a2 = a.clone() if a2 is None else a2
    lam = torch.ones(B, dtype=torch.float64) if lam is None else lam.double()
    counts = (a >= 0) & (a < C) & ((lam == 1) | ((a2 >= 0) & (a2 < C)))
    ia, ib = a.clamp(0, C - 1), a2.clamp(0, C - 1)
    onehot = lambda i: torch.nn.functional.one_hot(i, C).double()  # noqa: E731
    second = torch.where(((a2 >= 0) & (a2 < C)).unsqueeze(1), onehot(ib), torch.zeros(B, C, dtype=torch.float64))
    t = (1 - eps) * (lam.unsqueeze(1) * onehot(ia) + (1 - lam).unsqueeze(1) * second) + eps / C
    mx = lgk.max(dim=1, keepdim=True).values
    lse = mx + torch.log(torch.exp(lgk - mx).sum(1, keepdim=True))
    per = (t * (lse - lgk)).sum(1)
    csum = (mx - lgk).sum(1)
    per_bound = CE_RTOL * per.abs().clamp(min=1.0) + gamma(C + 4) * (eps / C) * csum
    sm = torch.softmax(lgk, dim=1)
    zero = torch.zeros((), dtype=torch.float64)
    per, per_bound = torch.where(counts, per, zero), torch.where(counts, per_bound, zero)
    t = torch.where(counts.unsqueeze(1), t, zero)
    sm_c = torch.where(counts.unsqueeze(1), sm, zero)
    return per, per_bound, sm_c, t, counts


@functools.lru_cache(maxsize=None)
def inputs_of(name, regime):
    shape, phases, K = CASES[name]
    B, L1 = shape[:2]
    x, w, labels = make_inputs(shape, regime, seed=sum(shape) + 5 * REGIMES.index(regime) + K, K=K)
    bucket = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(B + K)) if K > 1 else None
    slabs = None
    if phases & hip.CLS_L1_SLABS_GIVEN:  # part[L1/64][B][L2], as the FeatureTransformer forward's epilogue leaves it
        l0 = l0_of(x.double(), True)
        slabs = torch.stack([l0[:, 64 * s:64 * s + 64] @ w[0][:, 64 * s:64 * s + 64].double().t() for s in range(L1 // 64)]).float()
    return x, w, labels, bucket, slabs


def run_step(name, regime, clip, labels, soft):
    """One call at the case's phases.  Returns the named outputs (d_logits, d_z1 out of scratch) on the device."""
    shape, phases, K = CASES[name]
    B, L1, L2, L3, C = shape
    x, w, _, bucket, slabs = inputs_of(name, regime)
    xd, wd, yd = to_dev(x, w, labels)
    plan = hip.bucket_group(bucket.to(DEV, torch.int32), 0, K) if K > 1 else None
    scratch = scratch_for(B, L1, L2, L3, C, K)
    scratch.fill_(0x7F)
    if slabs is not None:
        scratch[:slabs.numel() * 4].view(torch.float32).copy_(slabs.reshape(-1).to(DEV))
    if soft is not None:
        soft = tuple(t.to(DEV) if torch.is_tensor(t) else t for t in soft)
    lead = (K,) if K > 1 else ()
    grads = [torch.full(lead + s, float("nan"), device=DEV) for s in ((L2, L1), (L2,), (L3, L2), (L3,), (C, L3), (C,))]
    res = hip.classifier_train_step(xd, True, *wd, yd, GRAD_SCALE, clip, scratch=scratch, phases=phases, buckets=plan, grads=grads,
                                    soft=soft)
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


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", list(CASES))
def test_soft_train_step_against_float64(name, regime, kind):
    shape, phases, K = CASES[name]
    B, L1, L2, L3, C = shape
    clip = CLIP if (sum(shape) + TARGETS.index(kind)) % 2 else 0.0
    x, w, labels, bucket, _ = inputs_of(name, regime)
    a, a2, lam, eps = make_targets(kind, labels, C, seed=sum(shape) + TARGETS.index(kind))
    got = run_step(name, regime, clip, a, (a2, lam, eps))
    plain = run_step(name, regime, clip, a, None)
    tag = f"{name} {regime} {kind}"
    for nm in ("h1", "h2", "logits"):
        assert torch.equal(bits(got[nm]), bits(plain[nm])), f"{tag} {nm}: not the plain call's bits"
    if kind == "plain":  # eps = 0, lam = 1, labels_b = labels
        assert torch.equal(bits(got["sample_loss"]), bits(plain["sample_loss"])), f"{tag} sample loss: not the plain call's bits"
        if K == 1:
            assert torch.equal(bits(got["d_logits"]), bits(plain["d_logits"])), f"{tag} d_logits: not the plain call's bits"

    st = Stacks(B, K, bucket)
    w1, b1, w2, b2, w3, b3 = (c64(t) for t in w)
    h1k, h2k, lgk, dz1k = c64(got["h1"]), c64(got["h2"]), c64(got["logits"]), c64(got["d_z1"])
    per, per_bound, sm, t, counts = soft_reference(lgk, a, a2, lam, eps)
    assert_within(got["sample_loss"], per, per_bound, f"{tag} sample loss")
    assert not bool(got["sample_loss"].cpu()[~counts].any()), f"{tag}: an excluded row has a loss"
    scale = GRAD_SCALE / B
    dl = (sm - t) * scale
    dl_b = torch.where(counts.unsqueeze(1), CE_RTOL * (sm + t) * scale + TINY, torch.zeros((), dtype=torch.float64))
    if K == 1:
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


def test_fused_tail_with_and_without_dx_tiles_agree_bitwise():
    """phases 123 (the SOFT arm inside the d_x launch) against 59 (the tile tail alone, then the d_x launch)."""
    for c10, c64_ in (("tile10dx", "tile10"), ("tile64dx", "tile64")):
        _, _, labels, _, _ = inputs_of(c10, "randn")
        a, a2, lam, eps = make_targets("edges", labels, CASES[c10][0][4], seed=3)
        on, off = run_step(c10, "randn", CLIP, a, (a2, lam, eps)), run_step(c64_, "randn", CLIP, a, (a2, lam, eps))
        for nm in ("h1", "h2", "logits", "sample_loss", "d_logits", "d_z1", "d_x"):
            assert torch.equal(bits(on[nm]), bits(off[nm])), (c10, nm)


# ------------------------------------------------------------------------------------------------- the stand-alone loss
@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("C", (1, 2, 64, 65, 1000))
def test_cross_entropy_soft_against_float64(C, regime, kind):
    B = 37
    gen = torch.Generator().manual_seed(C + TARGETS.index(kind))
    logits = torch.randn(B, C, generator=gen) * 3
    labels = torch.randint(0, C, (B,), generator=gen)
    if regime == "tie":  # logits near 1e4, the runner-up 3 below the maximum
        logits = logits * 1e-3 - 5e3 - torch.arange(C, dtype=torch.float32)
        logits[:, 0] += 1.5e4
        if C > 1:
            logits[:, 1] += 1.5e4 - 2
    a, a2, lam, eps = make_targets(kind, labels, C, seed=C + 11)
    dev = lambda v: v.to(DEV) if torch.is_tensor(v) else v  # noqa: E731
    sample_loss, loss, d_logits = hip.cross_entropy_soft(dev(logits), dev(a), dev(a2), dev(lam), eps, grad_scale=GRAD_SCALE)
    fwd_only = hip.cross_entropy_soft(dev(logits), dev(a), dev(a2), dev(lam), eps, grad_scale=GRAD_SCALE, want_grad=False)
    torch.cuda.synchronize()
    tag = f"C={C} {regime} {kind}"
    per, per_bound, sm, t, counts = soft_reference(logits.double(), a, a2, lam, eps)
    assert_within(sample_loss, per, per_bound, f"{tag} sample loss")
    assert_within(loss.reshape(1), per.mean().reshape(1), per_bound.mean() + gamma(B + 2) * per.abs().mean(), f"{tag} mean loss")
    scale = GRAD_SCALE / B
    dl_b = torch.where(counts.unsqueeze(1), CE_RTOL * (sm + t) * scale + TINY, torch.zeros((), dtype=torch.float64))
    assert_within(d_logits, (sm - t) * scale, dl_b, f"{tag} d_logits")
    assert not bool(sample_loss.cpu()[~counts].any()) and not bool(d_logits.cpu()[~counts].any()), f"{tag}: an excluded row is not zero"
    assert fwd_only[2] is None
    assert torch.equal(bits(fwd_only[0]), bits(sample_loss)) and torch.equal(bits(fwd_only[1].reshape(1)), bits(loss.reshape(1)))
    if kind == "plain":
        ref = hip.cross_entropy(dev(logits), dev(a), grad_scale=GRAD_SCALE)
        assert torch.equal(bits(ref[0]), bits(sample_loss)) and torch.equal(bits(ref[2]), bits(d_logits)), f"{tag}: not nnue_cross_entropy's bits"
