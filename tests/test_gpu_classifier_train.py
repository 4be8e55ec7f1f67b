"""The fused classifier training step (nnue_classifier_train_step and its _bucketed form: layer-1 products, the per-sample
tail kernel with its softmax cross-entropy, the small weight-gradient tiles) against float64 torch on the CPU, fed exactly
the float32 inputs the kernel got.  Torch itself, not the oracle, so that the two cannot share a mistake.  ``-m gpu``.

Reference chain (K > 1: each sample through its own stack, indexed out of the stacked weights):
  l0 = cat(x_a * x_b, x_a) (pairwise) or x;  z1 = l0 W1^T + b1, h1 = act(z1);  z2 = h1 W2^T + b2, h2 = act(z2);
  logits = h2 W3^T + b3;  F.cross_entropy(logits, y) * grad_scale -> backward
with act = relu, or clamp(0, clip).  Every stage is formed from the kernel's OWN previous stage (h1 from l0, h2 from the
kernel's h1, the loss and d_logits from the kernel's logits, d_w1 / d_b1 / d_x from the kernel's d_z1), so that the
rounding of one stage or a gate flip at a pre-activation within rounding of 0 cannot compound into the next.  The gates
are taken from the kernel's own h, with torch's autograd rule: relu passes the gradient unless h <= 0, clamp only inside
(0, clip), both as a select.  (torch's clamp also passes it at z == 0 and z == clip, the kernel does not: documented, out
of scope; the inputs here are continuous random numbers and never sit on those boundaries.)

Bounds, element by element (never against a tensor's maximum, so a dropped, doubled or misplaced term fails even where
the element is small).  U = 2^-24, gamma_n = n U / (1 - n U); a sum of n float32 roundings in any order -- a serial fma
chain, a shuffle tree, split-K slabs, the f32 MFMA -- lies within gamma_n * sum|terms| of the exact sum, plus n * 2^-126
for products flushed below float32's smallest normal.
* h1, h2, logits: gamma_n * (|W| @ |in| + |b|), n = the dot length + the slab count (<= L1 / 16) + a few roundings (the
  pairwise product, the bias, the reduction tree).  act is 1-Lipschitz, so the bound carries through it.
* per-sample loss and mean loss: 1e-5 * max(1, |ref|) (the stand-alone loss kernel's bar; the mean takes the mean of the
  per-sample bars plus gamma_B of the sum).  d_logits: 1e-5 * (softmax + onehot) * grad_scale / B + 2^-126.
* d_z2 is not published: its bound is propagated, gate(d_bound @ |W3| + gamma_C * (|d_logits| + d_bound) @ |W3|); d_w3,
  d_b3 (from d_logits) and d_w2, d_b2 (from d_z2) carry their input's bound through the batch sum plus gamma_B of it.
* d_z1 (in scratch at nnue_classifier_train_dz1_offset, or grouped for K > 1) is checked against the bound propagated from
  d_z2 the same way, with gamma_L3.
* d_w1, d_b1 from the kernel's d_z1 with gamma_B (+ batch slabs); d_x with gamma_L2 through the pairwise backward.
Margin: in a dot of n like-sized terms one term is about sum|terms| / n, while the bound is gamma_n * sum|terms|, so a
dropped or doubled term is 1 / (n^2 U) times the bound: at the largest dot here (n ~ 1100 for L1 = B = 1024) that is
~14x; at the narrow layers it is thousands.
"""
import pytest
import torch
import torch.nn.functional as F

from nnue_hip import lib as hip

pytestmark = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
TINY = 2.0 ** -126  # float32's smallest normal
CE_RTOL = 1e-5
GRAD_SCALE = 0.5
CLIP = 0.75


def gamma(n: int) -> float:
    return n * U / (1 - n * U)


SHAPES = {  # B, L1, L2, L3, C
    "C1": (32, 64, 32, 8, 10),
    "C2": (512, 1024, 128, 32, 10),
    "C3k1": (1024, 1024, 128, 32, 100),
    "C4": (128, 1024, 128, 32, 1000),     # NT = 512 at C = 1000
    "B1": (1, 64, 32, 8, 10),
    "B37": (37, 256, 48, 16, 7),          # B % 16 != 0; d_w1 on the plain kernel (L2 % 32 != 0)
    "cls1": (20, 64, 32, 8, 1),
    "cls2": (20, 64, 32, 8, 2),
    "cls64": (64, 96, 48, 36, 64),        # wave reduction; L3 > 32: second j0 pass, kPre3 continuation, b2[j] read
    "cls65": (64, 96, 48, 36, 65),        # block reduction
    "cls256": (40, 128, 64, 16, 256),     # largest C on 128 threads
    "cls257": (40, 320, 160, 40, 257),    # NT = 512 with C != 1000; L2 > 128: the loop after the kPre2 prefetch
    "L3r17": (48, 128, 64, 17, 10),       # L3 >= 16 with a remainder in the d_z1 sum; not VEC
    "simple": (33, 24, 7, 5, 3),          # every first-layer product on the plain kernels
    "C2mis": (512, 1024, 128, 32, 10),    # w2 / w3 one float off 16-byte alignment: VEC = false on a VEC shape
}
REGIMES = ("randn", "spread", "tie")


# ------------------------------------------------------------------------------------------------- inputs
def dev_buf(src: torch.Tensor, offset: int = 0) -> torch.Tensor:
    """A device copy of src that starts `offset` floats into its own allocation (offset 1: 4-byte aligned only)."""
    base = torch.zeros(src.numel() + offset, device=DEV)
    out = base[offset:]
    out.copy_(src.reshape(-1))
    return out.view(src.shape)


def make_inputs(shape, regime, seed, K=1):
    """x, the six (stacked for K > 1) weights and labels, float32 on the CPU.
    randn: logits of about unit scale.  spread: W3 scaled so that a row's logits span ~80.  tie: logits at ~1e4 with the
    runner-up 3 below the maximum and the label on it (loss ~3 beside logits of 1e4)."""
    B, L1, L2, L3, C = shape
    gen = torch.Generator().manual_seed(seed)
    lead = (K,) if K > 1 else ()
    mk = lambda *s: torch.randn(*lead, *s, generator=gen) / (s[-1] ** 0.5)  # noqa: E731
    x = torch.randn(B, L1, generator=gen)
    w = [mk(L2, L1), mk(L2) * 0.1, mk(L3, L2), mk(L3) * 0.1, mk(C, L3), mk(C) * 0.1]
    labels = torch.randint(0, C, (B,), generator=gen)
    if regime == "spread":
        w[4] = w[4] * 25.0
    elif regime == "tie":
        w[4] = w[4] * 1e-3
        b3 = torch.full((C,), -5e3) - torch.arange(C, dtype=torch.float32)
        b3[0] = 1e4
        if C > 1:
            b3[1] = 1e4 - 3
        w[5] = b3.expand(*lead, C).clone()
        labels = torch.full((B,), min(1, C - 1), dtype=torch.int64)
    return x, w, labels


# ------------------------------------------------------------------------------------------------- float64 stacks
class Stacks:
    """Per-sample layer stacks in float64: K == 1 is one group holding every sample."""

    def __init__(self, B, K=1, bucket=None):
        self.B, self.K = B, K
        self.groups = [torch.arange(B)] if K == 1 else [torch.nonzero(bucket == k).flatten() for k in range(K)]

    def _w(self, W, k):
        return W if self.K == 1 else W[k]

    def fwd(self, inp, W, b=None):  # out[s] = W_s inp[s] (+ b_s)
        out = torch.zeros(inp.shape[0], W.shape[-2], dtype=torch.float64)
        for k, rows in enumerate(self.groups):
            if rows.numel():
                out[rows] = inp[rows] @ self._w(W, k).t() + (0 if b is None else self._w(b, k))
        return out

    def bwd(self, d, W):  # out[s] = d[s] W_s
        out = torch.zeros(d.shape[0], W.shape[-1], dtype=torch.float64)
        for k, rows in enumerate(self.groups):
            if rows.numel():
                out[rows] = d[rows] @ self._w(W, k)
        return out

    def wgrad(self, d, inp):  # G_k = sum over the samples of stack k of d[s]^T inp[s]
        out = torch.zeros((self.K,) + (d.shape[1], inp.shape[1]), dtype=torch.float64)
        for k, rows in enumerate(self.groups):
            out[k] = d[rows].t() @ inp[rows]
        return out[0] if self.K == 1 else out

    def bgrad(self, d):
        out = torch.zeros((self.K, d.shape[1]), dtype=torch.float64)
        for k, rows in enumerate(self.groups):
            out[k] = d[rows].sum(0)
        return out[0] if self.K == 1 else out


def act64(z, clip):
    return z.clamp(0, clip) if clip > 0 else torch.relu(z)


def gate64(d, h, clip):
    """torch's autograd rule through act at the kernel's activation h (select: a blocked NaN becomes 0)."""
    keep = ((h > 0) & (h < clip)) if clip > 0 else ~(h <= 0)
    return torch.where(keep, d, torch.zeros_like(d))


def l0_of(x64, pairwise):
    if not pairwise:
        return x64
    h = x64.shape[1] // 2
    return torch.cat([x64[:, :h] * x64[:, h:], x64[:, :h]], dim=1)


def c64(t):
    return t.detach().double().cpu()


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound element by element; non-finite elements must sit exactly where the reference has them."""
    got, ref = c64(got).reshape(-1), c64(ref).reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).cpu()
    bound = bound.reshape(-1) if bound.numel() == ref.numel() else bound.expand_as(ref)
    assert got.numel() == ref.numel(), f"{what}: {got.numel()} elements vs {ref.numel()}"
    fin_g, fin_r = torch.isfinite(got), torch.isfinite(ref)
    assert torch.equal(fin_g, fin_r), f"{what}: non-finite pattern differs at {int((fin_g != fin_r).sum())} of {ref.numel()} elements"
    err = (got - ref).abs()
    bad = fin_r & ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements outside the bound; first at {i}: "
                             f"got {float(got[i])!r} ref {float(ref[i])!r} bound {float(bound[i]):.3e}")


# ------------------------------------------------------------------------------------------------- the stage checks
def check_step(res, d_z1, x, pairwise, w, clip, labels, st, slabs=None, tag=""):
    """Every output of one training step against float64, stage by stage (module header).  res: what
    hip.classifier_train_step returned; d_z1: the kernel's d_z1 [B, L2] from scratch; slabs: [S, B, L2] layer-1 slabs
    handed in through phases bit 8 (None: the kernel formed them)."""
    (h1, h2, logits), (sample_loss, loss), d_x, grads = res
    B, L1 = x.shape
    w1, b1, w2, b2, w3, b3 = (c64(t) for t in w)
    L2, L3, C = w1.shape[-2], w2.shape[-2], w3.shape[-2]
    x64 = c64(x)
    l0 = l0_of(x64, pairwise)
    h1k, h2k, lgk, dz1k = c64(h1), c64(h2), c64(logits), c64(d_z1)
    y = labels.cpu()
    # forward, each stage from the kernel's previous one
    if slabs is None:
        z1 = st.fwd(l0, w1, b1)
        m1, n1 = st.fwd(l0.abs(), w1.abs(), b1.abs()), L1 + L1 // 16 + 4
    else:
        s64 = c64(slabs)
        z1 = s64.sum(0) + b1
        m1, n1 = s64.abs().sum(0) + b1.abs(), s64.shape[0] + 2
    assert_within(h1, act64(z1, clip), gamma(n1) * m1 + n1 * TINY, f"{tag} h1")
    n2 = L2 + 4
    assert_within(h2, act64(st.fwd(h1k, w2, b2), clip), gamma(n2) * st.fwd(h1k.abs(), w2.abs(), b2.abs()) + n2 * TINY, f"{tag} h2")
    n3 = L3 + 4
    assert_within(logits, st.fwd(h2k, w3, b3), gamma(n3) * st.fwd(h2k.abs(), w3.abs(), b3.abs()) + n3 * TINY, f"{tag} logits")
    # loss and d_logits from the kernel's logits
    per = F.cross_entropy(lgk, y, reduction="none")
    per_bound = CE_RTOL * per.abs().clamp(min=1.0)
    assert_within(sample_loss, per, per_bound, f"{tag} sample loss")
    assert_within(loss.reshape(1), per.mean().reshape(1), per_bound.mean() + gamma(B + 2) * per.abs().mean(), f"{tag} mean loss")
    sm = torch.softmax(lgk, dim=1)
    onehot = F.one_hot(y, C).double()
    scale = GRAD_SCALE / B
    dl = (sm - onehot) * scale
    dl_b = CE_RTOL * (sm + onehot) * scale + TINY
    # d_z2 (not published): propagated
    nC = C + 8
    dz2 = gate64(st.bwd(dl, w3), h2k, clip)
    dz2_b = gate64(st.bwd(dl_b, w3.abs()) + gamma(nC) * st.bwd(dl.abs() + dl_b, w3.abs()) + nC * TINY, h2k, clip)
    nB = B + 8

    def batch_bound(d, d_b, inp):  # the input's own bound through the batch sum + that sum's rounding
        return st.wgrad(d_b, inp.abs()) + gamma(nB) * st.wgrad(d.abs() + d_b, inp.abs()) + nB * TINY

    def bias_bound(d, d_b):
        return st.bgrad(d_b) + gamma(nB) * st.bgrad(d.abs() + d_b) + nB * TINY

    d_w1, d_b1, d_w2, d_b2, d_w3, d_b3 = grads
    assert_within(d_w3, st.wgrad(dl, h2k), batch_bound(dl, dl_b, h2k), f"{tag} d_w3")
    assert_within(d_b3, st.bgrad(dl), bias_bound(dl, dl_b), f"{tag} d_b3")
    assert_within(d_w2, st.wgrad(dz2, h1k), batch_bound(dz2, dz2_b, h1k), f"{tag} d_w2")
    assert_within(d_b2, st.bgrad(dz2), bias_bound(dz2, dz2_b), f"{tag} d_b2")
    # d_z1: propagated from d_z2
    nL3 = L3 + 4
    dz1 = gate64(st.bwd(dz2, w2), h1k, clip)
    dz1_b = gate64(st.bwd(dz2_b, w2.abs()) + gamma(nL3) * st.bwd(dz2.abs() + dz2_b, w2.abs()) + nL3 * TINY, h1k, clip)
    assert_within(d_z1, dz1, dz1_b, f"{tag} d_z1")
    # first layer from the kernel's own d_z1
    nW1 = B + B // 16 + 8
    if d_w1 is not None:
        assert_within(d_w1, st.wgrad(dz1k, l0), gamma(nW1) * st.wgrad(dz1k.abs(), l0.abs()) + nW1 * TINY, f"{tag} d_w1")
    assert_within(d_b1, st.bgrad(dz1k), gamma(nB) * st.bgrad(dz1k.abs()) + nB * TINY, f"{tag} d_b1")
    nL2 = L2 + 4
    d_l0, a_l0 = st.bwd(dz1k, w1), st.bwd(dz1k.abs(), w1.abs())
    if pairwise:
        h = L1 // 2
        xa, xb = x64[:, :h], x64[:, h:]
        ref_dx = torch.cat([d_l0[:, :h] * xb + d_l0[:, h:], d_l0[:, :h] * xa], dim=1)
        a_dx = torch.cat([a_l0[:, :h] * xb.abs() + a_l0[:, h:], a_l0[:, :h] * xa.abs()], dim=1)
    else:
        ref_dx, a_dx = d_l0, a_l0
    assert_within(d_x, ref_dx, gamma(nL2) * a_dx + nL2 * TINY, f"{tag} d_x")


def scratch_for(B, L1, L2, L3, C, K=1):
    return torch.empty((hip.classifier_train_scratch_bytes(B, L1, L2, L3, C, K),), dtype=torch.uint8, device=DEV)


def read_dz1(scratch, B, L1, L2, L3, C, pairwise):
    off = hip.classifier_train_dz1_offset(B, L1, L2, L3, C, pairwise)
    assert off >= 0 and off % 16 == 0 and off + B * L2 * 4 <= scratch.numel()
    return scratch[off:off + B * L2 * 4].view(torch.float32).view(B, L2)


def to_dev(x, w, labels, misaligned=False):
    wd = [t.to(DEV) for t in w]
    if misaligned:  # w2 and w3 one float off 16-byte alignment
        wd[2], wd[4] = dev_buf(w[2], 1), dev_buf(w[4], 1)
        assert wd[2].data_ptr() % 16 == 4 and wd[4].data_ptr() % 16 == 4
    return x.to(DEV), wd, labels.to(DEV)


# ------------------------------------------------------------------------------------------------- 1. one stack
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("clip", (0.0, CLIP))
@pytest.mark.parametrize("pairwise", (True, False))
@pytest.mark.parametrize("name", list(SHAPES))
def test_train_step_against_float64(name, pairwise, clip, regime):
    shape = SHAPES[name]
    B, L1, L2, L3, C = shape
    x, w, labels = make_inputs(shape, regime, seed=sum(shape) + 7 * REGIMES.index(regime) + int(pairwise) + (2 if clip else 0))
    xd, wd, yd = to_dev(x, w, labels, misaligned=name == "C2mis")
    scratch = scratch_for(B, L1, L2, L3, C)
    res = hip.classifier_train_step(xd, pairwise, *wd, yd, GRAD_SCALE, clip, scratch=scratch, phases=3)
    torch.cuda.synchronize()
    check_step(res, read_dz1(scratch, B, L1, L2, L3, C, pairwise), x, pairwise, w, clip, labels, Stacks(B), tag=name)


# ------------------------------------------------------------------------------------------------- 2. other paths
PHASE_SEQUENCES = ((1, 2), (5, 6), (7,), (17, 18), (19,))


@pytest.mark.parametrize("pairwise", (True, False))
@pytest.mark.parametrize("name", [n for n in SHAPES if n not in ("C3k1",)])
def test_phase_splits_are_bitwise_the_one_call(name, pairwise):
    """phases 1 -> 2, 5 -> 6, 7, 17 -> 18 and 19 against phases 3, bit for bit (d_w1 untouched where bit 16 leaves it
    to the FeatureTransformer backward)."""
    shape = SHAPES[name]
    B, L1, L2, L3, C = shape
    x, w, labels = make_inputs(shape, "randn", seed=sum(shape) + 11)
    xd, wd, yd = to_dev(x, w, labels, misaligned=name == "C2mis")

    def run(sequence):
        scratch = scratch_for(B, L1, L2, L3, C)
        keep = None
        for ph in sequence:
            kw = {} if keep is None else dict(out=keep[0], loss_out=keep[1], d_x=keep[2], grads=keep[3])
            if keep is None:
                kw["grads"] = [torch.full((L2, L1), 7.0, device=DEV)] + [torch.empty(s, device=DEV) for s in ((L2,), (L3, L2), (L3,), (C, L3), (C,))]
            keep = hip.classifier_train_step(xd, pairwise, *wd, yd, GRAD_SCALE, 0.0, scratch=scratch, phases=ph, **kw)
        return keep

    ref = run((3,))
    for seq in PHASE_SEQUENCES:
        got = run(seq)
        for a, r, nm in zip(got[0] + got[1] + (got[2],), ref[0] + ref[1] + (ref[2],), ("h1", "h2", "logits", "sample loss", "loss", "d_x")):
            assert torch.equal(a, r), (seq, nm)
        left = 16 & seq[0]
        assert torch.equal(got[3][0], torch.full_like(got[3][0], 7.0) if left else ref[3][0]), (seq, "d_w1")
        for a, r, nm in zip(got[3][1:], ref[3][1:], ("d_b1", "d_w2", "d_b2", "d_w3", "d_b3")):
            assert torch.equal(a, r), (seq, nm)


@pytest.mark.parametrize("clip", (0.0, CLIP))
@pytest.mark.parametrize("shape", ((64, 576, 64, 16, 10), (128, 1024, 128, 32, 10)), ids=("slabs9", "slabs16"))
def test_slabs_handed_in_through_phases_bit_8(shape, clip):
    """part[L1/64][B][L2] placed at the start of scratch (what the FeatureTransformer forward's epilogue leaves): 9 slabs
    run the 8-unrolled sum plus a remainder, 16 two full rounds."""
    B, L1, L2, L3, C = shape
    x, w, labels = make_inputs(shape, "randn", seed=B + L1)
    S = L1 // 64
    l0 = l0_of(x.double(), True)
    slabs = torch.stack([l0[:, 64 * s:64 * s + 64] @ w[0][:, 64 * s:64 * s + 64].double().t() for s in range(S)]).float()
    xd, wd, yd = to_dev(x, w, labels)
    scratch = scratch_for(B, L1, L2, L3, C)
    scratch[:S * B * L2 * 4].view(torch.float32).copy_(slabs.reshape(-1).to(DEV))
    res = hip.classifier_train_step(xd, True, *wd, yd, GRAD_SCALE, clip, scratch=scratch, phases=11)
    torch.cuda.synchronize()
    check_step(res, read_dz1(scratch, B, L1, L2, L3, C, True), x, True, w, clip, labels, Stacks(B), slabs=slabs, tag=f"S={S}")


BUCKET_SHAPES = {"K3": (96, 256, 32, 16, 10, 3), "K8": (200, 1024, 128, 32, 100, 8), "K3simple": (37, 24, 8, 5, 3, 3),
                 "K8big": (512, 1024, 128, 32, 10, 8)}


def draw_buckets(mix, B, K, gen):
    if mix == "one":
        return torch.full((B,), K // 2, dtype=torch.int64)
    if mix == "two":  # only two of the stacks ever see a sample
        return torch.where(torch.rand(B, generator=gen) < 0.3, 0, K - 1).long()
    return torch.randint(0, K, (B,), generator=gen)


@pytest.mark.parametrize("clip", (0.0, CLIP))
@pytest.mark.parametrize("mix", ("random", "one", "two"))
@pytest.mark.parametrize("name", list(BUCKET_SHAPES))
def test_bucketed_train_step_and_grouped_rows(name, mix, clip):
    """K stacks: phases 3 against float64 per-sample stacks; phases 17 (grouped mode) leaves x_g = x[rows[g]] bitwise and
    d_z1_g, with zeros on padding rows.  The stage checks of d_w1 / d_x read d_z1 from d_z1_g (for K > 1 the plain
    nnue_classifier_train_dz1_offset describes another layout)."""
    B, L1, L2, L3, C, K = BUCKET_SHAPES[name]
    shape = (B, L1, L2, L3, C)
    x, w, labels = make_inputs(shape, "randn", seed=B * 3 + K, K=K)
    bucket = draw_buckets(mix, B, K, torch.Generator().manual_seed(B + K))
    plan = hip.bucket_group(bucket.to(DEV, torch.int32), 0, K)
    xd, wd, yd = to_dev(x, w, labels)
    res = hip.classifier_train_step(xd, True, *wd, yd, GRAD_SCALE, clip, scratch=scratch_for(B, L1, L2, L3, C, K), phases=3,
                                    buckets=plan)
    scratch = scratch_for(B, L1, L2, L3, C, K)
    grp = hip.classifier_train_step(xd, True, *wd, yd, GRAD_SCALE, clip, scratch=scratch, phases=17, buckets=plan)
    torch.cuda.synchronize()
    for a, r, nm in zip(grp[0] + (grp[1][0], grp[2]), res[0] + (res[1][0], res[2]), ("h1", "h2", "logits", "sample loss", "d_x")):
        assert torch.equal(a, r), nm
    rows = plan.rows.cpu().long()
    R = rows.numel()
    dz_off, x_off = hip.classifier_train_grouped_offsets(B, L1, L2, L3, C, K)
    assert dz_off >= 0 and x_off >= 0 and dz_off % 16 == 0 and x_off % 16 == 0
    assert dz_off + R * L2 * 4 <= scratch.numel() and x_off + R * L1 * 4 <= scratch.numel()
    d_z1_g = scratch[dz_off:dz_off + R * L2 * 4].view(torch.float32).view(R, L2).cpu()
    x_g = scratch[x_off:x_off + R * L1 * 4].view(torch.float32).view(R, L1).cpu()
    real = rows >= 0
    assert sorted(rows[real].tolist()) == list(range(B))
    assert torch.equal(x_g[real], x[rows[real]])
    assert not bool(x_g[~real].any()) and not bool(d_z1_g[~real].any())
    d_z1 = torch.empty(B, L2)
    d_z1[rows[real]] = d_z1_g[real]
    check_step(res, d_z1, x, True, w, clip, labels, Stacks(B, K, bucket), tag=f"{name} {mix}")


# ------------------------------------------------------------------------------------------------- 3. non-finite inputs
def torch_autograd(x, pairwise, w, clip, labels):
    """The whole step in float64 autograd: what every output is, finite or not."""
    xs = x.double().requires_grad_()
    ps = [t.double().requires_grad_() for t in w]
    l0 = l0_of(xs, pairwise)
    h1 = act64(F.linear(l0, ps[0], ps[1]), clip)
    h2 = act64(F.linear(h1, ps[2], ps[3]), clip)
    logits = F.linear(h2, ps[4], ps[5])
    per = F.cross_entropy(logits, labels, reduction="none")
    loss = per.mean()
    (loss * GRAD_SCALE).backward()
    return [h1, h2, logits, per, loss, xs.grad] + [p.grad for p in ps]


@pytest.mark.parametrize("row", (0, 17))
@pytest.mark.parametrize("clip", (0.0, CLIP))
@pytest.mark.parametrize("pairwise", (True, False))
@pytest.mark.parametrize("name", ("C2", "simple"))
def test_nan_input_row_follows_torch(name, pairwise, clip, row):
    """A NaN in one sample's input: every output is non-finite exactly where float64 autograd's is (that sample's
    activations, logits, loss and d_x row; the mean loss; whichever weight gradients torch makes NaN), and every finite
    element stays within the bounds of the header."""
    shape = SHAPES[name]
    B, L1, L2, L3, C = shape
    x, w, labels = make_inputs(shape, "randn", seed=sum(shape) + row)
    x[row, 3] = float("nan")
    xd, wd, yd = to_dev(x, w, labels)
    scratch = scratch_for(B, L1, L2, L3, C)
    res = hip.classifier_train_step(xd, pairwise, *wd, yd, GRAD_SCALE, clip, scratch=scratch, phases=3)
    torch.cuda.synchronize()
    got = list(res[0]) + list(res[1]) + [res[2]] + list(res[3])
    names = ("h1", "h2", "logits", "sample loss", "loss", "d_x", "d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3")
    for g, r, nm in zip(got, torch_autograd(x, pairwise, w, clip, labels), names):
        fin_g, fin_r = torch.isfinite(c64(g)), torch.isfinite(r.detach())
        assert torch.equal(fin_g.reshape(-1), fin_r.reshape(-1)), f"{nm}: non-finite pattern differs from torch at {int((fin_g != fin_r).sum())} elements"
    bad_rows = lambda t: torch.nonzero(~torch.isfinite(c64(t)).all(1)).flatten().tolist()  # noqa: E731
    for t, nm in ((res[0][0], "h1"), (res[0][1], "h2"), (res[0][2], "logits")):
        assert bad_rows(t) == [row], nm
    assert set(bad_rows(res[2])) <= {row}, "d_x"  # (clip, no pairwise block: torch's d_x row is 0, finite)
    assert torch.nonzero(~torch.isfinite(res[1][0].cpu())).flatten().tolist() == [row]
    assert torch.isnan(res[1][1].cpu())
    check_step(res, read_dz1(scratch, B, L1, L2, L3, C, pairwise), x, pairwise, w, clip, labels, Stacks(B), tag=f"{name} NaN row {row}")
