"""The NULL-output forms include/nnue_hip.h allows: either output of nnue_ft_backward_weight / nnue_ftb_backward_weight /
nnue_ftm_backward_weight, d_x of nnue_classifier_backward[_bucketed] and nnue_classifier_train_step[_bucketed], d_logits of
nnue_cross_entropy.  ``-m gpu``.

For each form, at two shapes per kernel family: the requested outputs are BITWISE those of the all-outputs call (which is held to
its float64 bar here), they sit between NaN guard bands that stay NaN, and the forms the code refuses keep their error codes.
nnue_classifier_train_step composes other launches without d_x (no first-layer product beside d_x under phases bit 4, no small
gradients riding in the d_x launch under bit 16): phases 3, 7 and 19 at K = 1, 3 and 7 at K = 4."""
import pytest
import torch

import gather_forms as gf
import nnue_oracle as orc
from conftest import assert_close_grad
from nnue_hip import lib
from test_gpu_buckets import stacked
from test_gpu_gather_forms import Banded, features

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRADS = ("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3")


def same(a, b):
    return torch.equal(a.contiguous().view(torch.int32).reshape(-1), b.contiguous().view(torch.int32).reshape(-1))


# ------------------------------------------------------------------ FeatureTransformer weight gradients
def _list_call(case, c, feats):
    act, _ = feats
    return lambda **kw: lib.ft_backward_weight(c["d_out"].to(DEV), act, case.rows, **kw)


def _bits_call(case, c, feats):
    _, bits = feats
    return lambda **kw: lib.ftb_backward_weight(c["d_out"].to(DEV), bits, **kw)


def _ftm_call(case, c, feats):
    fm = lib.ftm_binarize(c["conv_out"].to(DEV), c["thr"].to(DEV), case.rows, case.l1)
    return lambda **kw: lib.ftm_backward_weight(c["d_out"].to(DEV), fm, **kw)


FT_FORMS = (  # family, case: two shapes per family, one of them with another kernel form
    ("list", "l300"), ("list", "l768"), ("list", "l1280"),          # simple / three-wave / tail-block weight kernels
    ("bits", "m1_split_sink"), ("bits", "m1_sw4_ring"), ("bits", "b_tiny"),  # split + ftb_finish_kernel<1>, unsplit ring, one slot
    ("mfma", "m1_split_sink"), ("mfma", "m1_sw2_one"),             # clamp sink row / table larger than the map
)


@pytest.mark.parametrize("family, name", FT_FORMS, ids=lambda v: v)
def test_ft_weight_gradient_with_one_output(family, name):
    case = gf.BY_NAME[name]
    c, ref = gf.inputs(case, False), gf.reference(case, False)
    feats = features(lib, case, c)
    call = dict(list=_list_call, bits=_bits_call, mfma=_ftm_call)[family](case, c, feats)
    f, l1 = case.rows, case.l1
    band = Banded()
    d_w, d_b = call(d_weight=band(f, l1), d_bias=band(l1))
    assert_close_grad(d_w, ref["d_w"], f"{family} {name} d_weight")
    assert_close_grad(d_b, ref["d_b"], f"{family} {name} d_bias")
    w_only, none_b = call(d_weight=band(f, l1), want_bias=False)
    none_w, b_only = call(d_bias=band(l1), want_weight=False)
    torch.cuda.synchronize()
    assert none_b is None and none_w is None
    assert same(w_only, d_w), "d_weight without d_bias differs from the all-outputs call"
    assert same(b_only, d_b), "d_bias without d_weight differs from the all-outputs call"
    # an unrequested buffer handed over all the same is not written
    spare_w, spare_b = band(f, l1), band(l1)
    call(d_weight=spare_w, d_bias=band(l1), want_weight=False)
    call(d_weight=band(f, l1), d_bias=spare_b, want_bias=False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(spare_w).all()) and bool(torch.isnan(spare_b).all())
    assert band.untouched(), "a guard band was written"
    with pytest.raises(lib.NnueHipError, match=r"code -1\).*both outputs are null"):
        call(want_weight=False, want_bias=False)


# ------------------------------------------------------------------ classifier
def cls_case(shape, K=1):
    b, l1, l2, l3, c = shape
    gen = torch.Generator().manual_seed(sum(shape) + 31 * K)
    x = torch.randn(b, l1, generator=gen)
    if K == 1:
        mk = lambda *s: torch.randn(*s, generator=gen) / (s[-1] ** 0.5)  # noqa: E731
        p = [mk(l2, l1), mk(l2) * 0.1, mk(l3, l2), mk(l3) * 0.1, mk(c, l3), mk(c) * 0.1]
        bucket, plan = None, None
    else:
        p = stacked(K, l1, l2, l3, c, gen)
        bucket = torch.randint(0, K, (b,), generator=gen)
        plan = lib.bucket_group(bucket.to(DEV, torch.int32), 0, K)
    labels = torch.randint(0, c, (b,), generator=gen)
    up = torch.randn(b, c, generator=gen)
    return x, p, labels, up, bucket, plan


def replay(l0, p64, h1, h2, up, bucket, K):
    """The six gradients in float64 with the gates taken from the kernel's own activations (a pre-activation within rounding of
    zero may gate either way; tests/test_gpu_kernels.py holds the backward to the same contract)."""
    h1d, h2d, u = h1.cpu().double(), h2.cpu().double(), up.double()

    def one(w, rows):
        d_z2 = (u[rows] @ w[4]) * (h2d[rows] > 0)
        d_z1 = (d_z2 @ w[2]) * (h1d[rows] > 0)
        return [d_z1.t() @ l0[rows], d_z1.sum(0), d_z2.t() @ h1d[rows], d_z2.sum(0), u[rows].t() @ h2d[rows], u[rows].sum(0)]

    if K == 1:
        return one(p64, slice(None))
    per = [one([t[k] for t in p64], (bucket == k).nonzero().flatten()) for k in range(K)]
    return [torch.stack([per[k][i] for k in range(K)]) for i in range(6)]


def banded_grads(band, shape, K):
    _, l1, l2, l3, c = shape
    lead = (K,) if K > 1 else ()
    return [band(*lead, *s) for s in ((l2, l1), (l2,), (l3, l2), (l3,), (c, l3), (c,))]


CLS_FORMS = (((33, 256, 48, 16, 7), 1), ((5, 24, 7, 5, 3), 1), ((512, 1024, 128, 32, 10), 1),  # MFMA products / the simple kernels / C2
             ((96, 256, 32, 16, 10), 4), ((37, 24, 7, 5, 3), 4))


@pytest.mark.parametrize("shape, K", CLS_FORMS, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("pairwise", (True, False), ids=("pairwise", "plain"))
def test_classifier_backward_without_d_x(shape, K, pairwise):
    x, p, _, up, bucket, plan = cls_case(shape, K)
    xd, pd, upd = x.to(DEV), [t.to(DEV) for t in p], up.to(DEV)
    h1, h2, _ = lib.classifier_forward(xd, pairwise, *pd, 0.0, buckets=plan)
    band = Banded()
    d_x, full = lib.classifier_backward(xd, pairwise, pd[0], pd[2], pd[4], h1, h2, upd, 0.0, grads=banded_grads(band, shape, K),
                                        d_x=band(*x.shape), buckets=plan)
    none, got = lib.classifier_backward(xd, pairwise, pd[0], pd[2], pd[4], h1, h2, upd, 0.0, want_dx=False,
                                        grads=banded_grads(band, shape, K), buckets=plan)
    spare = band(*x.shape)  # a d_x buffer that is not asked for stays as it is
    lib.classifier_backward(xd, pairwise, pd[0], pd[2], pd[4], h1, h2, upd, 0.0, want_dx=False, d_x=spare,
                            grads=banded_grads(band, shape, K), buckets=plan)
    torch.cuda.synchronize()
    assert none is None and bool(torch.isnan(spare).all()) and not bool(torch.isnan(d_x).any())
    for name, a, r in zip(GRADS, got, full):
        assert same(a, r), f"{name} without d_x differs from the all-outputs call"
    assert band.untouched(), "a guard band was written"
    # the all-outputs call against float64, gates from the kernel's own activations (as tests/test_gpu_kernels.py does)
    x64, p64 = x.double(), [t.double() for t in p]
    l0 = orc.pairwise(x64) if pairwise else x64
    want = replay(l0, p64, h1, h2, up, bucket, K)
    for name, a, r in zip(GRADS, full, want):
        assert_close_grad(a, r, name)


def train_step(shape, K, case, phases, want_dx, band):
    x, p, labels, _, _, plan = case
    b, l1, l2, l3, c = shape
    scratch = band.bytes(lib.classifier_train_scratch_bytes(b, l1, l2, l3, c, K))
    grads = banded_grads(band, shape, K)
    if phases & 16:
        grads[0].fill_(7.0)  # left to another launch's rider: must stay as it is
    out = (band(b, l2), band(b, l3), band(b, c))
    loss_out = (band(b), band(1).view(()))
    return lib.classifier_train_step(x.to(DEV), True, *[t.to(DEV) for t in p], labels.to(DEV), 0.5, 0.0, want_dx=want_dx, scratch=scratch,
                                     out=out, loss_out=loss_out, grads=grads, d_x=band(b, l1) if want_dx else None, phases=phases, buckets=plan)


class BandedBytes(Banded):
    def bytes(self, n):
        """A 16-byte aligned uint8 scratch of n bytes between NaN bands."""
        return self((n + 3) // 4).view(torch.uint8)[:n]


TRAIN_FORMS = ([(s, 1, ph) for s in ((512, 1024, 128, 32, 10), (33, 256, 48, 16, 7), (5, 24, 7, 5, 3)) for ph in (3, 7, 19)]
               + [(s, 4, ph) for s in ((96, 256, 32, 16, 10), (37, 24, 7, 5, 3)) for ph in (3, 7)])


@pytest.mark.parametrize("shape, K, phases", TRAIN_FORMS, ids=lambda v: str(v).replace(" ", ""))
def test_classifier_train_step_without_d_x(shape, K, phases):
    case = cls_case(shape, K)
    band = BandedBytes()
    (h1, h2, logits), (sample, loss), d_x, grads = train_step(shape, K, case, phases, True, band)
    (g1, g2, glog), (gsample, gloss), none, ggrads = train_step(shape, K, case, phases, False, band)
    torch.cuda.synchronize()
    assert none is None and not bool(torch.isnan(d_x).any())
    for name, a, r in zip(("h1", "h2", "logits", "sample_loss", "loss") + GRADS, (g1, g2, glog, gsample, gloss, *ggrads),
                          (h1, h2, logits, sample, loss, *grads)):
        assert not bool(torch.isnan(r).any()), f"{name} of the all-outputs call holds NaN"
        assert same(a, r), f"phases {phases}: {name} without d_x differs from the all-outputs call"
    if phases & 16:
        assert bool((ggrads[0] == 7.0).all()) and bool((grads[0] == 7.0).all())  # d_w1 belongs to the rider
    assert band.untouched(), "a guard band was written"
    # the all-outputs call against float64 (loss and the gradients that this call forms)
    x, p, labels, _, bucket, _ = case
    l0, p64 = orc.pairwise(x.double()), [t.double() for t in p]
    ref_logits = orc.classifier_forward(l0, *p64) if K == 1 else orc.classifier_forward_bucketed(l0, bucket, *p64, None)
    ref_loss, d_logits = orc.cross_entropy_backward(ref_logits, labels)
    want = replay(l0, p64, h1, h2, d_logits * 0.5, bucket, K)
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss)))
    for name, a, r in list(zip(GRADS, grads, want))[1 if phases & 16 else 0:]:
        assert_close_grad(a, r, name)


def test_the_forms_that_need_d_x_are_refused():
    """phases bit 32 hands the small gradients to another launch's rider, which presumes the d_x launch: NNUE_E_SHAPE without d_x,
    for 51 = 1 | 2 | 16 | 32 and for 123 (the tail inside the d_x launch)."""
    shape = (512, 1024, 128, 32, 10)
    case = cls_case(shape)
    for phases in (51, 123):
        with pytest.raises(lib.NnueHipError, match=r"code -2\).*phases bit 32"):
            train_step(shape, 1, case, phases, False, BandedBytes())
    # bit 4 alone (no phase) stays an argument error with or without d_x
    with pytest.raises(lib.NnueHipError, match=r"code -1\)"):
        train_step(shape, 1, case, 4, False, BandedBytes())


# ------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("b, c", ((512, 10), (7, 1000), (1, 1)))
def test_cross_entropy_without_d_logits(b, c):
    gen = torch.Generator().manual_seed(b + c)
    logits = torch.randn(b, c, generator=gen) * 3
    labels = torch.randint(0, c, (b,), generator=gen)
    band = Banded()
    sample, loss, d = lib.cross_entropy(logits.to(DEV), labels.to(DEV), 0.5, out=(band(b), band(1).view(()), band(b, c)))
    s2, l2, none = lib.cross_entropy(logits.to(DEV), labels.to(DEV), 0.5, want_grad=False)
    s3, l3, _ = lib.cross_entropy(logits.to(DEV), labels.to(DEV), 0.5, out=(band(b), band(1).view(()), None))
    torch.cuda.synchronize()
    assert none is None and same(s2, sample) and same(l2, loss) and same(s3, sample) and same(l3, loss)
    assert band.untouched(), "a guard band was written"
    ref_loss, ref_d = orc.cross_entropy_backward(logits.double(), labels)
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
    assert_close_grad(d, ref_d * 0.5, "d_logits")
