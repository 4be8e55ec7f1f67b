"""Every kernel instantiation of the two gather families (tests/gather_forms.py lists them and the case that launches each) against
the float64 oracle.  ``-m gpu``.

Exact operands (small dyadic rationals: every partial sum in any order is a float32 number): the forward, the weight and bias
gradients and the value gradient EQUAL the float64 reference.  randn operands: the suite's logits / gradient bars, and per element
|got - ref| <= n * 2^-23 * sum |terms| (n terms: a row whose terms are all small has a small bound of its own, an element without
terms must be 0).  Bits-family results agree with the list kernels on the same batch; every result is bitwise reproducible; every
output is an interior view of a NaN-filled buffer whose bands must stay NaN, so an element left unwritten fails both comparisons."""
import pytest
import torch

import gather_forms as gf
from conftest import assert_close_grad, assert_close_logits

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASE_ID = lambda c: c.name  # noqa: E731
BITS_CASES = [c for c in gf.CASES if c.bits]


@pytest.fixture(scope="module")
def hip():
    from nnue_hip import lib
    lib.load()
    return lib


class Banded:
    """NaN-filled outputs as interior views (16-byte aligned) of NaN-filled buffers, 64 rows + 256 floats deep on either side."""

    def __init__(self):
        self.bufs = []

    def __call__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        band = (64 * shape[-1] + 256 + 3) // 4 * 4
        buf = torch.full((n + 2 * band,), float("nan"), device=DEV)
        self.bufs.append((buf, band, n))
        view = buf[band:band + n].view(shape)
        assert view.data_ptr() % 16 == 0
        return view

    def untouched(self):
        return all(bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[band + n:]).all()) for buf, band, n in self.bufs)


def features(hip, case, c):
    """The act list of a case and, where the bits family takes it, its bit form."""
    if case.kind == "prepare":
        return hip.ft_prepare(c["idx"].to(DEV), c["val"].to(DEV), case.rows), None
    x, thr = c["conv_out"].to(DEV), c["thr"].to(DEV)
    return hip.binarize_features(x, thr, case.rows), (hip.binarize_bits(x, thr, case.rows, case.l1) if case.bits else None)


def run_list(hip, case, c, act):
    """The four list-family results into banded outputs: dict(out, d_w, d_b, d_val)."""
    b, f, l1, m = case.batch, case.rows, case.l1, case.positions
    w, bias, d_out = (c[k].to(DEV) for k in ("weight", "bias", "d_out"))
    band = Banded()
    r = dict(out=hip.ft_forward(w, bias, act, out=band(b, l1)))
    r["d_w"], r["d_b"] = hip.ft_backward_weight(d_out, act, f, d_weight=band(f, l1), d_bias=band(l1))
    r["d_val"] = hip.ft_backward_values(d_out, w, act, m, dst=band(b, m))
    torch.cuda.synchronize()
    assert band.untouched(), f"{case.name}: a list kernel wrote into a guard band"
    return r


def run_bits(hip, case, c, bits):
    b, f, l1, p = case.batch, case.rows, case.l1, case.positions
    w, bias, d_out = (c[k].to(DEV) for k in ("weight", "bias", "d_out"))
    band = Banded()
    r = dict(out=hip.ftb_forward(w, bias, bits, out=band(b, l1)))
    r["d_w"], r["d_b"] = hip.ftb_backward_weight(d_out, bits, d_weight=band(f, l1), d_bias=band(l1))
    r["d_val"] = hip.ftb_backward_values(d_out, w, bits, dst=band(b, p))
    torch.cuda.synchronize()
    assert band.untouched(), f"{case.name}: a bits kernel wrote into a guard band"
    return r


def assert_equal_ref(got, ref, what):
    for k in ("out", "d_w", "d_b", "d_val"):
        g = got[k].cpu().double()
        differ = int((g != ref[k]).sum())  # NaN (never written) differs from everything
        assert differ == 0, f"{what}: {k} differs from the float64 value in {differ} of {g.numel()} elements"


def assert_within_bars(got, ref, what):
    assert_close_logits(got["out"], ref["out"], f"{what} out")
    for k in ("d_w", "d_b", "d_val"):
        assert_close_grad(got[k], ref[k], f"{what} {k}")
    for k in ("out", "d_w", "d_b", "d_val"):
        err = (got[k].cpu().double() - ref[k]).abs()
        bound = gf.term_bound(ref, k)
        bad = ~(err <= bound)  # NaN fails
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"{what} {k}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
        assert not bool(bad.any()), f"{what}: {k} has {int(bad.sum())} elements past n * 2^-23 * sum|terms| (worst ratio {worst:.3f})"


def same_bits(a, b):
    return all(torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)) for k in a)


@pytest.mark.parametrize("case", gf.CASES, ids=CASE_ID)
def test_list_kernels_are_exact_on_exact_operands(hip, case):
    c, ref = gf.inputs(case, True), gf.reference(case, True)
    act, _ = features(hip, case, c)
    assert torch.equal(act.n.cpu().long(), ref["n"])
    assert_equal_ref(run_list(hip, case, c, act), ref, f"{case.name} list")


@pytest.mark.parametrize("case", BITS_CASES, ids=CASE_ID)
def test_bits_kernels_are_exact_on_exact_operands(hip, case):
    c, ref = gf.inputs(case, True), gf.reference(case, True)
    _, bits = features(hip, case, c)
    assert torch.equal(bits.n.cpu().long(), ref["n"])
    assert_equal_ref(run_bits(hip, case, c, bits), ref, f"{case.name} bits")


@pytest.mark.parametrize("case", gf.CASES, ids=CASE_ID)
def test_list_kernels_meet_the_bars_and_the_term_bound(hip, case):
    c, ref = gf.inputs(case, False), gf.reference(case, False)
    act, _ = features(hip, case, c)
    got = run_list(hip, case, c, act)
    assert_within_bars(got, ref, f"{case.name} list")
    again = run_list(hip, case, c, features(hip, case, c)[0])  # from a fresh list: nnue_ft_prepare's atomics included
    assert same_bits(got, again), f"{case.name}: the list kernels are not bitwise reproducible"


@pytest.mark.parametrize("case", BITS_CASES, ids=CASE_ID)
def test_bits_kernels_meet_the_bars_and_agree_with_the_list_kernels(hip, case):
    c, ref = gf.inputs(case, False), gf.reference(case, False)
    act, bits = features(hip, case, c)
    got = run_bits(hip, case, c, bits)
    assert_within_bars(got, ref, f"{case.name} bits")
    lst = run_list(hip, case, c, act)
    assert_close_logits(got["out"], lst["out"], f"{case.name} bits vs list forward")
    for k in ("d_w", "d_b", "d_val"):
        assert_close_grad(got[k], lst[k], f"{case.name} bits vs list {k}")
    assert bool((got["d_val"].cpu()[ref["abs"]["d_val"] == 0] == 0).all())  # inactive positions: written, and zero
    assert same_bits(got, run_bits(hip, case, c, bits)), f"{case.name}: the bits kernels are not bitwise reproducible"
