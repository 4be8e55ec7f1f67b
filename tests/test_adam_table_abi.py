"""Host-side contract of the big table's Adam path (include/nnue_hip.h): nnue_adam_step_ext, nnue_ftm_backward_weight_update_adam
and nnue_ftm_backward_weight_update_forward_adam are exported, bound, cite the reference, and return their NNUE_E_* code for
every invalid call before anything is launched -- so these run without a GPU.  The pointers are host memory that a rejected
call never dereferences."""
import ctypes
import re

import pytest

from conftest import ROOT
from nnue_hip import lib

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4
NEW = ("nnue_adam_step_ext", "nnue_ftm_backward_weight_update_adam", "nnue_ftm_backward_weight_update_forward_adam")
BAD_BETAS = ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-3), (float("nan"), 0.999), (0.9, float("nan")))
BAD_EPS = (0.0, -1e-8, float("nan"))


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * (1 << 16))()
    p = (ctypes.addressof(buf) + 15) & ~15
    yield buf, p


def _last_error():
    return lib.load().nnue_hip_last_error()


def test_entry_points_are_exported_bound_and_cite_the_reference():
    header = (ROOT / "include" / "nnue_hip.h").read_text()
    raw = ctypes.CDLL(str(lib.LIB_PATH))
    for n in NEW:
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in lib.SIGNATURES, f"{n} is not bound"
        m = re.search(r"/\*((?:(?!/\*).)*?)\*/\s*int\s+" + n + r"\(", header, flags=re.S)
        assert m, f"{n}: no doc comment"
        assert re.search(r"train\.py:\d+", m.group(1)), f"{n}: comment cites no reference line"
    # argument counts of the bindings: the header's parameter lists
    for n in NEW:
        params = re.search(r"\bint\s+" + n + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(lib.SIGNATURES[n][1]) == params.count(",") + 1, n
    assert lib.load().nnue_hip_abi_version() == lib.ABI_VERSION >= 36


def test_adam_step_ext_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    count = 1000
    scratch_bytes = L.nnue_sgd_scratch(count)
    ok = dict(params=p, grads=p, m=p, v=p, counter=p, count=count, beta1=0.9, beta2=0.999, eps=1e-8, scratch=p,
              scratch_bytes=scratch_bytes, ext=None, ext_count=0, ext_lo=0, ext_hi=0, coef=None, applied=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nnue_adam_step_ext(a["params"], a["grads"], a["m"], a["v"], a["counter"], a["count"], 1e-3, a["beta1"], a["beta2"],
                                    a["eps"], 0.0, 1.0, 1.0, None, a["scratch"], a["scratch_bytes"], a["ext"], a["ext_count"],
                                    a["ext_lo"], a["ext_hi"], a["coef"], a["applied"], None, None)

    for name in ("params", "grads", "m", "v", "counter", "scratch"):
        assert call(**{name: None}) == E_ARG, name
        assert b"null pointer" in _last_error()
    assert call(count=0) == E_ARG
    for b1, b2 in BAD_BETAS:
        assert call(beta1=b1, beta2=b2) == E_ARG, (b1, b2)
        assert b"betas" in _last_error()
    for eps in BAD_EPS:
        assert call(eps=eps) == E_ARG, eps
    assert call(scratch_bytes=scratch_bytes - 1) == E_SCRATCH
    # ext_applied_elsewhere without coef_out, or without the producer's partials
    ext = dict(ext=p, ext_count=16, ext_lo=0, ext_hi=512)
    assert call(applied=1, **ext) == E_ARG
    assert b"coef_out" in _last_error()
    assert call(applied=1, coef=p) == E_ARG
    # ext range: bounds not multiples of 4 (hi may end the buffer unaligned), empty, outside [0, count]
    for lo, hi in ((2, 512), (4, 510), (0, 0), (512, 512), (512, 4), (-4, 512), (0, count + 4), (count, count + 4)):
        assert call(**dict(ext, ext_lo=lo, ext_hi=hi)) == E_ARG, (lo, hi)
        assert b"producer partials" in _last_error()
    for n in (0, 65537):
        assert call(**dict(ext, ext_count=n)) == E_ARG, n


def _update_args(p, **kw):
    a = dict(bits=p, d_out=p, B=128, F=8192, P=8192, L1=256, weight=p, m=p, v=p, coef=p, counter=p, beta1=0.9, beta2=0.999,
             eps=1e-8)
    a.update(kw)
    return a


def _update(L, a):
    return L.nnue_ftm_backward_weight_update_adam(a["bits"], a["d_out"], a["B"], a["F"], a["P"], a["L1"], a["weight"], a["m"], a["v"],
                                                  a["coef"], a["counter"], 1e-3, a["beta1"], a["beta2"], a["eps"], 2e-4, 1.0, None, None)


def _update_forward(L, a, p, **kw):
    b = dict(bits_next=p + 4096, sink_next=p, B_next=a["B"], bias=p, out_next=p, scratch=p, scratch_bytes=1 << 40)
    b.update(kw)
    return L.nnue_ftm_backward_weight_update_forward_adam(a["bits"], a["d_out"], a["B"], a["F"], a["P"], a["L1"], a["weight"], a["m"],
                                                          a["v"], a["coef"], a["counter"], 1e-3, a["beta1"], a["beta2"], a["eps"], 2e-4,
                                                          1.0, None, b["bits_next"], b["sink_next"], b["B_next"], b["bias"],
                                                          b["out_next"], b["scratch"], b["scratch_bytes"], None)


@pytest.mark.parametrize("fused", [False, True])
def test_table_update_rejects_bad_arguments_without_launching(host, fused):
    L = lib.load()
    _, p = host
    call = (lambda **kw: _update_forward(L, _update_args(p, **kw), p)) if fused else (lambda **kw: _update(L, _update_args(p, **kw)))
    for name in ("bits", "d_out", "weight", "m", "v", "coef", "counter"):
        assert call(**{name: None}) == E_ARG, name
        assert b"null pointer" in _last_error()
    # moment rows off a 16-byte boundary
    for name in ("m", "v"):
        assert call(**{name: p + 4}) == E_ARG, name
        assert b"16-byte aligned" in _last_error()
    assert call(weight=p + 4) == E_ARG
    for b1, b2 in BAD_BETAS:
        assert call(beta1=b1, beta2=b2) == E_ARG, (b1, b2)
        assert b"betas" in _last_error()
    for eps in BAD_EPS:
        assert call(eps=eps) == E_ARG, eps
    # sizes: non-positive, P / L1 not multiples of 4, B * L1 above 2^24
    assert call(B=0) == E_ARG
    assert call(L1=0) == E_ARG
    assert call(L1=254) == E_SHAPE
    assert call(P=8190) == E_SHAPE
    assert call(B=32768, L1=1024) == E_SHAPE
    assert b"2^24" in _last_error()


def test_fused_pass_rejects_its_own_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    a = _update_args(p)
    for name in ("bits_next", "sink_next", "bias", "out_next", "scratch"):
        assert _update_forward(L, a, p, **{name: None}) == E_ARG, name
        assert b"null pointer" in _last_error()
    # a launch-sized table is not a split-K forward; a next batch wider than one forward tile neither
    assert _update_forward(L, _update_args(p, B=512, F=800, P=968, L1=1024), p) == E_SHAPE
    assert b"split-K" in _last_error()
    assert _update_forward(L, a, p, B_next=256) == E_SHAPE
    if L.nnue_ftm_update_forward_supported(128, 128, 8192, 8192, 256):  # (a developer knob may take the forward off these tiles)
        assert _update_forward(L, a, p, bits_next=p) == E_ARG
        assert b"different buffers" in _last_error()
        assert _update_forward(L, a, p, scratch_bytes=16) == E_SCRATCH
        assert _update_forward(L, a, p, out_next=p + 4) == E_ARG
