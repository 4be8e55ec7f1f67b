"""Host-side contract of the loss, metric and optimizer entry points (optim_kernels.hip): every invalid call returns its
NNUE_E_* code before anything is launched, so these run without a GPU.  The pointers are host memory that a rejected
call never dereferences."""
import ctypes

import pytest

from nnue_hip import lib

E_ARG, E_SCRATCH = -1, -4


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * (1 << 16))()
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15
    yield buf, p


def _last_error():
    return lib.load().nnue_hip_last_error()


def test_sgd_step_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    count = 1000
    scratch_bytes = L.nnue_sgd_scratch(count)
    assert scratch_bytes > 0
    ok = dict(params=p, grads=p, mom=p, count=count, lr=0.1, momentum=0.9, wd=0.0, max_norm=1.0, scale=1.0, first=1, norm=p,
              scratch=p, scratch_bytes=scratch_bytes, ste_partial=None, ste_chunks=0, ste_fps=0, ste_thr=None, ste_w=None,
              ext=None, ext_count=0, ext_lo=0, ext_hi=0, coef=None, applied=0, lr_dev=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nnue_sgd_step(a["params"], a["grads"], a["mom"], a["count"], a["lr"], a["momentum"], a["wd"], a["max_norm"],
                               a["scale"], a["first"], a["norm"], a["scratch"], a["scratch_bytes"], a["ste_partial"],
                               a["ste_chunks"], a["ste_fps"], a["ste_thr"], a["ste_w"], a["ext"], a["ext_count"], a["ext_lo"],
                               a["ext_hi"], a["coef"], a["applied"], a["lr_dev"], None)

    assert call(params=None) == E_ARG
    assert b"null pointer" in _last_error()
    assert call(scratch=None) == E_ARG
    assert call(count=0) == E_ARG
    # momentum without a buffer
    assert call(mom=None) == E_ARG
    assert b"momentum buffer" in _last_error()
    # scratch below nnue_sgd_scratch
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
    # ext_count out of (0, 65536]
    for n in (0, 65537):
        assert call(**dict(ext, ext_count=n)) == E_ARG, n
    # deferred STE sums: fps * 28 above 4096, outputs not the first elements of grads, ext below the STE outputs
    fps = 8
    ste = dict(ste_partial=p, ste_chunks=4, ste_fps=fps, ste_thr=p, ste_w=p + 4 * 8)
    assert call(**dict(ste, ste_fps=147)) == E_ARG
    assert b"fps * 28" in _last_error()
    assert call(**dict(ste, ste_chunks=0)) == E_ARG
    assert call(**dict(ste, ste_thr=None)) == E_ARG
    assert call(**dict(ste, ste_thr=p + 64, ste_w=p + 64 + 4 * 8)) == E_ARG
    assert b"first elements of grads" in _last_error()
    assert call(**dict(ste, ext=p, ext_count=16, ext_lo=0, ext_hi=512)) == E_ARG
    assert b"first elements of grads" in _last_error()
    assert call(**dict(ste, count=16)) == E_ARG  # the outputs do not fit in grads


def test_adam_step_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    count = 1000
    scratch_bytes = L.nnue_sgd_scratch(count)

    def call(params=p, count=count, beta1=0.9, beta2=0.999, eps=1e-8, scratch_bytes=scratch_bytes, counter=p):
        return L.nnue_adam_step(params, p, p, p, counter, count, 1e-3, beta1, beta2, eps, 0.0, 1.0, 1.0, None, p, scratch_bytes,
                                None, None)

    assert call(params=None) == E_ARG
    assert call(counter=None) == E_ARG
    assert call(count=0) == E_ARG
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-3), (float("nan"), 0.999), (0.9, float("nan"))):
        assert call(beta1=b1, beta2=b2) == E_ARG, (b1, b2)
        assert b"betas" in _last_error()
    for eps in (0.0, -1e-8, float("nan")):
        assert call(eps=eps) == E_ARG, eps
    assert call(scratch_bytes=scratch_bytes - 1) == E_SCRATCH


def test_sqnorm_partials_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    for nparts in (0, 65537, -1):
        assert L.nnue_sqnorm_partials(p, 1000, p, nparts, None) == E_ARG, nparts
        assert b"out of range" in _last_error()
    assert L.nnue_sqnorm_partials(p, 0, p, 64, None) == E_ARG
    assert L.nnue_sqnorm_partials(None, 1000, p, 64, None) == E_ARG


def test_loss_and_confusion_reject_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    for b, c in ((0, 10), (10, 0), (-1, 10), (10, -1)):
        assert L.nnue_cross_entropy(p, p, b, c, 1.0, p, p, p, None) == E_ARG, (b, c)
        assert b"must be positive" in _last_error()
        assert L.nnue_confusion_accumulate(p, p, b, c, p, None) == E_ARG, (b, c)
        assert b"must be positive" in _last_error()
    assert L.nnue_cross_entropy(p, p, 4, 10, 1.0, None, p, p, None) == E_ARG
    assert L.nnue_confusion_accumulate(p, p, 4, 10, None, None) == E_ARG
