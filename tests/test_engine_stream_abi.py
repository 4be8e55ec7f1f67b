"""Host-side contract of the engine's incremental entry points (nnue_engine_stream_state_bytes, nnue_engine_stream_step):
every invalid call returns its NNUE_E_* code before anything is launched, so these run without a GPU."""
import ctypes

import pytest

from nnue_hip import lib
from nnue_hip.engine import _CModel

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4


def _model(g=4, oc=8, l1=256, l2=32, l3=16, classes=10, ptr=0):
    c = _CModel()
    c.num_features, c.l1, c.l2, c.l3, c.classes, c.grid, c.oc = g * g * oc, l1, l2, l3, classes, g, oc
    c.conv_scale, c.threshold, c.quantized_one, c.l1_scale, c.l2_scale, c.out_scale = 64.0, 0.0, 127.0, 64.0, 64.0, 16.0
    for k in ("conv_w", "conv_b", "ft_w", "ft_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(c, k, ptr)
    return c


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * (1 << 16))()  # 16-byte aligned host memory; never dereferenced by a rejected call
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15
    yield buf, p


def _step(m, images, active, S, H, W, state, state_bytes, out, scratch, scratch_bytes):
    L = lib.load()
    mp = ctypes.addressof(m) if m is not None else None
    return L.nnue_engine_stream_step(mp, images, active, S, H, W, state, state_bytes, out, out, out, scratch, scratch_bytes, None)


def test_state_bytes_query():
    L = lib.load()
    m = _model()
    assert L.nnue_engine_stream_state_bytes(None, 4) == 0
    assert L.nnue_engine_stream_state_bytes(ctypes.addressof(m), 0) == 0
    assert L.nnue_engine_stream_state_bytes(ctypes.addressof(m), -3) == 0
    sizes = [L.nnue_engine_stream_state_bytes(ctypes.addressof(m), s) for s in (1, 2, 64, 1024)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    for g, oc, l1 in ((4, 8, 256), (10, 8, 1024), (32, 64, 512), (3, 5, 2)):
        m = _model(g=g, oc=oc, l1=l1)
        f = g * g * oc
        for s in (1, 7, 64, 1024):
            got = L.nnue_engine_stream_state_bytes(ctypes.addressof(m), s)
            assert got >= s * (2 * l1 + 2 * 8 * ((f + 63) // 64)), (g, oc, l1, s, got)
            assert got % 16 == 0
    small, big = _model(l1=256), _model(l1=512)
    assert L.nnue_engine_stream_state_bytes(ctypes.addressof(big), 16) > L.nnue_engine_stream_state_bytes(ctypes.addressof(small), 16)


def test_step_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    m = _model(ptr=p)
    S = 4
    need = L.nnue_engine_stream_state_bytes(ctypes.addressof(m), S)
    assert 0 < need <= (1 << 15)
    F = m.num_features
    ok = dict(images=p, active=None, S=S, H=32, W=32, state=p, state_bytes=need, out=p, scratch=p, scratch_bytes=S * F)

    def call(model=m, **kw):
        a = dict(ok, **kw)
        return _step(model, a["images"], a["active"], a["S"], a["H"], a["W"], a["state"], a["state_bytes"], a["out"],
                     a["scratch"], a["scratch_bytes"])

    # null model, state, outputs
    assert call(model=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(state=None) == E_ARG
    assert call(out=None) == E_ARG
    assert L.nnue_engine_stream_step(ctypes.addressof(m), p, None, S, 32, 32, p, need, p, None, p, p, S * F, None) == E_ARG
    assert L.nnue_engine_stream_step(ctypes.addressof(m), p, None, S, 32, 32, p, need, p, p, None, p, S * F, None) == E_ARG
    # exactly one of images / active
    assert call(active=p) == E_ARG
    assert b"exactly one" in L.nnue_hip_last_error()
    assert call(images=None) == E_ARG
    # missing model tensor
    assert call(model=_model(ptr=0)) == E_ARG
    # S <= 0
    assert call(S=0) == E_ARG
    assert call(S=-2) == E_ARG
    # state too small (also for the feature-map input)
    assert call(state_bytes=need - 1) == E_SCRATCH
    assert b"state" in L.nnue_hip_last_error()
    assert call(images=None, active=p, state_bytes=need - 16) == E_SCRATCH
    # scratch: missing or too small for images
    assert call(scratch_bytes=S * F - 1) == E_SCRATCH
    assert call(scratch=None) == E_ARG
    # the grid-overrun shape: the stride comes from H, so a wide image overruns the 4x4 grid buffer
    assert call(H=8, W=40) == E_SHAPE
    assert b"overruns" in L.nnue_hip_last_error()
    assert call(H=0) == E_ARG
    # inconsistent model shapes and scales, as nnue_engine_evaluate_logits
    bad = _model(ptr=p)
    bad.num_features = F + 1
    assert call(model=bad) == E_SHAPE
    bad = _model(ptr=p, l1=4096)
    assert call(model=bad, state_bytes=1 << 40) == E_SHAPE
    bad = _model(ptr=p)
    bad.l2_scale = 0.0
    assert call(model=bad) == E_ARG
    # state not 16-byte aligned
    assert call(state=p + 8) == E_ARG


def test_abi_version_and_bindings_agree():
    assert lib.load().nnue_hip_abi_version() == lib.ABI_VERSION
    for n in ("nnue_engine_stream_state_bytes", "nnue_engine_stream_step"):
        assert n in lib.SIGNATURES
        assert hasattr(lib.load(), n)
