"""Host-side contract of nnue_engine_stream_update (sparse add / remove lists on the engine's stream state): every invalid call
returns its NNUE_E_* code before anything is launched, so these run without a GPU."""
import ctypes

import pytest

from nnue_hip import lib
from nnue_hip.engine import _CModel, _CStacks

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4


def _model(g=4, oc=8, l1=256, l2=32, l3=16, classes=10, ptr=0):
    c = _CModel()
    c.num_features, c.l1, c.l2, c.l3, c.classes, c.grid, c.oc = g * g * oc, l1, l2, l3, classes, g, oc
    c.conv_scale, c.threshold, c.quantized_one, c.l1_scale, c.l2_scale, c.out_scale = 64.0, 0.0, 127.0, 64.0, 64.0, 16.0
    for k in ("conv_w", "conv_b", "ft_w", "ft_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(c, k, ptr)
    return c


def _stacks(ptr, scales):
    st = _CStacks()
    st.count = len(scales) // 3
    st.scales = ctypes.cast(scales, ctypes.POINTER(ctypes.c_float))
    for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(st, k, ptr)
    return st


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * (1 << 16))()  # 16-byte aligned host memory; never dereferenced by a rejected call
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15
    yield buf, p


def test_symbol_is_exported_and_bound_and_the_abi_version_stays():
    L = lib.load()
    assert "nnue_engine_stream_update" in lib.SIGNATURES
    assert hasattr(L, "nnue_engine_stream_update")
    assert hasattr(ctypes.CDLL(str(lib.LIB_PATH)), "nnue_engine_stream_update")
    assert L.nnue_hip_abi_version() == lib.ABI_VERSION == 39
    res, args = lib.SIGNATURES["nnue_engine_stream_update"]
    assert res is ctypes.c_int and len(args) == 18
    assert args[4] is ctypes.c_int64 and args[7] is ctypes.c_int64 and args[12] is ctypes.c_int64


def test_update_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    m = _model(ptr=p)
    S = 4
    need = L.nnue_engine_stream_state_bytes(ctypes.addressof(m), S)
    assert 0 < need <= (1 << 15)
    ok = dict(st=None, added=p, added_off=p, n_added=3, removed=p, removed_off=p, n_removed=2, S=S, rebuild=0, stack_in=None,
              state=p, state_bytes=need, logits=p, density=p, changed=p, stack_out=None)

    def call(model=m, **kw):
        a = dict(ok, **kw)
        mp = ctypes.addressof(model) if model is not None else None
        stp = ctypes.addressof(a["st"]) if a["st"] is not None else None
        return L.nnue_engine_stream_update(mp, stp, a["added"], a["added_off"], a["n_added"], a["removed"], a["removed_off"],
                                           a["n_removed"], a["S"], a["rebuild"], a["stack_in"], a["state"], a["state_bytes"],
                                           a["logits"], a["density"], a["changed"], a["stack_out"], None)

    # null model, state, outputs
    assert call(model=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(state=None) == E_ARG
    assert call(logits=None) == E_ARG
    assert call(density=None) == E_ARG
    assert call(changed=None) == E_ARG
    # S <= 0
    assert call(S=0) == E_ARG
    assert call(S=-2) == E_ARG
    # negative n
    assert call(n_added=-1) == E_ARG
    assert b"negative" in L.nnue_hip_last_error()
    assert call(n_removed=-5) == E_ARG
    assert call(n_added=-(1 << 40)) == E_ARG
    # n > 0 with a NULL id or offset pointer (n == 0 may pass both as NULL: only the later checks can refuse such a call)
    assert call(added=None) == E_ARG
    assert b"id and offset pointers" in L.nnue_hip_last_error()
    assert call(added_off=None) == E_ARG
    assert call(removed=None) == E_ARG
    assert call(removed_off=None) == E_ARG
    assert call(added=None, added_off=None, n_added=0, removed=None, removed_off=None, n_removed=0, state_bytes=need - 1) == E_SCRATCH
    # missing model tensor
    assert call(model=_model(ptr=0)) == E_ARG
    assert b"tensor missing" in L.nnue_hip_last_error()
    # st without stack_out; a bad stack count; a missing stack tensor
    scales = (ctypes.c_float * 6)(64.0, 64.0, 16.0, 64.0, 64.0, 16.0)
    st = _stacks(p, scales)
    assert call(st=st, stack_out=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    many = _stacks(p, scales)
    many.count = 65
    assert call(st=many, stack_out=p) == E_ARG
    assert call(st=_stacks(0, scales), stack_out=p) == E_ARG
    bad_scales = (ctypes.c_float * 6)(64.0, 64.0, 16.0, 64.0, 0.5, 16.0)
    assert call(st=_stacks(p, bad_scales), stack_out=p) == E_ARG
    assert b"scales" in L.nnue_hip_last_error()
    # state too small, and state misaligned
    assert call(state_bytes=need - 1) == E_SCRATCH
    assert b"state" in L.nnue_hip_last_error()
    assert call(st=st, stack_out=p, state_bytes=need - 16) == E_SCRATCH
    assert call(state=p + 8) == E_ARG
    assert b"aligned" in L.nnue_hip_last_error()
    # inconsistent model shapes and scales, as nnue_engine_stream_step
    bad = _model(ptr=p)
    bad.num_features += 1
    assert call(model=bad) == E_SHAPE
    bad = _model(ptr=p, l1=4096)
    assert call(model=bad, state_bytes=1 << 40) == E_SHAPE
    bad = _model(ptr=p)
    bad.l2_scale = 0.0
    assert call(model=bad) == E_ARG
    bad = _model(ptr=p)
    bad.conv_scale = 0.0
    assert call(model=bad) == E_ARG
    # a feature count whose bit words do not fit a workgroup's LDS
    big = _model(g=64, oc=128, ptr=p)
    assert call(model=big, state_bytes=1 << 40) == E_SHAPE
    assert b"LDS" in L.nnue_hip_last_error()
