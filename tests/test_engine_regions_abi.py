"""Host-side contract of nnue_engine_stream_step_u8_regions (the stream step from the dirty rectangles of uint8 frames):
exported, bound, documented, and every invalid call returns its NNUE_E_* code before anything is launched, so these run
without a GPU.  The pointers handed over are host memory that a rejected call never dereferences; a call that passes the check
under test is stopped by a state buffer one byte short (NNUE_E_SCRATCH), which is checked after it."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from nnue_hip import lib
from nnue_hip.engine import _CModel, _CStacks, _CU8Frames, pack_rect_lists, u8_constants

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4
NAME = "nnue_engine_stream_step_u8_regions"
S, H, W = 4, 32, 32


def _model(g=4, oc=8, l1=256, l2=32, l3=16, classes=10, ptr=0):
    c = _CModel()
    c.num_features, c.l1, c.l2, c.l3, c.classes, c.grid, c.oc = g * g * oc, l1, l2, l3, classes, g, oc
    c.conv_scale, c.threshold, c.quantized_one, c.l1_scale, c.l2_scale, c.out_scale = 64.0, 0.0, 127.0, 64.0, 64.0, 16.0
    for k in ("conv_w", "conv_b", "ft_w", "ft_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(c, k, ptr)
    return c


def _frames(p, count=S, indices=None, layout=1):
    s = _CU8Frames()
    s.data, s.indices, s.count, s.layout = p, indices, count, layout
    mean255, inv_std255 = u8_constants()
    s.mean255[:], s.inv_std255[:] = mean255.tolist(), inv_std255.tolist()
    return s


def _stacks(ptr, count=2):
    st = _CStacks()
    st.count = count
    scales = (ctypes.c_float * 6)(64.0, 64.0, 16.0, 64.0, 64.0, 16.0)
    st.scales = ctypes.cast(scales, ctypes.POINTER(ctypes.c_float))
    st._keep = scales
    for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(st, k, ptr)
    return st


@pytest.fixture(scope="module")
def call():
    """call(**overrides) -> the return code on otherwise valid arguments (which alone would launch: every use overrides)."""
    L = lib.load()
    buf = (ctypes.c_uint8 * (1 << 16))()
    p = (ctypes.addressof(buf) + 15) & ~15
    m = _model(ptr=p)
    need = L.nnue_engine_stream_state_bytes(ctypes.addressof(m), S)
    assert 0 < need <= (1 << 15)
    ok = dict(model=m, st=None, src=_frames(p), S=S, H=H, W=W, rects=p, rect_off=p, n_rects=3, stack_in=None, state=p,
              state_bytes=need, logits=p, density=p, changed=p, stack_out=None)

    def run(**kw):
        assert kw, "a call with valid arguments would launch"
        a = dict(ok, **kw)
        mp = ctypes.addressof(a["model"]) if a["model"] is not None else None
        stp = ctypes.addressof(a["st"]) if a["st"] is not None else None
        sp = ctypes.addressof(a["src"]) if a["src"] is not None else None
        return L.nnue_engine_stream_step_u8_regions(mp, stp, sp, a["S"], a["H"], a["W"], a["rects"], a["rect_off"], a["n_rects"],
                                                    a["stack_in"], a["state"], a["state_bytes"], a["logits"], a["density"],
                                                    a["changed"], a["stack_out"], None)

    run.p, run.need, run.keep = p, need, buf
    return run


def test_symbol_is_exported_bound_and_documented():
    L = lib.load()
    assert NAME in lib.SIGNATURES
    assert hasattr(L, NAME) and hasattr(ctypes.CDLL(str(lib.LIB_PATH)), NAME)
    res, args = lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 17
    assert args[8] is ctypes.c_int64 and args[11] is ctypes.c_int64  # n_rects, state_bytes
    assert [a for a in args[3:6]] == [ctypes.c_int] * 3
    header = (ROOT / "include" / "nnue_hip.h").read_text()
    doc = re.search(r"/\*((?:(?!/\*).)*?)\*/\s*int\s+" + NAME + r"\(", header, flags=re.S)
    assert doc, "no doc comment"
    text = doc.group(1)
    assert re.search(r"nnue_engine\.cpp:739-786", text) and re.search(r":818-821", text) and re.search(r"nnue_engine\.cpp:48-158", text)
    assert re.search(r"evaluate\.py:\d+", text) and re.search(r"datasets\.py:\d+", text)
    assert "promise" in text and "not undefined behaviour" in text
    assert "hwc" in text and "No scratch" in text


def test_the_abi_version_stays():
    L = lib.load()
    header = (ROOT / "include" / "nnue_hip.h").read_text()
    assert L.nnue_hip_abi_version() == lib.ABI_VERSION == 39
    assert int(re.search(r"NNUE_HIP_ABI_VERSION (\d+)", header).group(1)) == 39


def test_null_pointers(call):
    L = lib.load()
    for field in ("model", "src", "state", "logits", "density", "changed"):
        assert call(**{field: None}) == E_ARG, field
        assert b"null pointer" in L.nnue_hip_last_error(), field
        assert NAME.encode() in L.nnue_hip_last_error()
    assert call(src=_frames(None)) == E_ARG  # the descriptor without frames
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(model=_model(ptr=0)) == E_ARG
    assert b"tensor missing" in L.nnue_hip_last_error()


def test_layout(call):
    L = lib.load()
    p = call.p
    assert call(src=_frames(p, layout=0)) == E_ARG
    msg = L.nnue_hip_last_error()
    assert b"layout" in msg and b"hwc" in msg and b"chw" in msg and b"rectangle" in msg
    assert call(src=_frames(p, layout=2)) == E_ARG
    assert b"layout" in L.nnue_hip_last_error()
    assert call(src=_frames(p, layout=-1)) == E_ARG
    assert call(src=_frames(p, layout=1), state_bytes=call.need - 1) == E_SCRATCH  # hwc passes


def test_rectangle_lists(call):
    L = lib.load()
    assert call(n_rects=-1) == E_ARG
    assert b"negative" in L.nnue_hip_last_error()
    assert call(n_rects=-(1 << 40)) == E_ARG
    assert call(rects=None) == E_ARG
    assert b"rectangle and offset pointers" in L.nnue_hip_last_error()
    assert call(rect_off=None) == E_ARG
    assert call(rects=None, rect_off=None) == E_ARG
    # n_rects == 0 may pass both as NULL; a count beyond int32 is accepted (the offsets cannot reach past 2^31 - 1)
    assert call(rects=None, rect_off=None, n_rects=0, state_bytes=call.need - 1) == E_SCRATCH
    assert call(n_rects=1 << 40, state_bytes=call.need - 1) == E_SCRATCH


def test_stream_count_and_frames(call):
    L = lib.load()
    p = call.p
    assert call(S=0) == E_ARG
    assert b"positive" in L.nnue_hip_last_error()
    assert call(S=-2) == E_ARG
    assert call(src=_frames(p, count=0)) == E_ARG
    assert call(src=_frames(p, count=S - 1)) == E_ARG
    assert b"without indices" in L.nnue_hip_last_error()
    assert call(src=_frames(p, count=1, indices=p), state_bytes=call.need - 1) == E_SCRATCH
    s = _frames(p)
    s.inv_std255[2] = float("nan")
    assert call(src=s) == E_ARG
    assert b"channel 2" in L.nnue_hip_last_error()


def test_state(call):
    L = lib.load()
    p = call.p
    assert call(state=p + 8) == E_ARG
    assert b"aligned" in L.nnue_hip_last_error()
    assert call(state_bytes=call.need - 1) == E_SCRATCH
    assert b"state" in L.nnue_hip_last_error()
    assert call(state_bytes=0) == E_SCRATCH


def test_stacks_argument(call):
    L = lib.load()
    p = call.p
    st = _stacks(p)
    assert call(st=st, stack_out=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(st=st, stack_out=p, state_bytes=call.need - 1) == E_SCRATCH
    assert call(st=_stacks(p, count=65), stack_out=p) == E_ARG
    assert call(st=_stacks(0), stack_out=p) == E_ARG


def test_shapes(call):
    L = lib.load()
    p = call.p
    assert call(H=0) == E_ARG
    assert call(W=-3) == E_ARG
    assert call(H=8, W=40) == E_SHAPE  # the stride comes from H: a wide frame overruns the 4 x 4 grid buffer
    assert b"overruns" in L.nnue_hip_last_error()
    bad = _model(ptr=p)
    bad.num_features += 1
    assert call(model=bad) == E_SHAPE
    assert call(model=_model(ptr=p, l1=4096), state_bytes=1 << 40) == E_SHAPE
    # the bit words, the work list and the table must fit a workgroup's LDS
    assert call(model=_model(g=64, oc=128, ptr=p), state_bytes=1 << 40) == E_SHAPE
    assert b"LDS" in L.nnue_hip_last_error()
    # a frame of 2^31 bytes or more (grid 1: any size maps to one cell)
    assert call(model=_model(g=1, oc=8, ptr=p), H=30000, W=30000) == E_SHAPE
    assert b"2^31" in L.nnue_hip_last_error()


def test_pack_rect_lists():
    rects, off = pack_rect_lists([[(0, 0, 4, 4), (1, 2, 3, 4)], [], np.array([[5, 6, 7, 8]]), [(-1, 2 ** 40, -2 ** 40, 9)]], 4)
    assert rects.dtype == off.dtype == torch.int32 and not rects.is_cuda
    assert rects.tolist() == [[0, 0, 4, 4], [1, 2, 3, 4], [5, 6, 7, 8], [-1, 2 ** 31 - 1, -2 ** 31, 9]]
    assert off.tolist() == [0, 2, 2, 3, 4]
    rects, off = pack_rect_lists([[], []], 2)
    assert tuple(rects.shape) == (0, 4) and off.tolist() == [0, 0, 0]
    for bad in ([[(0, 0, 4)]], [[(0.5, 0, 4, 4)]], [(0, 0, 4, 4)], [[(0, 0, 4, 4)], []], "ab", np.zeros((1, 4), np.int32)):
        with pytest.raises(ValueError):
            pack_rect_lists(bad, 1)
