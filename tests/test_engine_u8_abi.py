"""Host-side contract of the engine's uint8 entry points (nnue_engine_evaluate_logits_u8, nnue_engine_evaluate_logits_matrix_u8,
nnue_engine_stream_step_u8): exported, bound, and every invalid call returns its NNUE_E_* code before anything is launched, so
these run without a GPU.  The pointers handed over are host memory that a rejected call never dereferences."""
import ctypes

import numpy as np
import pytest

from nnue_hip import lib
from nnue_hip.engine import _CModel, _CStacks, _CU8Frames, u8_constants

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4
NAMES = ("nnue_engine_evaluate_logits_u8", "nnue_engine_evaluate_logits_matrix_u8", "nnue_engine_stream_step_u8")
B, H, W = 4, 32, 32


def _model(g=4, oc=8, l1=256, l2=32, l3=16, classes=10, ptr=0):
    c = _CModel()
    c.num_features, c.l1, c.l2, c.l3, c.classes, c.grid, c.oc = g * g * oc, l1, l2, l3, classes, g, oc
    c.conv_scale, c.threshold, c.quantized_one, c.l1_scale, c.l2_scale, c.out_scale = 64.0, 0.0, 127.0, 64.0, 64.0, 16.0
    for k in ("conv_w", "conv_b", "ft_w", "ft_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(c, k, ptr)
    return c


def _frames(p, count=B, indices=None, layout=0, mean=None, std=None):
    s = _CU8Frames()
    s.data, s.indices, s.count, s.layout = p, indices, count, layout
    mean255, inv_std255 = u8_constants(mean, std)
    s.mean255[:], s.inv_std255[:] = mean255.tolist(), inv_std255.tolist()
    return s


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * (1 << 16))()
    yield buf, (ctypes.addressof(buf) + 15) & ~15


@pytest.fixture(scope="module", params=NAMES)
def call(request, host):
    """call(model=, src=, **overrides) -> the return code of one entry point on otherwise valid arguments."""
    L = lib.load()
    name = request.param
    _, p = host
    m = _model(ptr=p)
    mp = ctypes.addressof(m)
    if name == "nnue_engine_evaluate_logits_matrix_u8":
        need = L.nnue_engine_matrix_scratch(mp, B, 1)
    else:
        need = L.nnue_engine_scratch(mp, B)
    state = L.nnue_engine_stream_state_bytes(mp, B)
    assert 0 < need <= (1 << 15) and 0 < state <= (1 << 15)
    ok = dict(model=m, src=_frames(p), st=None, B=B, H=H, W=W, stack_in=None, logits=p, density=p, stack_out=None, scratch=p,
              scratch_bytes=need, state_bytes=state)

    def run(**kw):
        a = dict(ok, **kw)
        mptr = ctypes.addressof(a["model"]) if a["model"] is not None else None
        sptr = ctypes.addressof(a["src"]) if a["src"] is not None else None
        if name == "nnue_engine_evaluate_logits_u8":
            return L.nnue_engine_evaluate_logits_u8(mptr, a["st"], sptr, a["B"], a["H"], a["W"], a["stack_in"], a["logits"],
                                                    a["density"], a["stack_out"], a["scratch"], a["scratch_bytes"], None)
        if name == "nnue_engine_evaluate_logits_matrix_u8":
            return L.nnue_engine_evaluate_logits_matrix_u8(mptr, a["st"], p, 1, sptr, a["B"], a["H"], a["W"], a["stack_in"],
                                                           a["logits"], a["density"], a["stack_out"], a["scratch"],
                                                           a["scratch_bytes"], None)
        return L.nnue_engine_stream_step_u8(mptr, a["st"], sptr, a["B"], a["H"], a["W"], a["stack_in"], p, a["state_bytes"], a["logits"],
                                            a["density"], p, a["stack_out"], a["scratch"], a["scratch_bytes"], None)

    run.need, run.p, run.name = need, p, name
    return run


def test_symbols_are_exported_and_bound():
    L = lib.load()
    raw = ctypes.CDLL(str(lib.LIB_PATH))
    for n in NAMES:
        assert n in lib.SIGNATURES
        assert hasattr(raw, n) and hasattr(L, n)
    assert L.nnue_hip_abi_version() == lib.ABI_VERSION
    assert ctypes.sizeof(_CU8Frames) == 56  # two pointers, int64, int32, six floats


def test_null_source(call):
    L = lib.load()
    assert call(src=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(src=_frames(None)) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(model=None) == E_ARG
    assert call(logits=None) == E_ARG
    assert call(scratch=None) == E_ARG
    assert call(model=_model(ptr=0)) == E_ARG  # model tensor missing


def test_layout_and_count(call):
    L = lib.load()
    p = call.p
    assert call(src=_frames(p, layout=2)) == E_ARG
    assert b"layout" in L.nnue_hip_last_error()
    assert call(src=_frames(p, layout=-1)) == E_ARG
    assert call(src=_frames(p, count=0)) == E_ARG
    assert call(src=_frames(p, count=-5, indices=p)) == E_ARG
    assert call(src=_frames(p, count=B - 1)) == E_ARG  # NULL indices: frame b is data + b * 3HW
    assert b"without indices" in L.nnue_hip_last_error()
    assert call(B=0) == E_ARG
    assert call(H=0) == E_ARG
    # with indices one frame serves any B: the call passes every host check up to the scratch size
    assert call(src=_frames(p, count=1, indices=p), scratch_bytes=call.need - 1) == E_SCRATCH


def test_constants(call):
    L = lib.load()
    p = call.p
    for field, value in (("inv_std255", float("inf")), ("inv_std255", float("nan")), ("mean255", float("nan")),
                         ("mean255", float("-inf")), ("inv_std255", 0.0), ("inv_std255", -1.0)):
        for c in range(3):
            s = _frames(p)
            getattr(s, field)[c] = value
            assert call(src=s) == E_ARG, (field, value, c)
    assert b"channel 2" in L.nnue_hip_last_error()
    # int32 overflow under the model's conv_scale: (255 - 0) * inv * scale reaches 2^31 in channel 1 alone
    s = _frames(p)
    s.mean255[1], s.inv_std255[1] = 0.0, float(np.float32(2.0 ** 31 / 255.0 / 64.0) * np.float32(1.0001))
    assert call(src=s) == E_ARG
    assert b"outside int32" in L.nnue_hip_last_error()
    s.inv_std255[1] = float(np.float32(2.0 ** 31 / 255.0 / 64.0) * np.float32(0.999))
    assert call(src=s, scratch_bytes=call.need - 1) == E_SCRATCH  # just inside: accepted
    big = _model(ptr=p)
    big.conv_scale = 2.0 ** 24  # the defaults reach about 2.64 * 2^24 < 2^31 ...
    assert call(model=big, scratch_bytes=call.need - 1) == E_SCRATCH
    big.conv_scale = 2.0 ** 30  # ... and 2.64 * 2^30 does not fit
    assert call(model=big) == E_ARG
    assert b"outside int32" in L.nnue_hip_last_error()


def test_shape_and_scratch(call):
    L = lib.load()
    p = call.p
    assert call(H=8, W=40) == E_SHAPE  # the stride comes from H: a wide frame overruns the 4 x 4 grid buffer
    assert b"overruns" in L.nnue_hip_last_error()
    assert call(scratch_bytes=call.need - 1) == E_SCRATCH
    assert b"scratch" in L.nnue_hip_last_error()
    bad = _model(ptr=p)
    bad.num_features += 1
    assert call(model=bad) == E_SHAPE
    # the front's own limit: the three source rows of one output row must fit a workgroup's LDS
    wide = _model(ptr=p, g=64, oc=1)
    assert call(model=wide, H=2, W=2000, scratch_bytes=1 << 40, state_bytes=1 << 40) == E_SHAPE
    assert b"LDS" in L.nnue_hip_last_error()


def test_stacks_argument(call):
    L = lib.load()
    p = call.p
    st = _CStacks()
    st.count = 2
    scales = (ctypes.c_float * 6)(64.0, 64.0, 16.0, 64.0, 64.0, 16.0)
    st.scales = ctypes.cast(scales, ctypes.POINTER(ctypes.c_float))
    for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(st, k, p)
    sp = ctypes.addressof(st)
    assert call(st=sp, stack_out=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(st=sp, stack_out=p, scratch_bytes=call.need - 1) == E_SCRATCH
    st.count = 65
    assert call(st=sp, stack_out=p) == E_ARG


def test_u8_constants_are_load_batch_constants():
    """The defaults, formed in float32 on the host, are the literals of load_batch_kernel: 0.485f * 255.0f, 1.0f / (0.229f * 255.0f)."""
    mean255, inv_std255 = u8_constants()
    f = np.float32
    assert mean255.dtype == inv_std255.dtype == np.float32
    assert mean255.tolist() == [f(0.485) * f(255), f(0.456) * f(255), f(0.406) * f(255)]
    assert inv_std255.tolist() == [f(1) / (f(0.229) * f(255)), f(1) / (f(0.224) * f(255)), f(1) / (f(0.225) * f(255))]
    for bad in ((0.2, 0.0, 0.2), (0.2, -1.0, 0.2), (0.2, float("nan"), 0.2), (0.2, 0.2), "abc"):
        with pytest.raises(ValueError):
            u8_constants(std=bad)
    with pytest.raises(ValueError):
        u8_constants(mean=(0.1, float("inf"), 0.1))
