"""Host-side contract of the engine's matrix form (nnue_engine_matrix_supported, nnue_engine_table_planes_bytes,
nnue_engine_matrix_scratch, nnue_engine_pack_table, nnue_engine_evaluate_logits_matrix): the queries are pure, and every invalid
call returns its NNUE_E_* code before anything is launched, so these run without a GPU."""
import ctypes

import pytest

from nnue_hip import lib
from nnue_hip.engine import _CModel, _CStacks

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4
NAMES = ("nnue_engine_matrix_supported", "nnue_engine_table_planes_bytes", "nnue_engine_matrix_scratch", "nnue_engine_pack_table",
         "nnue_engine_evaluate_logits_matrix")


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
    p = (ctypes.addressof(buf) + 15) & ~15
    yield buf, p


def test_symbols_are_exported_and_bound():
    L = lib.load()
    raw = ctypes.CDLL(str(lib.LIB_PATH))
    for n in NAMES:
        assert n in lib.SIGNATURES
        assert hasattr(raw, n) and hasattr(L, n)
    assert L.nnue_hip_abi_version() == lib.ABI_VERSION == 39


def test_queries():
    L = lib.load()
    m = _model()
    mp = ctypes.addressof(m)
    for planes in (1, 2):
        assert L.nnue_engine_matrix_supported(None, 4, planes) == 0
        assert L.nnue_engine_matrix_supported(mp, 0, planes) == 0
        assert L.nnue_engine_matrix_supported(mp, -3, planes) == 0
        assert L.nnue_engine_matrix_supported(mp, 4, planes) == 1
        assert L.nnue_engine_table_planes_bytes(None, planes) == 0
        assert L.nnue_engine_matrix_scratch(None, 4, planes) == 0
        assert L.nnue_engine_matrix_scratch(mp, 0, planes) == 0
        assert L.nnue_engine_matrix_scratch(mp, -1, planes) == 0
    for planes in (0, 3, -1):
        assert L.nnue_engine_matrix_supported(mp, 4, planes) == 0
        assert L.nnue_engine_table_planes_bytes(mp, planes) == 0
        assert L.nnue_engine_matrix_scratch(mp, 4, planes) == 0
    # F = 2^24: F * 128 would reach 2^31, an int32 sum could overflow
    big = _model(g=512, oc=64)
    assert big.num_features == 1 << 24
    assert L.nnue_engine_matrix_supported(ctypes.addressof(big), 4, 1) == 0
    almost = _model(g=512, oc=63)
    assert L.nnue_engine_matrix_supported(ctypes.addressof(almost), 4, 1) == 1
    # the tail's LDS budget, as the gather call's
    assert L.nnue_engine_matrix_supported(ctypes.addressof(_model(l1=2048, l2=8192, l3=8192)), 4, 1) == 0
    assert L.nnue_engine_matrix_supported(ctypes.addressof(_model(l1=4096)), 4, 1) == 0

    # sizes: the planes hold at least F x L1 bytes each, 16-byte granular, and grow with F and L1
    for g, oc, l1 in ((4, 8, 256), (10, 8, 1024), (32, 64, 512), (3, 5, 2), (4, 96, 2048)):
        mm = _model(g=g, oc=oc, l1=l1)
        f = g * g * oc
        one = L.nnue_engine_table_planes_bytes(ctypes.addressof(mm), 1)
        two = L.nnue_engine_table_planes_bytes(ctypes.addressof(mm), 2)
        assert one >= f * l1 and one % 16 == 0 and two == 2 * one
        for b in (1, 7, 64, 1024):
            for planes in (1, 2):
                s = L.nnue_engine_matrix_scratch(ctypes.addressof(mm), b, planes)
                assert s >= L.nnue_engine_scratch(ctypes.addressof(mm), b) + 4 * b * l1
    small, wide, tall = _model(l1=256), _model(l1=512), _model(g=5)
    bytes_of = lambda c: L.nnue_engine_table_planes_bytes(ctypes.addressof(c), 1)
    assert bytes_of(wide) > bytes_of(small) and bytes_of(tall) > bytes_of(small)
    scratch = [L.nnue_engine_matrix_scratch(mp, b, 1) for b in (1, 2, 64, 1024)]
    assert all(a < b for a, b in zip(scratch, scratch[1:]))
    assert L.nnue_engine_matrix_scratch(ctypes.addressof(wide), 16, 1) > L.nnue_engine_matrix_scratch(ctypes.addressof(small), 16, 1)
    assert L.nnue_engine_matrix_scratch(ctypes.addressof(tall), 16, 1) > L.nnue_engine_matrix_scratch(ctypes.addressof(small), 16, 1)


def test_pack_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    m = _model(ptr=p)
    mp = ctypes.addressof(m)
    need = L.nnue_engine_table_planes_bytes(mp, 1)
    assert L.nnue_engine_pack_table(None, 1, p, need, p, None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert L.nnue_engine_pack_table(mp, 1, None, need, p, None) == E_ARG
    assert L.nnue_engine_pack_table(mp, 1, p, need, None, None) == E_ARG
    assert L.nnue_engine_pack_table(ctypes.addressof(_model(ptr=0)), 1, p, need, p, None) == E_ARG
    assert L.nnue_engine_pack_table(mp, 1, p + 8, need, p, None) == E_ARG
    assert b"aligned" in L.nnue_hip_last_error()
    assert L.nnue_engine_pack_table(mp, 1, p, need, p + 2, None) == E_ARG
    assert L.nnue_engine_pack_table(mp, 0, p, need, p, None) == E_SHAPE
    assert L.nnue_engine_pack_table(mp, 3, p, 3 * need, p, None) == E_SHAPE
    assert L.nnue_engine_pack_table(ctypes.addressof(_model(ptr=p, l1=4096)), 1, p, 1 << 40, p, None) == E_SHAPE
    assert L.nnue_engine_pack_table(ctypes.addressof(_model(ptr=p, g=512, oc=64)), 1, p, 1 << 40, p, None) == E_SHAPE
    assert L.nnue_engine_pack_table(mp, 1, p, need - 1, p, None) == E_SCRATCH
    assert L.nnue_engine_pack_table(mp, 2, p, 2 * need - 1, p, None) == E_SCRATCH
    assert b"table_planes" in L.nnue_hip_last_error()


def test_evaluate_rejects_bad_arguments_without_launching(host):
    """The rejection table of test_engine_stream_abi, replayed against the matrix entry point."""
    L = lib.load()
    _, p = host
    m = _model(ptr=p)
    B = 4
    F = m.num_features
    need = L.nnue_engine_matrix_scratch(ctypes.addressof(m), B, 1)
    assert 0 < need <= (1 << 15)
    ok = dict(st=None, planes_ptr=p, planes=1, images=p, active=None, B=B, H=32, W=32, stack_in=None, logits=p, density=p,
              stack_out=None, scratch=p, scratch_bytes=need)

    def call(model=m, **kw):
        a = dict(ok, **kw)
        mp = ctypes.addressof(model) if model is not None else None
        return L.nnue_engine_evaluate_logits_matrix(mp, a["st"], a["planes_ptr"], a["planes"], a["images"], a["active"], a["B"],
                                                    a["H"], a["W"], a["stack_in"], a["logits"], a["density"], a["stack_out"],
                                                    a["scratch"], a["scratch_bytes"], None)

    # null model, planes, outputs, scratch
    assert call(model=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(planes_ptr=None) == E_ARG
    assert call(logits=None) == E_ARG
    assert call(density=None) == E_ARG
    assert call(scratch=None) == E_ARG
    assert call(images=None, active=p, scratch=None) == E_ARG  # the sums live in the scratch whatever the input
    # exactly one of images / active
    assert call(active=p) == E_ARG
    assert b"exactly one" in L.nnue_hip_last_error()
    assert call(images=None) == E_ARG
    # missing model tensor
    assert call(model=_model(ptr=0)) == E_ARG
    # B <= 0
    assert call(B=0) == E_ARG
    assert call(B=-2) == E_ARG
    # scratch too small, for both inputs
    assert call(scratch_bytes=need - 1) == E_SCRATCH
    assert b"scratch" in L.nnue_hip_last_error()
    assert call(images=None, active=p, scratch_bytes=need - 16) == E_SCRATCH
    assert call(scratch_bytes=B * F) == E_SCRATCH  # what the gather call needs is not enough
    # the grid-overrun shape: the stride comes from H, so a wide image overruns the 4x4 grid buffer
    assert call(H=8, W=40) == E_SHAPE
    assert b"overruns" in L.nnue_hip_last_error()
    assert call(H=0) == E_ARG
    assert call(images=None, active=p, H=0, W=0, scratch_bytes=need - 1) == E_SCRATCH  # H, W are not looked at with a map
    # inconsistent model shapes and scales, as nnue_engine_evaluate_logits
    bad = _model(ptr=p)
    bad.num_features = F + 1
    assert call(model=bad) == E_SHAPE
    assert call(model=_model(ptr=p, l1=4096), scratch_bytes=1 << 40) == E_SHAPE
    bad = _model(ptr=p)
    bad.l2_scale = 0.0
    assert call(model=bad) == E_ARG
    # stacks: st without stack_out, a bad count, missing scales
    st = _CStacks()
    st.count = 2
    scales = (ctypes.c_float * 6)(64.0, 64.0, 16.0, 64.0, 64.0, 16.0)
    st.scales = ctypes.cast(scales, ctypes.POINTER(ctypes.c_float))
    for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(st, k, p)
    sp = ctypes.addressof(st)
    assert call(st=sp, stack_out=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(st=sp, stack_out=p, scratch_bytes=need - 1) == E_SCRATCH  # a complete stacks call reaches the size check
    st.count = 65
    assert call(st=sp, stack_out=p) == E_ARG
    st.count = 2
    scales[1] = 0.0
    assert call(st=sp, stack_out=p) == E_ARG
    scales[1] = 64.0
    st.l2_w = 0
    assert call(st=sp, stack_out=p) == E_ARG
    # planes: misaligned, and a count the kernels do not have
    assert call(planes_ptr=p + 8) == E_ARG
    assert b"aligned" in L.nnue_hip_last_error()
    assert call(planes=3) == E_SHAPE
    assert call(planes=0) == E_SHAPE
    # F = 2^24 is refused where _supported says 0
    big = _model(ptr=p, g=512, oc=64)
    assert call(model=big, images=None, active=p, scratch_bytes=1 << 40) == E_SHAPE
    assert b"2^24" in L.nnue_hip_last_error()
