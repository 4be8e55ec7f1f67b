"""The value planes' C ABI without a GPU: exports, the plane buffer's size against its closed form, the shape policy with its
two per-call knobs, what nnue_ftm_uses_bf16 reports for the merged launch's value tiles, and argument checks that return
before anything is launched.  CPU only."""
import ctypes

import pytest

from nnue_hip import lib

BLOCK = 3 * 64 * 128 * 2  # one (64-column value tile, 128-deep K tile) block: three bf16 planes of 64 x 128
C2 = (512, 800, 968, 1024, 32, 32, 3)  # B, F, P, L1, H, W, stride


@pytest.fixture(autouse=True)
def knobs_unset(monkeypatch):
    for knob in ("NNUE_FTM_VAL_PLANES", "NNUE_FTM_VAL_PLANES_MIN_TILES", "NNUE_FTM_BF16", "NNUE_FTM_BF_WM"):
        monkeypatch.delenv(knob, raising=False)


def test_exports():
    L = lib.load()
    for name in ("nnue_ftm_value_planes_supported", "nnue_ftm_value_planes_bytes", "nnue_ftm_conv_binarize_value_planes", "nnue_ftm_backward_planes"):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    assert lib._TIMED_AS["nnue_ftm_conv_binarize_value_planes"] == "nnue_ftm_conv_binarize"
    assert lib._TIMED_AS["nnue_ftm_backward_planes"] == "nnue_ftm_backward"


@pytest.mark.parametrize("b,f,p,l1", [(512, 800, 968, 1024), (37, 968, 968, 136), (1, 864, 864, 64), (5, 1352, 1352, 264), (9, 300, 1152, 104)])
def test_size_query_is_the_closed_form(b, f, p, l1):
    g = p // 8
    assert lib.ftm_value_planes_bytes(b, f, p, l1) == ((g + 7) // 8) * ((l1 + 127) // 128) * BLOCK


def test_size_query_at_the_flagship_shape_and_at_sizes_without_a_buffer():
    assert lib.ftm_value_planes_bytes(512, 800, 968, 1024) == 16 * 8 * 48 * 1024  # 6.3 MB
    for args in ((0, 800, 968, 1024), (512, 1, 968, 1024), (512, 800, 0, 1024), (512, 800, 968, 0), (512, 800, 968, 1020), (512, 800, 964, 1024)):
        assert lib.ftm_value_planes_bytes(*args) == 0, args


def test_shape_policy(monkeypatch):
    ok, uses5 = lib.ftm_value_planes_supported, lambda b, f, p, l1: lib.load().nnue_ftm_uses_bf16(5, b, f, p, l1)  # noqa: E731
    assert ok(*C2) and uses5(*C2[:4]) == 1                       # c2: 16 x 16 value tiles of 32 rows, the STE ride
    assert not ok(32, 800, 968, 64, 32, 32, 3)                   # c1: one row tile
    assert not ok(1024, 800, 968, 1024, 32, 32, 3)               # c3's sizes: 64-row value tiles (six plane products already)
    assert uses5(1024, 800, 968, 1024) == 1
    assert not ok(128, 65536, 65536, 1024, 224, 224, 7)          # c4
    assert not ok(512, 800, 968, 1020, 32, 32, 3) and uses5(512, 800, 968, 1020) == 0   # L1 % 8 == 4
    assert not ok(512, 800, 968, 1024, 32, 32, 2)                # an image whose grid is not the map's
    assert not ok(256, 800, 968, 1024, 32, 32, 3) and uses5(256, 800, 968, 1024) == 0   # 128 value tiles: below the floor ...
    monkeypatch.setenv("NNUE_FTM_VAL_PLANES_MIN_TILES", "1")
    assert ok(256, 800, 968, 1024, 32, 32, 3) and ok(1, 864, 864, 64, 17, 23, 2) and uses5(256, 800, 968, 1024) == 1  # ... which tests lower
    assert not ok(1024, 800, 968, 1024, 32, 32, 3) and not ok(512, 800, 968, 1020, 32, 32, 3)
    for args in (C2, (256, 800, 968, 1024, 32, 32, 3), (37, 968, 968, 136, 31, 31, 3)):  # every shape it takes rides the STE on 32-row tiles
        assert ok(*args) and lib.ftm_backward_ste_chunks(*args) == -(-args[0] // 32) * -(-(args[2] // 8) // 8), args
    monkeypatch.setenv("NNUE_FTM_VAL_PLANES", "0")               # the knob, read per call
    assert not ok(*C2) and uses5(*C2[:4]) == 0
    monkeypatch.setenv("NNUE_FTM_VAL_PLANES", "1")
    monkeypatch.setenv("NNUE_FTM_BF16", "0")                     # f32 weight tiles: no ride, no planes
    assert not ok(*C2) and uses5(*C2[:4]) == 0


def test_argument_checks_return_before_any_launch():
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += -p % 16  # (only compared, never dereferenced: every call below fails its checks)
    need = lib.ftm_value_planes_bytes(512, 800, 968, 1024)
    part_bytes = 8 * 28 * 256 * 4

    def conv(vp, nbytes, b=512):
        return L.nnue_ftm_conv_binarize_value_planes(p, p, p, b, 32, 32, 8, 3, 800, p, 1024, 128, None, 0, vp, nbytes, p, p, p, p, None)

    def bwd(vp, nbytes):
        return L.nnue_ftm_backward_planes(p, p, p, p, 512, 800, 968, 1024, p, p, None, None, None, 0, None, None, None, p, None, p, p, 32, 32, 3,
                                          p, part_bytes, vp, nbytes, None)

    assert conv(None, need) == -1 and b"null pointer" in L.nnue_hip_last_error()
    assert bwd(None, need) == -1 and b"null pointer" in L.nnue_hip_last_error()
    assert conv(p, need - BLOCK) == -4 and b"value-plane buffer" in L.nnue_hip_last_error()
    assert bwd(p, need - BLOCK) == -4 and b"value-plane buffer" in L.nnue_hip_last_error()
    assert conv(p + 4, need) == -1 and b"aligned" in L.nnue_hip_last_error()
    assert bwd(p + 4, need) == -1 and b"aligned" in L.nnue_hip_last_error()
    assert conv(p, need, b=1024) == -2 and b"value-planes shape" in L.nnue_hip_last_error()
