"""The planes-fed fused forward's C ABI without a GPU: exports, ABI version, the plane buffer's size against its closed form,
the shape policy, and argument checks that return before anything is launched.  CPU only."""
import ctypes

import pytest

from nnue_hip import lib

BLOCK = 3 * 64 * 128 * 2  # one (64-column tile, 128-row K tile) block: three bf16 images of 64 x 128


def test_exports_and_abi_version():
    L = lib.load()
    assert L.nnue_hip_abi_version() == lib.ABI_VERSION == 39
    for name in ("nnue_ftm_conv_binarize_planes", "nnue_ftm_forward_l1_planes", "nnue_ftm_forward_l1_planes_supported",
                 "nnue_ftm_forward_planes_bytes"):
        assert name in lib.SIGNATURES and hasattr(L, name), name


@pytest.mark.parametrize("b,f,p,l1", [(512, 800, 968, 1024), (256, 801, 800, 128), (250, 300, 392, 256), (512, 129, 128, 256),
                                      (512, 2000, 968, 1024), (32, 2, 4, 64)])
def test_size_query_is_the_closed_form(b, f, p, l1):
    direct = min(f - 1, p)
    assert lib.ftm_forward_planes_bytes(b, f, p, l1) == (l1 // 64) * ((direct + 127) // 128) * BLOCK


def test_size_query_at_the_flagship_shape_and_at_sizes_without_a_buffer():
    assert lib.ftm_forward_planes_bytes(512, 800, 968, 1024) == 16 * 7 * 48 * 1024  # 5.25 MB
    for args in ((0, 800, 968, 1024), (512, 1, 968, 1024), (512, 800, 0, 1024), (512, 800, 968, 0), (512, 800, 968, 96)):
        assert lib.ftm_forward_planes_bytes(*args) == 0, args


def test_shape_policy(monkeypatch):
    monkeypatch.delenv("NNUE_FTM_FWD_PLANES_MIN_WG", raising=False)
    monkeypatch.delenv("NNUE_FTM_BF_BM", raising=False)
    ok = lib.ftm_forward_l1_planes_supported
    assert ok(512, 800, 968, 1024, 128)            # c2: 16 x 16 tiles of 32 rows, today's f32 32-row forward
    assert not ok(32, 800, 968, 64, 32)            # c1: one row tile (a split-K forward, not a fused-forward shape at all)
    assert not ok(128, 65536, 65536, 1024, 128)    # c4: split-K over a table of 268 MB
    assert not ok(1024, 800, 968, 1024, 128)       # c3's sizes: 64-row tiles fill the chip and amortise their own split
    assert not ok(128, 800, 968, 1024, 128)        # any batch a single 128-row tile covers splits K
    assert not ok(512, 800, 968, 1000, 128)        # L1 % 64
    assert not ok(512, 800, 968, 512, 128)         # 128 workgroups: below the floor ...
    monkeypatch.setenv("NNUE_FTM_FWD_PLANES_MIN_WG", "1")
    assert ok(512, 800, 968, 512, 128) and ok(256, 801, 800, 128, 128)  # ... which the test override lowers (read per call)
    assert not ok(1024, 800, 968, 1024, 128) and not ok(128, 800, 968, 1024, 128)
    # every shape it takes is a fused-forward shape
    for args in ((512, 800, 968, 1024, 128), (256, 801, 800, 128, 128), (250, 300, 392, 256, 128), (512, 129, 128, 256, 128)):
        assert ok(*args) and lib.ftm_forward_l1_supported(*args), args


def test_argument_checks_return_before_any_launch(monkeypatch):
    monkeypatch.delenv("NNUE_FTM_FWD_PLANES_MIN_WG", raising=False)
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += -p % 16  # (only compared, never dereferenced: every call below fails its checks)
    need = lib.ftm_forward_planes_bytes(512, 800, 968, 1024)
    fwd = lambda planes, nbytes, b=512: L.nnue_ftm_forward_l1_planes(p, p, planes, nbytes, p, p, p, b, 800, 968, 1024, 128, p, p, None)  # noqa: E731
    conv = lambda planes, nbytes, b=512: L.nnue_ftm_conv_binarize_planes(p, p, p, b, 32, 32, 8, 3, 800, p, 1024, 128, planes, nbytes,  # noqa: E731
                                                                         p, p, p, p, None)
    assert fwd(None, need) == -1 and b"null pointer" in L.nnue_hip_last_error()
    assert conv(None, need) == -1 and b"null pointer" in L.nnue_hip_last_error()
    assert fwd(p, need - BLOCK) == -4 and conv(p, need - BLOCK) == -4 and b"plane buffer" in L.nnue_hip_last_error()
    assert fwd(p + 4, need) == -1 and conv(p + 4, need) == -1 and b"aligned" in L.nnue_hip_last_error()
    assert fwd(p, need, b=1024) == -2 and conv(p, need, b=1024) == -2 and b"planes-fed" in L.nnue_hip_last_error()
