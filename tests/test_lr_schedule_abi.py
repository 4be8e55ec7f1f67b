"""nnue_lr_schedule_step at the C ABI, with no launch: exported, bound, the ABI number unchanged by the addition, and every
bad argument refused with the library's argument code before anything reaches the device.  CPU only."""
import ctypes
import re

from conftest import ROOT
from nnue_hip import lib

HEADER = (ROOT / "include" / "nnue_hip.h").read_text()
INT32_MAX = 2**31 - 1


def test_symbol_is_exported_bound_and_declared():
    raw = ctypes.CDLL(str(lib.LIB_PATH))
    assert hasattr(raw, "nnue_lr_schedule_step")
    res, args = lib.SIGNATURES["nnue_lr_schedule_step"]
    assert res is ctypes.c_int and len(args) == 5 and args[1] is ctypes.c_int64
    assert re.search(r"int nnue_lr_schedule_step\(const float\* table, int64_t n, int32_t\* position, float\* lr_out, nnue_stream_t stream\);",
                     HEADER)
    assert callable(lib.lr_schedule_step)


def test_abi_version_is_still_39():
    assert lib.ABI_VERSION == 39 == lib.load().nnue_hip_abi_version()
    assert int(re.search(r"NNUE_HIP_ABI_VERSION (\d+)", HEADER).group(1)) == 39


def test_header_comment_cites_both_reference_places():
    m = re.search(r"/\*((?:(?!/\*).)*?)\*/\s*int\s+nnue_lr_schedule_step\(", HEADER, flags=re.S)
    assert m and "train.py:457-471" in m.group(1) and "training_utils.py:283-336" in m.group(1)


def test_bad_arguments_return_the_argument_code_without_launching():
    L = lib.load()
    buf = (ctypes.c_float * 8)()
    pos = (ctypes.c_int32 * 1)(3)
    p, q = ctypes.addressof(buf), ctypes.addressof(pos)
    for args in ((0, 5, q, p), (p, 5, 0, p), (p, 5, q, 0)):
        assert L.nnue_lr_schedule_step(*args, None) == -1
        assert b"nnue_lr_schedule_step: null pointer" in L.nnue_hip_last_error()
    for n in (0, -1, INT32_MAX + 1, 2**40):
        assert L.nnue_lr_schedule_step(p, n, q, p, None) == -1
        assert b"nnue_lr_schedule_step: n=" in L.nnue_hip_last_error()
    assert pos[0] == 3 and all(v == 0.0 for v in buf)  # host memory handed in by mistake was never touched
