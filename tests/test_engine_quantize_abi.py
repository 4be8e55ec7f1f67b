"""Host-side contract of nnue_engine_quantize_model (the engine's tensors from a live model) and of EngineModel.from_model:
every invalid call returns its NNUE_E_* code before anything is launched, so these run without a GPU."""
import ctypes

import pytest
import torch

import nnue
from nnue_hip import lib
from nnue_hip.engine import EngineModel, _CModel, _CStacks

E_ARG, E_SHAPE = -1, -2
SOURCES = ("conv_w", "ft_w", "ft_b", "w1", "b1", "w2", "b2", "w3", "b3")
DIMS = dict(oc=8, F=128, L1=64, L2=8, L3=4, C=10)


def _dst(ptr, **over):
    d = dict(DIMS, **over)
    c = _CModel()
    c.num_features, c.l1, c.l2, c.l3, c.classes, c.grid, c.oc = d["F"], d["L1"], d["L2"], d["L3"], d["C"], 4, d["oc"]
    c.conv_scale, c.threshold, c.quantized_one, c.l1_scale, c.l2_scale, c.out_scale = 64.0, 0.0, 127.0, 64.0, 64.0, 64.0
    for k in ("conv_w", "conv_b", "ft_w", "ft_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(c, k, ptr)
    return c


def _stacks(count, ptr):
    st = _CStacks()
    st.count = count
    st._keep = (ctypes.c_float * (3 * max(1, count)))(*([64.0] * (3 * max(1, count))))
    st.scales = ctypes.cast(st._keep, ctypes.POINTER(ctypes.c_float))
    for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(st, k, ptr)
    return st


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * 4096)()  # 16-byte aligned host memory; never dereferenced by a rejected call
    yield buf, (ctypes.addressof(buf) + 15) & ~15


def _addr(x):
    return ctypes.addressof(x) if x is not None else None


def _call(p, **kw):
    a = dict({k: p for k in SOURCES}, **DIMS, K=1, stack=0, dst=_dst(p), st=None, bad=p)
    a.update(kw)
    return lib.load().nnue_engine_quantize_model(*[a[k] for k in SOURCES], a["oc"], a["F"], a["L1"], a["L2"], a["L3"], a["C"], a["K"],
                                                 a["stack"], _addr(a["dst"]), _addr(a["st"]), a["bad"], None)


def test_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    for k in SOURCES + ("dst", "bad"):  # a null source, destination or counter
        assert _call(p, **{k: None}) == E_ARG, k
        assert b"null pointer" in L.nnue_hip_last_error()
    for K in (0, 65, -1):
        assert _call(p, K=K, st=_stacks(K, p)) == E_ARG, K
        assert b"layer stacks" in L.nnue_hip_last_error()
    assert _call(p, L1=63, dst=_dst(p, L1=63)) == E_SHAPE  # odd L1
    assert b"even" in L.nnue_hip_last_error()
    for k in DIMS:  # a destination whose dimensions disagree with the model's
        assert _call(p, dst=_dst(p, **{k: DIMS[k] + 2})) == E_SHAPE, k
        assert b"destination" in L.nnue_hip_last_error()
        assert _call(p, **{k: 0}) == E_ARG, k
    assert _call(p, K=8, st=_stacks(4, p)) == E_SHAPE  # the destination holds all K stacks ...
    assert _call(p, K=8, stack=8) == E_ARG  # ... or exactly one the model has
    assert _call(p, K=8, stack=-1) == E_ARG
    for k in ("conv_w", "ft_w", "ft_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        d = _dst(p)
        setattr(d, k, 0)
        assert _call(p, dst=d) == E_ARG, k
        assert b"tensor missing" in L.nnue_hip_last_error()
    st = _stacks(8, p)
    st.l2_w = 0
    assert _call(p, K=8, st=st) == E_ARG
    # any 4-byte aligned view is a source; the int16 table is stored 16 bytes at a time
    assert _call(p, ft_w=p + 2) == E_ARG
    d = _dst(p)
    d.ft_w = p + 8
    assert _call(p, dst=d) == E_ARG
    assert b"aligned" in L.nnue_hip_last_error()


def test_binding():
    assert lib.load().nnue_hip_abi_version() == lib.ABI_VERSION >= 38
    assert "nnue_engine_quantize_model" in lib.SIGNATURES and hasattr(lib.load(), "nnue_engine_quantize_model")
    assert len(lib.SIGNATURES["nnue_engine_quantize_model"][1]) == 21


def test_from_model_needs_the_gpu():
    model = nnue.NNUE(nnue.GridFeatureSet(4, 3), 10, 3, 5, num_classes=7)
    with pytest.raises(lib.NnueHipError, match="no CPU fallback"):  # what EngineModel.load raises without a GPU
        EngineModel.from_model(model)
    with pytest.raises(ValueError, match="bucket"):
        EngineModel.from_model(model, bucket="all")
    assert model.training
