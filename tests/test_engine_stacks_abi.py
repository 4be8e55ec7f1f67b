"""Host-side contract of the engine's stack-selecting entry points (nnue_engine_evaluate_logits_stacks,
nnue_engine_stream_step_stacks) and of the selection rule: every invalid call returns its NNUE_E_* code before anything is
launched, so these run without a GPU."""
import ctypes

import pytest
import torch

import nnue
from nnue_hip import engine, lib
from nnue_hip.engine import _CModel, _CStacks

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4


def _model(g=4, oc=8, l1=256, l2=32, l3=16, classes=10, ptr=0):
    c = _CModel()
    c.num_features, c.l1, c.l2, c.l3, c.classes, c.grid, c.oc = g * g * oc, l1, l2, l3, classes, g, oc
    c.conv_scale, c.threshold, c.quantized_one = 64.0, 0.0, 127.0
    c.l1_scale, c.l2_scale, c.out_scale = 0.0, 0.0, 0.0  # the model's own stack fields are not read by these calls
    for k in ("conv_w", "conv_b", "ft_w", "ft_b"):
        setattr(c, k, ptr)
    return c


def _stacks(count, ptr, scales=None):
    st = _CStacks()
    st.count = count
    n = max(1, min(count, 64))
    values = scales if scales is not None else [64.0, 64.0, 16.0] * n
    st._keep = (ctypes.c_float * len(values))(*values)
    st.scales = ctypes.cast(st._keep, ctypes.POINTER(ctypes.c_float))
    for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        setattr(st, k, ptr)
    return st


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * (1 << 16))()  # 16-byte aligned host memory; never dereferenced by a rejected call
    p = (ctypes.addressof(buf) + 15) & ~15
    yield buf, p


def _addr(x):
    return ctypes.addressof(x) if x is not None else None


def test_evaluate_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    m, B = _model(ptr=p), 4
    F = m.num_features
    ok = dict(m=m, st=_stacks(8, p), images=p, B=B, H=32, W=32, stack_in=None, logits=p, density=p, stack_out=p, scratch=p,
              scratch_bytes=B * F)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nnue_engine_evaluate_logits_stacks(_addr(a["m"]), _addr(a["st"]), a["images"], a["B"], a["H"], a["W"], a["stack_in"],
                                                    a["logits"], a["density"], a["stack_out"], a["scratch"], a["scratch_bytes"], None)

    assert call(st=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(m=None) == E_ARG
    for k in ("images", "logits", "density", "stack_out", "scratch"):
        assert call(**{k: None}) == E_ARG, k
    assert call(st=_stacks(0, p)) == E_ARG
    assert b"layer stacks" in L.nnue_hip_last_error()
    assert call(st=_stacks(65, p)) == E_ARG
    assert call(st=_stacks(-1, p)) == E_ARG
    st = _stacks(8, p)
    st.scales = None
    assert call(st=st) == E_ARG
    # a missing stack tensor; a missing tensor of the model
    for k in ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"):
        st = _stacks(8, p)
        setattr(st, k, 0)
        assert call(st=st) == E_ARG, k
    assert b"tensor missing" in L.nnue_hip_last_error()
    assert call(m=_model(ptr=0)) == E_ARG
    # scales the single-stack call would refuse, in any stack: l1_scale 0, l2_scale below 1, out_scale 0, NaN
    for k, j, v in ((0, 0, 0.0), (7, 0, 0.0), (3, 1, 0.5), (0, 1, 0.0), (5, 2, 0.0), (2, 0, -1.0), (1, 1, float("nan"))):
        values = [64.0, 64.0, 16.0] * 8
        values[3 * k + j] = v
        assert call(st=_stacks(8, p, values)) == E_ARG, (k, j, v)
        assert b"scales" in L.nnue_hip_last_error()
    bad = _model(ptr=p)
    bad.conv_scale = 0.5
    assert call(m=bad) == E_ARG
    # what nnue_engine_evaluate_logits checks, with the same codes
    assert call(B=0) == E_ARG and call(H=0) == E_ARG and call(W=-1) == E_ARG
    assert call(scratch_bytes=B * F - 1) == E_SCRATCH
    assert call(H=8, W=40) == E_SHAPE
    assert b"overruns" in L.nnue_hip_last_error()
    bad = _model(ptr=p)
    bad.num_features = F + 1
    assert call(m=bad) == E_SHAPE
    assert call(m=_model(ptr=p, l1=4096)) == E_SHAPE
    # K = 1 and K = 64 are inside the range: the next check fails instead
    assert call(st=_stacks(1, p), scratch_bytes=0) == E_SCRATCH
    assert call(st=_stacks(64, p), scratch_bytes=0) == E_SCRATCH
    # the model's own stack scalars (zero here) and stack pointers (null here) were never read
    assert call(scratch_bytes=0) == E_SCRATCH


def test_stream_step_rejects_bad_arguments_without_launching(host):
    L = lib.load()
    _, p = host
    m, S = _model(ptr=p), 4
    F = m.num_features
    need = L.nnue_engine_stream_state_bytes(ctypes.addressof(m), S)
    assert 0 < need <= (1 << 15)
    ok = dict(m=m, st=_stacks(4, p), images=p, active=None, S=S, H=32, W=32, stack_in=None, state=p, state_bytes=need, logits=p,
              density=p, changed=p, stack_out=p, scratch=p, scratch_bytes=S * F)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nnue_engine_stream_step_stacks(_addr(a["m"]), _addr(a["st"]), a["images"], a["active"], a["S"], a["H"], a["W"],
                                                a["stack_in"], a["state"], a["state_bytes"], a["logits"], a["density"], a["changed"],
                                                a["stack_out"], a["scratch"], a["scratch_bytes"], None)

    assert call(st=None) == E_ARG
    assert b"null pointer" in L.nnue_hip_last_error()
    assert call(m=None) == E_ARG
    for k in ("state", "logits", "density", "changed", "stack_out"):
        assert call(**{k: None}) == E_ARG, k
    assert call(st=_stacks(0, p)) == E_ARG
    assert call(st=_stacks(65, p)) == E_ARG
    values = [64.0, 64.0, 16.0] * 4
    values[3 * 2 + 0] = 0.0  # a zero l1_scale
    assert call(st=_stacks(4, p, values)) == E_ARG
    assert b"scales" in L.nnue_hip_last_error()
    values = [64.0, 64.0, 16.0] * 4
    values[3 * 3 + 1] = 0.999  # an l2_scale below 1
    assert call(st=_stacks(4, p, values)) == E_ARG
    st = _stacks(4, p)
    st.out_b = 0
    assert call(st=st) == E_ARG
    # both or neither of images / active
    assert call(active=p) == E_ARG
    assert b"exactly one" in L.nnue_hip_last_error()
    assert call(images=None) == E_ARG
    assert b"exactly one" in L.nnue_hip_last_error()
    # what nnue_engine_stream_step checks, with the same codes
    assert call(S=0) == E_ARG
    assert call(state=p + 8) == E_ARG
    assert call(state_bytes=need - 1) == E_SCRATCH
    assert call(images=None, active=p, state_bytes=need - 16) == E_SCRATCH
    assert call(scratch_bytes=S * F - 1) == E_SCRATCH
    assert call(scratch=None) == E_ARG
    assert call(H=8, W=40) == E_SHAPE
    assert call(H=0) == E_ARG
    assert call(m=_model(ptr=p, l1=4096), state_bytes=1 << 40) == E_SHAPE


def test_bindings():
    assert lib.load().nnue_hip_abi_version() == lib.ABI_VERSION >= 37
    for n in ("nnue_engine_evaluate_logits_stacks", "nnue_engine_stream_step_stacks"):
        assert n in lib.SIGNATURES and hasattr(lib.load(), n)
    assert ctypes.sizeof(_CStacks) == 16 + 6 * 8  # int32 + padding + the host pointer, then six device pointers


def test_stack_of_is_the_training_rule():
    for K in (1, 2, 3, 4, 8, 63, 64):
        for F in (1, 2, 7, 63, 64, 800, 1024, 65536):
            edges = {0, 1, F - 1, F, F // 2}
            for k in range(1, K):  # both sides of every boundary: the smallest n of stack k is ceil(k (F+1) / K)
                lo = -(-k * (F + 1) // K)
                edges.update((lo - 1, lo, lo + 1))
            n = torch.tensor(sorted(e for e in edges if 0 <= e <= F), dtype=torch.int64)
            got = engine.stack_of(n, K, F)
            closed = torch.tensor([min(K - 1, int(v) * K // (F + 1)) for v in n])
            assert torch.equal(got, nnue.bucket_of(n, K, F)) and torch.equal(got, closed), (K, F)
            assert int(got[0]) == 0 and int(got[-1]) == (K - 1 if F >= K - 1 else F * K // (F + 1)), (K, F)
            assert torch.equal(engine.stack_of(n.to(torch.int32), K, F), closed)
    # dense sweep at one shape
    n = torch.arange(0, 801)
    assert torch.equal(engine.stack_of(n, 8, 800), torch.clamp(n * 8 // 801, max=7))
