"""The weight average's launch-free side (include/nnue_hip.h, "weight average"): the exports and their signatures, the argument
checks of the C entry points, of the trainer, the drop-in optimizers' groups and the config reader, the warm-up table, and the
step mode, which the option is not an input of.  CPU only."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from nnue_hip import lib, optim, step_mode, train_loop
from nnue_hip.trainer import NnueTrainer

HEADER = (ROOT / "include" / "nnue_hip.h").read_text()
BAD_DECAY = (-0.1, 1.0, 1.5, float("nan"), float("inf"))
BAD_OMD = (0.0, -0.5, 1.5, float("nan"), float("inf"))
SIBLINGS = ("nnue_sgd_step", "nnue_adam_step", "nnue_adam_step_ext", "nnue_ftm_backward_weight_update", "nnue_ftm_backward_weight_update_adam",
            "nnue_ftm_backward_weight_update_forward", "nnue_ftm_backward_weight_update_forward_adam", "nnue_multi_sgd_step",
            "nnue_multi_adam_step")


def _prototype(name: str) -> str:
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", body, flags=re.S)
    assert m, f"{name} is not declared in nnue_hip.h"
    return " ".join(m.group(1).split())


def test_the_exports_exist_with_the_documented_signatures():
    raw = ctypes.CDLL(str(lib.LIB_PATH))
    assert _prototype("nnue_ema_update") == ("float* ema, const float* params, int64_t count, float omd, const float* ema_omd_dev, "
                                             "nnue_stream_t stream")
    assert hasattr(raw, "nnue_ema_update") and len(lib.SIGNATURES["nnue_ema_update"][1]) == 6
    for name in SIBLINGS:
        assert hasattr(raw, name + "_ema"), name
        clip, ema = _prototype(name + "_clip"), _prototype(name + "_ema")
        head = clip[:-len(", nnue_stream_t stream")]
        multi = name.startswith("nnue_multi")
        tail = "float* const* ema, const float* ema_omd" if multi else "float* ema, float ema_omd, const float* ema_omd_dev"
        assert ema == f"{head}, {tail}, nnue_stream_t stream", name  # the _clip sibling's arguments plus the average's
        assert len(lib.SIGNATURES[name + "_ema"][1]) == len(lib.SIGNATURES[name + "_clip"][1]) + (2 if multi else 3)
    # the siblings are timed under the plain form's name (bench.py's timer keys name the plain forms): the 14 rows, spelled out
    assert {k: v for k, v in lib._TIMED_AS.items() if k.endswith(("_clip", "_ema"))} == {
        "nnue_sgd_step_ema": "nnue_sgd_step", "nnue_adam_step_ema": "nnue_adam_step", "nnue_adam_step_ext_ema": "nnue_adam_step_ext",
        "nnue_ftm_backward_weight_update_ema": "nnue_ftm_backward_weight_update",
        "nnue_ftm_backward_weight_update_forward_ema": "nnue_ftm_backward_weight_update_forward",
        "nnue_ftm_backward_weight_update_adam_ema": "nnue_ftm_backward_weight_update_adam",
        "nnue_ftm_backward_weight_update_forward_adam_ema": "nnue_ftm_backward_weight_update_forward_adam",
        "nnue_sgd_step_clip": "nnue_sgd_step", "nnue_adam_step_clip": "nnue_adam_step", "nnue_adam_step_ext_clip": "nnue_adam_step_ext",
        "nnue_ftm_backward_weight_update_clip": "nnue_ftm_backward_weight_update",
        "nnue_ftm_backward_weight_update_forward_clip": "nnue_ftm_backward_weight_update_forward",
        "nnue_ftm_backward_weight_update_adam_clip": "nnue_ftm_backward_weight_update_adam",
        "nnue_ftm_backward_weight_update_forward_adam_clip": "nnue_ftm_backward_weight_update_forward_adam"}


def test_the_entry_points_refuse_bad_arguments_without_launching():
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    # the stand-alone pass: NULL pointers, count <= 0, a bad rate (a device rate replaces the float unseen)
    assert L.nnue_ema_update(None, p, 16, 0.1, None, None) == -1 and b"null pointer" in L.nnue_hip_last_error()
    assert L.nnue_ema_update(p, None, 16, 0.1, None, None) == -1
    for count in (0, -4):
        assert L.nnue_ema_update(p, p, count, 0.1, None, None) == -1 and b"count" in L.nnue_hip_last_error()
    for omd in BAD_OMD:
        assert L.nnue_ema_update(p, p, 16, omd, None, None) == -1 and b"omd" in L.nnue_hip_last_error()
    ranges = (ctypes.c_int64 * 2)(0, 8)
    sgd = lambda e, o, n=16, w=p: L.nnue_sgd_step_ema(w, p, p, n, 0.1, 0.9, 0.0, 1.0, 1.0, 1, None, p, 1 << 20, None, 0, 0, None, None,  # noqa: E731
                                                      None, 0, 0, 0, None, 0, None, 1.0, ranges, 1, e, o, None, None)
    adam = lambda e, o, n=16, w=p: L.nnue_adam_step_ema(w, p, p, p, p, n, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, None, p, 1 << 20, None, 1.0,  # noqa: E731
                                                        ranges, 1, e, o, None, None)
    adam_ext = lambda e, o, n=16, w=p: L.nnue_adam_step_ext_ema(w, p, p, p, p, n, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, None, p, 1 << 20,  # noqa: E731
                                                                None, 0, 0, 0, None, 0, None, 1.0, ranges, 1, e, o, None, None)
    table = lambda e, o, n=8, w=p: L.nnue_ftm_backward_weight_update_ema(p, p, n, 16, 16, 64, w, p, p, 0.1, 0.9, 0.0, 1.0, 0, 1.0, None, e, o,  # noqa: E731
                                                                         None, None)
    table_adam = lambda e, o, n=8, w=p: L.nnue_ftm_backward_weight_update_adam_ema(p, p, n, 16, 16, 64, w, p, p, p, p, 0.1, 0.9, 0.999, 1e-8,  # noqa: E731
                                                                                   0.0, 1.0, 1.0, None, e, o, None, None)
    ptrs, counts = (ctypes.c_void_p * 1)(p), (ctypes.c_int64 * 1)(16)
    one = lambda v: (ctypes.c_float * 1)(v)  # noqa: E731
    i32 = (ctypes.c_int32 * 1)(1)

    def multi_sgd(e, o, n=16, w=p):
        return L.nnue_multi_sgd_step_ema((ctypes.c_void_p * 1)(w), ptrs, ptrs, (ctypes.c_int64 * 1)(n), 1, one(0.1), one(0.9), one(0.0), i32,
                                         one(1.0), 1.0, None, p, 1 << 20, None, (ctypes.c_void_p * 1)(e), one(o), None)

    def multi_adam(e, o, n=16, w=p):
        return L.nnue_multi_adam_step_ema((ctypes.c_void_p * 1)(w), ptrs, ptrs, ptrs, ptrs, (ctypes.c_int64 * 1)(n), 1, one(0.1), one(0.9),
                                          one(0.999), one(1e-8), one(0.0), one(1.0), 1.0, None, p, 1 << 20, None, (ctypes.c_void_p * 1)(e),
                                          one(o), None)
    fused = lambda e, o, n=8, w=p: L.nnue_ftm_backward_weight_update_forward_ema(p, p, n, 16, 16, 64, w, p, p, 0.1, 0.9, 0.0, 1.0, 0, 1.0, None,  # noqa: E731
                                                                                 p, p, 8, p, p, p, 1 << 20, e, o, None, None)
    fused_adam = lambda e, o, n=8, w=p: L.nnue_ftm_backward_weight_update_forward_adam_ema(p, p, n, 16, 16, 64, w, p, p, p, p, 0.1, 0.9, 0.999,  # noqa: E731
                                                                                           1e-8, 0.0, 1.0, 1.0, None, p, p, 8, p, p, p, 1 << 20,
                                                                                           e, o, None, None)
    for call in (sgd, adam, adam_ext, table, table_adam, fused, fused_adam, multi_sgd, multi_adam):
        for omd in BAD_OMD:
            assert call(p, omd) == -1, (call, omd)
            assert b"ema_omd" in L.nnue_hip_last_error()
        if call in (fused, fused_adam):  # a batch of 0 is refused there as by the _clip sibling: not a shape the fused pass takes
            assert call(p, 0.1, 0) == call(None, 0.0, 0) < 0 and call(p, 0.1, -1) == call(None, 0.0, -1) < 0
        else:
            assert call(p, 0.1, 0) == -1, call    # a count (table forms: a batch) of 0
            assert call(p, 0.1, -1) == -1, call
        assert call(p, 0.1, 16, None) == -1, call  # NULL parameters
        assert call(None, float("nan"), 0) < 0     # (average off: the _clip sibling's own checks)
    # the fused pass with or without an average refuses what its _clip sibling refuses (this shape is no split-K forward over a big table)
    assert fused(p, 0.1) == fused(None, 0.0) == fused_adam(p, 0.1) == fused_adam(None, 0.0) == -2


@pytest.mark.parametrize("value", BAD_DECAY)
def test_trainer_optimizers_and_config_refuse_a_bad_decay(value):
    with pytest.raises(ValueError, match="ema_decay"):  # before the model, the library or the device is touched
        NnueTrainer(None, 8, (8, 8), lr=0.1, ema_decay=value)
    with pytest.raises(ValueError, match="ema_decay"):
        train_loop.config_ema(SimpleNamespace(ema_decay=value))
    w, b = torch.nn.Parameter(torch.zeros(4, 4)), torch.nn.Parameter(torch.zeros(4))
    for cls in (optim.SGD, optim.Adam):
        with pytest.raises(ValueError, match="ema_decay"):
            cls([w, b], lr=0.1, ema_decay=value)
        with pytest.raises(ValueError, match="ema_decay"):
            cls([dict(params=[w], ema_decay=value), dict(params=[b])], lr=0.1)


def test_the_config_reader_and_the_warm_up_without_a_decay():
    assert train_loop.config_ema(SimpleNamespace()) == (0.0, False)
    assert train_loop.config_ema(SimpleNamespace(ema_decay=0.999, ema_warmup=1)) == (0.999, True)
    with pytest.raises(ValueError, match="ema_decay"):
        train_loop.config_ema(SimpleNamespace(ema_decay=1.5))
    with pytest.raises(ValueError, match="ema_warmup"):
        train_loop.config_ema(SimpleNamespace(ema_warmup=True))
    with pytest.raises(ValueError, match="ema_warmup"):
        NnueTrainer(None, 8, (8, 8), lr=0.1, ema_warmup=True)


@pytest.mark.parametrize("decay", (0.05, 0.1, 0.5, 0.9, 0.999, 0.9999))
def test_the_warm_up_table_is_the_formula_in_float64(decay):
    table = lib.ema_warmup_table(decay)
    assert table.dtype == torch.float32 and table.dim() == 1
    t = torch.arange(table.numel(), dtype=torch.float64)
    decay_t = torch.minimum(torch.tensor(decay, dtype=torch.float64), (1.0 + t) / (10.0 + t))
    assert torch.equal(table, (1.0 - decay_t).to(torch.float32))
    # the table ends where the decay itself is reached: the launch clamps its position there, so every later step uses it
    assert float(table[-1]) == lib.ema_omd(decay) and float(decay_t[-1]) == decay
    assert table.numel() <= 2 or float(decay_t[-3]) < decay  # (and no sooner, but for one entry of slack)
    n = table.numel()
    assert (1.0 + n) / (10.0 + n) >= decay  # (steps beyond the table would not warm up any more)
    assert lib.ema_omd(decay) == float(torch.tensor(1.0 - decay, dtype=torch.float64).to(torch.float32))


def test_the_option_is_a_group_option_with_its_state_on_the_cpu_path():
    w, b = torch.nn.Parameter(torch.full((4, 4), 3.0)), torch.nn.Parameter(torch.full((4,), 3.0))
    for cls in (optim.SGD, optim.Adam):
        opt = cls([dict(params=[w], ema_decay=0.9), dict(params=[b])], lr=0.1)
        assert [g["ema_decay"] for g in opt.param_groups] == [0.9, 0.0] and opt.defaults["ema_decay"] == 0.0
        assert [g["ema_decay"] for g in opt.state_dict()["param_groups"]] == [0.9, 0.0]
        start = w.detach().clone()
        w.grad, b.grad = torch.ones_like(w), torch.ones_like(b)
        opt.step()
        ema = opt.ema_state()
        assert list(ema) == [w] and ema[w] is opt.state[w]["ema"]
        assert torch.allclose(ema[w], start + lib.ema_omd(0.9) * (w.detach() - start), rtol=1e-6)
        other = cls([dict(params=[w]), dict(params=[b], ema_decay=0.5)], lr=0.1)
        other.load_state_dict(opt.state_dict())
        assert [g["ema_decay"] for g in other.param_groups] == [0.9, 0.0]
        assert torch.equal(other.ema_state()[w], ema[w])


def test_the_option_is_not_an_input_of_the_step_mode():
    """The average is a hyper-parameter, not a mode: resolve() has no argument and StepMode no field that could carry it, so the
    goldens are untouched whatever the option is (the signatures are the whole check: nothing else could tell the two apart)."""
    assert not [p for p in inspect.signature(step_mode.resolve).parameters if "ema" in p]
    assert not [f for f in step_mode.StepMode.__dataclass_fields__ if "ema" in f]
    assert {"ema_decay", "ema_warmup"} <= set(inspect.signature(NnueTrainer.__init__).parameters)
