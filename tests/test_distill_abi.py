"""Distillation at the C ABI and on the host, with no launch: the three new symbols are declared with reference citations,
exported and bound; their refusals return the argument code before anything reaches the device (the pointers are host memory a
rejected call never dereferences); the binding, the trainer and the train loop check alpha and T on the host.  CPU only."""
import ctypes
import re
import types

import pytest
import torch

from conftest import ROOT
from nnue_hip import lib, train_loop
from nnue_hip.trainer import NnueTrainer

HEADER = (ROOT / "include" / "nnue_hip.h").read_text()
E_ARG = -1
NEW = ("nnue_cross_entropy_distill", "nnue_classifier_train_step_distill", "nnue_classifier_train_step_distill_bucketed")
BAD_ALPHA = (-0.01, 1.01, float("nan"), float("inf"))
BAD_T = (0.0, -1.0, float("nan"), float("inf"))


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_uint8 * (1 << 16))()
    yield (ctypes.addressof(buf) + 15) & ~15
    del buf


def _err():
    return lib.load().nnue_hip_last_error()


def test_symbols_are_declared_exported_bound_and_documented():
    raw = ctypes.CDLL(str(lib.LIB_PATH))
    for name in NEW:
        doc = re.search(r"/\*((?:(?!/\*).)*?)\*/\s*int\s+" + name + r"\(", HEADER, flags=re.S)
        assert doc and re.search(r"train\.py:250-254", doc.group(1)), name
        assert hasattr(raw, name), name
        assert name in lib.SIGNATURES and lib.SIGNATURES[name][0] is ctypes.c_int, name
    f, vp = ctypes.c_float, ctypes.c_void_p
    for soft, distill in (("nnue_classifier_train_step_soft", "nnue_classifier_train_step_distill"),
                          ("nnue_classifier_train_step_soft_bucketed", "nnue_classifier_train_step_distill_bucketed")):
        s, d = lib.SIGNATURES[soft][1], lib.SIGNATURES[distill][1]
        tail = 2 if soft.endswith("bucketed") else 1  # [buckets,] stream
        assert d[:len(s) - tail] == s[:-tail] and d[-tail:] == s[-tail:]  # the soft arguments, then teacher, alpha, temperature
        assert d[len(s) - tail:-tail] == [vp, f, f]
    s, d = lib.SIGNATURES["nnue_cross_entropy_soft"][1], lib.SIGNATURES["nnue_cross_entropy_distill"][1]
    assert d[:len(s) - 1] == s[:-1] and d[len(s) - 1:] == [vp, f, f, vp]
    assert "KL_b" in HEADER and "pT_c" in HEADER and HEADER.count("alpha T^2 KL_b") == 1  # the definition is in the header, once
    assert lib.ABI_VERSION == 39 and "#define NNUE_HIP_ABI_VERSION 39" in HEADER
    assert callable(lib.cross_entropy_distill)


def _step(p, alpha=0.5, T=2.0, teacher="p", eps=0.1, labels_b="p", lam="p", phases=3, bucketed=False, B=64, L1=128):
    L = lib.load()
    pick = lambda v: p if v == "p" else v  # noqa: E731
    args = (p, 1, p, p, p, p, p, p, 0.0, p, 1.0, B, L1, 64, 16, 10, p, p, p, p, p, p, p, p, p, p, p, p, p, 1 << 30, phases,
            pick(labels_b), pick(lam), eps, pick(teacher), alpha, T)
    if bucketed:
        return L.nnue_classifier_train_step_distill_bucketed(*args, None, None)
    return L.nnue_classifier_train_step_distill(*args, None)


@pytest.mark.parametrize("bucketed", (False, True))
def test_train_step_distill_refusals(p, bucketed):
    for alpha in BAD_ALPHA:
        assert _step(p, alpha=alpha, bucketed=bucketed) == E_ARG and b"alpha" in _err(), alpha
    for T in BAD_T:
        assert _step(p, T=T, bucketed=bucketed) == E_ARG and b"temperature" in _err(), T
    assert _step(p, teacher=None, bucketed=bucketed) == E_ARG and b"without teacher" in _err()
    # the two soft refusals
    for eps in (-0.01, 1.0, float("nan")):
        assert _step(p, eps=eps, bucketed=bucketed) == E_ARG and b"eps" in _err(), eps
    assert _step(p, lam=None, bucketed=bucketed) == E_ARG and b"labels_b without lam" in _err()
    # ... and the plain call's, with the same codes, also on the alpha == 0 path (no teacher needed)
    assert _step(p, phases=0, bucketed=bucketed) == E_ARG and b"phases" in _err()
    assert _step(p, alpha=0.0, teacher=None, phases=0, bucketed=bucketed) == E_ARG and b"phases" in _err()
    assert _step(p, B=0, bucketed=bucketed) == E_ARG


def test_cross_entropy_distill_refusals(p):
    L = lib.load()

    def call(alpha=0.5, T=2.0, teacher=p, eps=0.1, lam=p, logits=p, B=4, C=10):
        return L.nnue_cross_entropy_distill(logits, p, p, lam, eps, B, C, 1.0, p, p, p, teacher, alpha, T, None)

    for alpha in BAD_ALPHA:
        assert call(alpha=alpha) == E_ARG and b"alpha" in _err(), alpha
    for T in BAD_T:
        assert call(T=T) == E_ARG and b"temperature" in _err(), T
    assert call(teacher=None) == E_ARG and b"without teacher" in _err()
    assert call(eps=1.0) == E_ARG and b"eps" in _err()
    assert call(lam=None) == E_ARG and b"labels_b without lam" in _err()
    assert call(logits=None) == E_ARG and b"null pointer" in _err()
    assert call(B=0) == E_ARG and call(C=0) == E_ARG
    assert call(alpha=0.0, teacher=None, eps=1.0) == E_ARG and b"eps" in _err()  # alpha == 0: the soft call and its refusals


def test_binding_checks_alpha_and_temperature_on_the_host():
    """ValueError before any tensor is looked at (CPU tensors would otherwise be refused as such)."""
    z, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    for alpha in BAD_ALPHA:
        with pytest.raises(ValueError, match="alpha"):
            lib.cross_entropy_distill(z, y, z, alpha, 2.0)
        with pytest.raises(ValueError, match="alpha"):
            lib.classifier_train_step(z, True, z, z, z, z, z, z, y, distill=(z, alpha, 2.0))
    for T in BAD_T:
        with pytest.raises(ValueError, match="temperature"):
            lib.cross_entropy_distill(z, y, z, 0.5, T)
        with pytest.raises(ValueError, match="temperature"):
            lib.classifier_train_step(z, True, z, z, z, z, z, z, y, distill=(z, 0.5, T))
    assert lib.check_distill(0, 1) == (0.0, 1.0) and lib.check_distill(1.0, 0.5) == (1.0, 0.5)


@pytest.mark.parametrize("kw", [dict(distill_alpha=a) for a in BAD_ALPHA] + [dict(distill_alpha=0.5, distill_temperature=t) for t in BAD_T]
                         + [dict(distill_temperature=0.0)])
def test_trainer_refuses_bad_distill_values(kw):
    """Refused before the model, the library or the device is touched."""
    with pytest.raises(ValueError, match="distill"):
        NnueTrainer(None, 8, (8, 8), lr=0.1, **kw)


def _bare_trainer(alpha, T=1.0):
    """A trainer's host state without its buffers: enough for the checks that run before anything touches the device."""
    t = NnueTrainer.__new__(NnueTrainer)
    t.B, t.C, t.two_labels, t.soft_inputs = 4, 3, False, None
    t.inputs = [(torch.zeros(4, 3, 2, 2), torch.zeros(4, dtype=torch.int64))]
    t.distill_alpha, t.distill_temperature = alpha, T
    t.teacher_inputs = [torch.zeros(4, 3)] if alpha > 0 else None
    return t


def test_stage_refuses_teacher_logits_that_do_not_belong():
    images, labels, teacher = torch.zeros(4, 3, 2, 2), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="distill_alpha > 0"):  # a trainer built with alpha = 0 has no use for them
        _bare_trainer(0.0)._stage(0, images, labels, None, None, None, teacher)
    with pytest.raises(ValueError, match="beside images"):
        _bare_trainer(0.5)._stage(0, None, None, None, None, None, teacher)
    with pytest.raises(ValueError, match="needs teacher_logits"):  # ... and one built with alpha > 0 needs them with a copied batch
        _bare_trainer(0.5)._stage(0, images, labels, None, None, None, None)


def test_load_state_dict_refuses_other_distill_values():
    """tests/test_trainer_state_validation.py's stub with the values the later checks read: a state that passes every other check
    is refused for its distill values alone, before any copy; a state from before the keys reads as 0 and 1.  The round trip on
    a real trainer is tests/test_gpu_distill_trainer.py's."""
    from test_trainer_state_validation import _state, _stub

    def stub(alpha, T):
        tr = _stub()
        tr._label_smoothing, tr._hyper = 0.0, dict(weight_clip=0.0)
        tr.distill_alpha, tr.distill_temperature = alpha, T
        tr._apply_optimizer_state = lambda *a: pytest.fail("copied before the state was validated")
        return tr

    for (alpha, T), keys in (((0.0, 1.0), dict(distill_alpha=0.5, distill_temperature=1.0)),
                             ((0.0, 1.0), dict(distill_temperature=2.0)),
                             ((0.5, 2.0), dict(distill_alpha=0.5, distill_temperature=4.0)),
                             ((0.5, 2.0), dict(distill_alpha=0.25, distill_temperature=2.0)),
                             ((0.5, 1.0), dict())):
        with pytest.raises(ValueError, match="distill_alpha"):
            stub(alpha, T).load_state_dict(dict(_state(), **keys))


def test_run_training_needs_a_teacher_when_the_config_distils():
    config = types.SimpleNamespace(optimizer_type="sgd", distill_alpha=0.5, distill_temperature=2.0)
    with pytest.raises(ValueError, match="needs a teacher"):
        train_loop.run_training(config, [], [])
    for bad in (dict(distill_alpha=1.5), dict(distill_alpha=0.5, distill_temperature=0.0)):
        with pytest.raises(ValueError, match="distill"):
            train_loop.run_training(types.SimpleNamespace(optimizer_type="sgd", **bad), [], [], teacher=lambda x: x)
