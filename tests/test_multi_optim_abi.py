"""Host side of the multi-tensor optimizer (nnue_multi_sgd_step / nnue_multi_adam_step and nnue_hip.optim): every invalid
call returns its NNUE_E_* code before anything is launched, the optimizer classes refuse what the kernels do not implement,
and CPU parameters follow clip_grad_norm_ + torch.optim bit for bit.  No GPU needed: the pointers handed to rejected calls
are host memory that is never dereferenced."""
import ctypes

import pytest
import torch

from nnue_hip import lib
from nnue_hip import optim

E_ARG, E_SCRATCH = -1, -4


class Host:
    """n segments of host memory and the per-segment host arrays the entry points take."""

    def __init__(self, n=3, counts=(5, 16384, 40000)):
        self.keep = (ctypes.c_uint8 * (1 << 12))()
        p = (ctypes.addressof(self.keep) + 15) & ~15
        self.n = n
        self.ptrs = (ctypes.c_void_p * n)(*([p] * n))
        self.counts = (ctypes.c_int64 * n)(*counts[:n])
        self.f = lambda v: (ctypes.c_float * n)(*([v] * n))
        self.first = (ctypes.c_int32 * n)()
        self.scratch = p
        self.scratch_bytes = lib.load().nnue_multi_optim_scratch(self.counts, n)


def sgd(h, **kw):
    a = dict(params=h.ptrs, grads=h.ptrs, m=h.ptrs, counts=h.counts, n=h.n, lr=h.f(0.1), mom=h.f(0.9), wd=h.f(0.0), first=h.first,
             max_norm=1.0, norm=None, scratch=h.scratch, scratch_bytes=h.scratch_bytes, lr_dev=None)
    a.update(kw)
    return lib.load().nnue_multi_sgd_step(a["params"], a["grads"], a["m"], a["counts"], a["n"], a["lr"], a["mom"], a["wd"], a["first"],
                                          a["max_norm"], a["norm"], a["scratch"], a["scratch_bytes"], a["lr_dev"], None)


def adam(h, **kw):
    a = dict(params=h.ptrs, grads=h.ptrs, m=h.ptrs, v=h.ptrs, steps=h.ptrs, counts=h.counts, n=h.n, lr=h.f(1e-3), b1=h.f(0.9),
             b2=h.f(0.999), eps=h.f(1e-8), wd=h.f(0.0), max_norm=1.0, norm=None, scratch=h.scratch, scratch_bytes=h.scratch_bytes)
    a.update(kw)
    return lib.load().nnue_multi_adam_step(a["params"], a["grads"], a["m"], a["v"], a["steps"], a["counts"], a["n"], a["lr"], a["b1"],
                                           a["b2"], a["eps"], a["wd"], a["max_norm"], a["norm"], a["scratch"], a["scratch_bytes"], None,
                                           None)


def last_error():
    return lib.load().nnue_hip_last_error()


def test_scratch_query():
    L = lib.load()
    counts = (ctypes.c_int64 * 3)(1, 16384, 16385)  # one partial per 16384 elements of each tensor: 1 + 1 + 2
    assert L.nnue_multi_optim_scratch(counts, 3) >= 4 * 4
    big = (ctypes.c_int64 * 1)(1 << 26)
    assert L.nnue_multi_optim_scratch(big, 1) >= 4 * (1 << 26) // 16384
    assert L.nnue_multi_optim_scratch(counts, 0) == 0
    assert L.nnue_multi_optim_scratch(None, 3) == 0


def test_multi_sgd_rejects_bad_arguments_without_launching():
    h = Host()
    assert sgd(h, n=0) == E_ARG and b"must be positive" in last_error()
    assert sgd(h, params=None) == E_ARG and b"null pointer" in last_error()
    assert sgd(h, first=None) == E_ARG
    assert sgd(h, scratch=None) == E_ARG
    assert sgd(h, lr=None) == E_ARG
    one_null = (ctypes.c_void_p * 3)(h.ptrs[0], None, h.ptrs[0])
    assert sgd(h, grads=one_null) == E_ARG and b"segment 1" in last_error()
    # momentum without a buffer; momentum 0 needs none
    assert sgd(h, m=None) == E_ARG and b"momentum buffer" in last_error()
    assert sgd(h, m=one_null) == E_ARG
    for c in (0, -5):
        assert sgd(h, counts=(ctypes.c_int64 * 3)(5, c, 7)) == E_ARG and b"out of range" in last_error()
    assert sgd(h, scratch_bytes=h.scratch_bytes - 1) == E_SCRATCH
    assert sgd(h, scratch_bytes=h.scratch_bytes - 1, mom=h.f(0.0), m=None) == E_SCRATCH  # momentum 0: valid up to the scratch


def test_multi_adam_rejects_bad_arguments_without_launching():
    h = Host()
    assert adam(h, n=-1) == E_ARG
    for k in ("params", "m", "v", "steps", "b2", "eps"):
        assert adam(h, **{k: None}) == E_ARG, k
    one_null = (ctypes.c_void_p * 3)(h.ptrs[0], h.ptrs[0], None)
    for k in ("grads", "m", "v", "steps"):
        assert adam(h, **{k: one_null}) == E_ARG and b"segment 2" in last_error(), k
    nan = float("nan")
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-3), (nan, 0.999), (0.9, nan)):
        assert adam(h, b1=h.f(b1), b2=h.f(b2)) == E_ARG and b"betas" in last_error(), (b1, b2)
    for eps in (0.0, -1e-8, nan):
        assert adam(h, eps=h.f(eps)) == E_ARG, eps
    assert adam(h, counts=(ctypes.c_int64 * 3)(5, 0, 7)) == E_ARG
    assert adam(h, scratch_bytes=h.scratch_bytes - 1) == E_SCRATCH


# ------------------------------------------------------------------------------------------------- optimizer classes
def params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]


@pytest.mark.parametrize("kw", [dict(nesterov=True, momentum=0.9), dict(dampening=0.1), dict(maximize=True), dict(fused=True),
                                dict(differentiable=True), dict(lr=torch.tensor(0.1))])
def test_sgd_refuses_unsupported_options(kw):
    with pytest.raises(ValueError, match="not supported"):
        optim.SGD(params(), **dict(dict(lr=0.1), **kw))


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(fused=True), dict(capturable=True),
                                dict(differentiable=True), dict(decoupled_weight_decay=True), dict(lr=torch.tensor(1e-3)),
                                dict(betas=(torch.tensor(0.9), 0.999))])
def test_adam_refuses_unsupported_options(kw):
    with pytest.raises(ValueError, match="not supported"):
        optim.Adam(params(), **kw)


def test_groups_must_share_max_grad_norm():
    a, b = params()
    with pytest.raises(ValueError, match="same max_grad_norm"):
        optim.SGD([{"params": [a]}, {"params": [b], "max_grad_norm": 2.0}], lr=0.1, max_grad_norm=1.0)
    opt = optim.Adam([a], max_grad_norm=1.0)
    with pytest.raises(ValueError, match="same max_grad_norm"):
        opt.add_param_group({"params": [b], "max_grad_norm": 0.5})
    with pytest.raises(ValueError, match="not supported"):
        opt.add_param_group({"params": [b], "amsgrad": True})
    assert len(opt.param_groups) == 1
    opt.add_param_group({"params": [b], "lr": 0.5})
    assert opt.param_groups[1]["max_grad_norm"] == 1.0


def test_step_rejects_tensors_the_kernels_cannot_take():
    p = torch.nn.Parameter(torch.randn(4, 4, dtype=torch.float64))
    p.grad = torch.ones_like(p)
    with pytest.raises(TypeError, match="float32"):
        optim.SGD([p], lr=0.1).step()
    q = torch.nn.Parameter(torch.randn(4, 4))
    q.grad = torch.ones(4, 4).t()
    with pytest.raises(ValueError, match="contiguous"):
        optim.SGD([q], lr=0.1).step()
    q.grad = torch.ones(4, 4).to_sparse()
    with pytest.raises(TypeError, match="sparse"):
        optim.SGD([q], lr=0.1).step()


def _grads(ps, step, scale):
    gen = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(ps):
        p.grad = None if (i == 1 and step == 1) else torch.randn(p.shape, generator=gen) * scale  # a None gradient at step 1


@pytest.mark.parametrize("kind", ("sgd", "sgd0", "adam"))
@pytest.mark.parametrize("max_norm", (0.0, 1.0))
def test_cpu_parameters_follow_torch_bitwise(kind, max_norm):
    """CPU parameters: clip_grad_norm_ and then torch's single-tensor optimizer -- the same bits as writing them out."""
    ours, ref = params(), params()
    groups = lambda ps: [{"params": [ps[0]]}, {"params": [ps[1]], "lr": 0.03, "weight_decay": 1e-2}]
    if kind == "adam":
        opt = optim.Adam(groups(ours), lr=1e-2, weight_decay=1e-3, max_grad_norm=max_norm)
        tref = torch.optim.Adam(groups(ref), lr=1e-2, weight_decay=1e-3)
    else:
        mom = 0.9 if kind == "sgd" else 0.0
        opt = optim.SGD(groups(ours), lr=0.1, momentum=mom, weight_decay=1e-3, max_grad_norm=max_norm)
        tref = torch.optim.SGD(groups(ref), lr=0.1, momentum=mom, weight_decay=1e-3)
    for s in range(4):
        _grads(ours, s, 3.0)
        _grads(ref, s, 3.0)
        opt.step()
        if max_norm > 0:
            norm = torch.nn.utils.clip_grad_norm_([p for p in ref if p.grad is not None], max_norm)
            assert torch.equal(opt.grad_norm, norm)
        else:
            assert opt.grad_norm is None
        tref.step()
        for a, b in zip(ours, ref):
            assert torch.equal(a, b), (kind, s)
    if kind == "adam":
        assert float(opt.state[ours[1]]["step"]) == 3.0 and float(opt.state[ours[0]]["step"]) == 4.0  # the None step did not count


@pytest.mark.parametrize("kind", ("sgd", "adam"))
def test_state_dict_round_trip_with_torch(kind):
    """ours -> torch.optim -> ours: the state moves in torch's format and the trajectories stay bitwise equal (CPU)."""
    make = {"sgd": (lambda ps, cls: cls(ps, lr=0.1, momentum=0.9, weight_decay=1e-3)),
            "adam": (lambda ps, cls: cls(ps, lr=1e-2, weight_decay=1e-3))}[kind]
    cls = optim.SGD if kind == "sgd" else optim.Adam
    tcls = torch.optim.SGD if kind == "sgd" else torch.optim.Adam
    a, b = params(), params()
    opt_a = make(a, cls)
    opt_b = make(b, tcls)
    for s in range(2):
        _grads(a, s + 5, 1.0)
        _grads(b, s + 5, 1.0)
        opt_a.step()
        opt_b.step()
    sd = opt_a.state_dict()
    if kind == "adam":
        assert sd["state"][0]["step"].device.type == "cpu" and sd["state"][0]["step"].dtype == torch.float32
    else:
        assert set(sd["state"][0]) == {"momentum_buffer"}
    t2 = make(b, tcls)
    t2.load_state_dict(sd)  # ours -> torch
    o2 = make(a, cls)
    o2.load_state_dict(opt_b.state_dict())  # torch -> ours
    assert o2.param_groups[0]["max_grad_norm"] == 0.0
    for s in range(2):
        _grads(a, s + 9, 1.0)
        _grads(b, s + 9, 1.0)
        o2.step()
        t2.step()
        for x, y in zip(a, b):
            assert torch.equal(x, y), s


def test_closure_and_zero_grad():
    ps = params()
    opt = optim.SGD(ps, lr=0.1, momentum=0.9)

    def closure():
        opt.zero_grad()
        loss = sum((p * p).sum() for p in ps)
        loss.backward()
        return loss

    before = [p.detach().clone() for p in ps]
    loss = opt.step(closure)
    assert float(loss.detach()) > 0
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b - 0.1 * 2 * b)
    opt.zero_grad()
    assert all(p.grad is None for p in ps)
