"""Drop-in torch optimizers whose GPU step runs on the multi-tensor HIP kernels (nnue_multi_sgd_step / nnue_multi_adam_step).

The reference's inner loop (train.py:359-366) ends in ``clip_grad_norm_`` and ``optimizer.step()`` on the optimizer
``create_optimizer`` builds (train.py:455-471).  With these classes the clip is part of the step::

    optimizer = nnue_hip.optim.SGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=wd, max_grad_norm=max_grad_norm)
    ...
    loss.backward()
    optimizer.step()            # clip_grad_norm_ + SGD in two launches; optimizer.grad_norm = the pre-clip norm

``weight_clip`` (a per-group option, 0 = off; the keyword is the groups' default) clamps every parameter of the group to
[-weight_clip, weight_clip] inside the update launch -- the reference's ``_clip_weights`` (nnue.py:528-539) at 1.0, for a group
holding ``input.weight`` and the classifier's three weights; the rest goes into a group without it.

``ema_decay`` (a per-group option, 0 = off, else in (0, 1); the keyword is the groups' default) keeps a moving average of every
parameter of the group in ``state[p]["ema"]`` -- a clone of the parameter made at its first step, then moved by the update launch
itself: ``e <- fmaf(omd, p_new - e, e)`` with omd = float32(1 - ema_decay) (include/nnue_hip.h, "weight average").
``optimizer.ema_state()`` returns {parameter: its average}.

They subclass ``torch.optim.SGD`` / ``torch.optim.Adam``: the constructor signature, ``param_groups``, ``zero_grad``,
hooks, schedulers and the ``state_dict`` format are torch's own, so a checkpoint moves between these and torch's
optimizers (and ``NnueTrainer.optimizer_state_dict()``) in both directions.  Options the kernels do not implement are
refused when the optimizer is built; tensors they cannot take are refused at ``step()``.

Parameters on the CPU take the same formulas in stock torch (``clip_grad_norm_``, then torch's single-tensor optimizer),
as the rest of the module surface does.  Parameters on the GPU always take the HIP kernels.
"""
import ctypes
from typing import List, Optional

import torch

from . import lib

__all__ = ["SGD", "Adam"]

_P = ctypes.c_void_p


def _refuse(cond: bool, what: str) -> None:
    if cond:
        raise ValueError(f"nnue_hip.optim: {what} is not supported by the HIP optimizer kernels")


class _Table:
    """The host arrays of one segment list, kept between steps and refilled in place (no allocation after the first step)."""

    FIELDS = ("params", "grads", "m", "v", "steps", "counts", "lr", "a", "b", "eps", "wd", "first", "clip", "ema", "omd")

    def __init__(self, params: List[torch.Tensor]):
        n = self.n = len(params)
        self.params, self.grads, self.m, self.v, self.steps, self.ema = ((_P * n)() for _ in range(6))
        self.counts = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        self.lr, self.a, self.b, self.eps, self.wd, self.clip, self.omd = ((ctypes.c_float * n)() for _ in range(7))
        self.first = (ctypes.c_int32 * n)()
        self.addr = {k: ctypes.addressof(getattr(self, k)) for k in self.FIELDS}
        dev = params[0].device
        nbytes = int(lib.load().nnue_multi_optim_scratch(self.addr["counts"], n))
        self.scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.norm = torch.zeros((), dtype=torch.float32, device=dev)


_GLOBAL_CLIP = ("nnue_hip.optim: every param group must have the same max_grad_norm (the clip is global, as "
                "clip_grad_norm_(model.parameters()))")


class _MultiTensor:
    """What SGD and Adam share: option checks, the segment list, the CPU / GPU split and the state hand-over.  Mixed in
    ahead of torch's class, whose constructor, param_groups, zero_grad, hooks and state_dict stay as they are."""

    def _setup(self) -> None:
        self.defaults["max_grad_norm"] = self._max_grad_norm
        self.defaults["weight_clip"] = self._weight_clip
        self.defaults["ema_decay"] = self._ema_decay
        self.grad_norm: Optional[torch.Tensor] = None  # the pre-clip norm of the last step (a device scalar; None: no clip)
        self._table: Optional[_Table] = None
        self._key = None

    def add_param_group(self, param_group: dict) -> None:
        param_group.setdefault("max_grad_norm", self._max_grad_norm)
        if param_group["max_grad_norm"] != self._max_grad_norm:
            raise ValueError(_GLOBAL_CLIP)
        param_group.setdefault("weight_clip", self._weight_clip)
        param_group.setdefault("ema_decay", self._ema_decay)
        super().add_param_group(param_group)
        try:
            self._check_group(self.param_groups[-1])
        except ValueError:
            self.param_groups.pop()
            raise

    def _check_group(self, g: dict) -> None:
        g["weight_clip"] = lib.checked_weight_clip(g.get("weight_clip", 0.0))
        g["ema_decay"] = lib.checked_ema_decay(g.get("ema_decay", 0.0))
        _refuse(isinstance(g["lr"], torch.Tensor), "a tensor lr")
        _refuse(isinstance(g["weight_decay"], torch.Tensor), "a tensor weight_decay")
        for k in ("maximize", "fused", "capturable", "differentiable"):
            _refuse(bool(g.get(k)), f"{k}=True")

    def load_state_dict(self, state_dict: dict) -> None:
        own = [(g["weight_clip"], g["ema_decay"]) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, (clip, decay) in zip(self.param_groups, own):  # a torch.optim state_dict has no max_grad_norm: ours stays
            g["max_grad_norm"] = self._max_grad_norm
            g.setdefault("weight_clip", clip)  # (a group option like any other: the dict's value where it has one)
            g.setdefault("ema_decay", decay)
            self._check_group(g)
        self._key = None  # the state tensors were replaced

    def _segments(self):
        """[(param, group)] of the parameters with a gradient, in param_groups order, and the device they share."""
        segs, device = [], None
        for g in self.param_groups:
            for p in g["params"]:
                gr = p.grad
                if gr is None:
                    continue
                if p.dtype != torch.float32 or gr.dtype != torch.float32:
                    raise TypeError(f"nnue_hip.optim: parameters and gradients must be float32, got {p.dtype} / {gr.dtype}")
                if gr.is_sparse or p.is_sparse:
                    raise TypeError("nnue_hip.optim: sparse parameters or gradients are not supported")
                if not (p.is_contiguous() and gr.is_contiguous()):
                    raise ValueError("nnue_hip.optim: parameters and gradients must be contiguous")
                if gr.device != p.device or (device is not None and p.device != device):
                    raise ValueError("nnue_hip.optim: all parameters and gradients must be on one device")
                device = p.device
                segs.append((p, g))
        return segs, device

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        segs, device = self._segments()
        if not segs:
            return loss
        max_norm = self._max_grad_norm
        if device.type != "cuda":  # the CPU convenience path: the same formulas in stock torch
            self.grad_norm = torch.nn.utils.clip_grad_norm_([p for p, _ in segs], max_norm, foreach=False) if max_norm > 0 else None
            # a new average starts as the parameter it follows: cloned before the update, entered into the state after it (torch's
            # Adam creates its own state only in an empty dict)
            new = {p: p.detach().clone(memory_format=torch.contiguous_format) for p, g in segs
                   if g["ema_decay"] and self.state.get(p, {}).get("ema") is None}
            super().step()
            for p, e in new.items():
                self.state[p]["ema"] = e
            for (p, g), before in zip(segs, self._averages(segs)):
                if g["weight_clip"] > 0:
                    p.clamp_(-g["weight_clip"], g["weight_clip"])
                if before is not None:
                    before.lerp_(p, lib.ema_omd(g["ema_decay"]))
            return loss
        key = tuple(id(p) for p, _ in segs)
        if key != self._key:  # a new set of parameters with gradients (or new state tensors): new arrays
            self._table = _Table([p for p, _ in segs])
            self._key = key
        t = self._table
        for i, (p, g) in enumerate(segs):
            t.params[i] = p.data_ptr()
            t.grads[i] = p.grad.data_ptr()
            t.lr[i] = g["lr"]  # read at every step: schedulers work unchanged
            t.wd[i] = g["weight_decay"]
            t.clip[i] = g["weight_clip"]  # the group's weight clip (0: the segment is not clamped)
        self._fill_state(t, segs)
        for i, ((p, g), e) in enumerate(zip(segs, self._averages(segs))):  # (after _fill_state: Adam's lazy state asks for an empty dict)
            t.ema[i] = None if e is None else _state_buffer(self.state[p], "ema", p).data_ptr()
            t.omd[i] = 0.0 if e is None else lib.ema_omd(g["ema_decay"])
        norm_out = t.norm.data_ptr() if max_norm > 0 else None
        self._launch(t, max_norm, norm_out, torch.cuda.current_stream(device).cuda_stream)
        self.grad_norm = t.norm if max_norm > 0 else None
        return loss


    def _averages(self, segs):
        """Per segment the parameter's average (``state[p]["ema"]``, a clone of the parameter where the group asks for one and
        there is none yet) or None."""
        out = []
        for p, g in segs:
            if not g["ema_decay"]:
                out.append(None)
                continue
            st = self.state[p]
            if st.get("ema") is None:
                st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
            out.append(st["ema"])
        return out

    def ema_state(self) -> dict:
        """{parameter: its moving average} for every parameter that has one (a group with ema_decay > 0, after its first step)."""
        return {p: self.state[p]["ema"] for g in self.param_groups for p in g["params"] if self.state.get(p, {}).get("ema") is not None}


def _state_buffer(state: dict, key: str, p: torch.Tensor) -> torch.Tensor:
    buf = state[key]
    if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != p.device or buf.shape != p.shape:
        raise ValueError(f"nnue_hip.optim: state '{key}' must be a contiguous float32 tensor shaped and placed like its parameter")
    return buf


class SGD(_MultiTensor, torch.optim.SGD):
    """``torch.optim.SGD`` with ``clip_grad_norm_(params, max_grad_norm)`` folded into ``step()`` when max_grad_norm > 0,
    on the HIP kernels for GPU parameters.  nesterov, dampening != 0, maximize, fused and differentiable are refused.
    ``foreach`` is accepted and ignored (the CPU path is torch's single-tensor form)."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, *, maximize: bool = False, foreach: Optional[bool] = None, differentiable: bool = False,
                 fused: Optional[bool] = None, max_grad_norm: float = 0.0, weight_clip: float = 0.0, ema_decay: float = 0.0):
        _refuse(bool(nesterov), "nesterov=True")
        _refuse(dampening != 0, "dampening != 0")
        _refuse(bool(maximize), "maximize=True")
        _refuse(bool(fused), "fused=True")
        _refuse(bool(differentiable), "differentiable=True")
        _refuse(isinstance(lr, torch.Tensor), "a tensor lr")
        self._max_grad_norm = float(max_grad_norm)
        self._weight_clip = lib.checked_weight_clip(weight_clip)  # the default of a group that does not set its own
        self._ema_decay = lib.checked_ema_decay(ema_decay)        # likewise
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         maximize=maximize, foreach=False, differentiable=differentiable, fused=fused)
        self._setup()

    def _check_group(self, g: dict) -> None:
        super()._check_group(g)
        _refuse(bool(g["nesterov"]), "nesterov=True")
        _refuse(g["dampening"] != 0, "dampening != 0")

    def _fill_state(self, t: _Table, segs) -> None:
        for i, (p, g) in enumerate(segs):
            mom = g["momentum"]
            t.a[i] = mom
            if mom == 0:  # torch keeps no buffer
                t.m[i] = None
                continue
            st = self.state[p]
            if st.get("momentum_buffer") is None:  # torch's first step: the buffer is the gradient itself, written not read
                st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                t.first[i] = 1
            else:
                t.first[i] = 0
            t.m[i] = _state_buffer(st, "momentum_buffer", p).data_ptr()

    def _launch(self, t: _Table, max_norm: float, norm_out, stream: int) -> None:
        A = t.addr
        if any(t.ema):
            lib._call("nnue_multi_sgd_step_ema", A["params"], A["grads"], A["m"], A["counts"], t.n, A["lr"], A["a"], A["wd"], A["first"],
                      A["clip"], max_norm, norm_out, t.scratch.data_ptr(), t.scratch.numel(), None, A["ema"], A["omd"], stream)
            return
        if any(t.clip):
            lib._call("nnue_multi_sgd_step_clip", A["params"], A["grads"], A["m"], A["counts"], t.n, A["lr"], A["a"], A["wd"], A["first"],
                      A["clip"], max_norm, norm_out, t.scratch.data_ptr(), t.scratch.numel(), None, stream)
            return
        lib._call("nnue_multi_sgd_step", A["params"], A["grads"], A["m"], A["counts"], t.n, A["lr"], A["a"], A["wd"], A["first"],
                  max_norm, norm_out, t.scratch.data_ptr(), t.scratch.numel(), None, stream)


class Adam(_MultiTensor, torch.optim.Adam):
    """``torch.optim.Adam`` (L2 weight decay) with ``clip_grad_norm_(params, max_grad_norm)`` folded into ``step()`` when
    max_grad_norm > 0, on the HIP kernels for GPU parameters.  amsgrad, decoupled_weight_decay, maximize, capturable, fused
    and differentiable are refused.  The step counts live on the device for the kernels; ``state[p]["step"]`` is kept as
    torch keeps it (a CPU float tensor), so ``state_dict()`` is torch's format."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, foreach: Optional[bool] = None, maximize: bool = False, capturable: bool = False,
                 differentiable: bool = False, fused: Optional[bool] = None, decoupled_weight_decay: bool = False,
                 max_grad_norm: float = 0.0, weight_clip: float = 0.0, ema_decay: float = 0.0):
        _refuse(bool(amsgrad), "amsgrad=True")
        _refuse(bool(decoupled_weight_decay), "decoupled_weight_decay=True")
        _refuse(bool(maximize), "maximize=True")
        _refuse(bool(capturable), "capturable=True")
        _refuse(bool(differentiable), "differentiable=True")
        _refuse(bool(fused), "fused=True")
        _refuse(isinstance(lr, torch.Tensor), "a tensor lr")
        _refuse(any(isinstance(b, torch.Tensor) for b in betas), "tensor betas")
        self._max_grad_norm = float(max_grad_norm)
        self._weight_clip = lib.checked_weight_clip(weight_clip)  # the default of a group that does not set its own
        self._ema_decay = lib.checked_ema_decay(ema_decay)        # likewise
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=False,
                         maximize=maximize, capturable=capturable, differentiable=differentiable, fused=fused,
                         decoupled_weight_decay=decoupled_weight_decay)
        self._setup()
        self._dev_steps: Optional[torch.Tensor] = None  # one int32 counter per parameter (param_groups order), on the device
        self._dev_index = {}
        self._dev_synced = set()  # parameters whose device counter equals state["step"]

    def _check_group(self, g: dict) -> None:
        super()._check_group(g)
        _refuse(bool(g["amsgrad"]), "amsgrad=True")
        _refuse(bool(g.get("decoupled_weight_decay")), "decoupled_weight_decay=True")
        _refuse(any(isinstance(b, torch.Tensor) for b in g["betas"]), "tensor betas")

    def load_state_dict(self, state_dict: dict) -> None:
        super().load_state_dict(state_dict)
        self._dev_synced = set()

    def _fill_state(self, t: _Table, segs) -> None:
        if self._dev_steps is None:
            params = [p for g in self.param_groups for p in g["params"]]
            self._dev_index = {id(p): i for i, p in enumerate(params)}
            self._dev_steps = torch.zeros((len(params),), dtype=torch.int32, device=segs[0][0].device)
        base = self._dev_steps.data_ptr()
        steps = []
        for i, (p, g) in enumerate(segs):
            st = self.state[p]
            if "step" not in st:  # torch's lazy state (the dict may already hold a caller's "ema")
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            j = self._dev_index[id(p)]
            if id(p) not in self._dev_synced:  # new state, or loaded: the device count starts from torch's
                self._dev_steps[j].fill_(int(st["step"]))
                self._dev_synced.add(id(p))
            steps.append(st["step"])
            b1, b2 = g["betas"]
            t.a[i], t.b[i], t.eps[i] = b1, b2, g["eps"]
            t.m[i] = _state_buffer(st, "exp_avg", p).data_ptr()
            t.v[i] = _state_buffer(st, "exp_avg_sq", p).data_ptr()
            t.steps[i] = base + 4 * j
        self._host_steps = steps

    def _launch(self, t: _Table, max_norm: float, norm_out, stream: int) -> None:
        A = t.addr
        if any(t.ema):
            lib._call("nnue_multi_adam_step_ema", A["params"], A["grads"], A["m"], A["v"], A["steps"], A["counts"], t.n, A["lr"], A["a"],
                      A["b"], A["eps"], A["wd"], A["clip"], max_norm, norm_out, t.scratch.data_ptr(), t.scratch.numel(), None, A["ema"],
                      A["omd"], stream)
        elif any(t.clip):
            lib._call("nnue_multi_adam_step_clip", A["params"], A["grads"], A["m"], A["v"], A["steps"], A["counts"], t.n, A["lr"], A["a"],
                      A["b"], A["eps"], A["wd"], A["clip"], max_norm, norm_out, t.scratch.data_ptr(), t.scratch.numel(), None, stream)
        else:
            lib._call("nnue_multi_adam_step", A["params"], A["grads"], A["m"], A["v"], A["steps"], A["counts"], t.n, A["lr"], A["a"],
                      A["b"], A["eps"], A["wd"], max_norm, norm_out, t.scratch.data_ptr(), t.scratch.numel(), None, stream)
        torch._foreach_add_(self._host_steps, 1.0)  # torch's own count, on the host (what state_dict() hands on)
