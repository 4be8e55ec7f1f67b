"""Which run form every public call of NnueTrainer takes: a recorder and the scripted calls it is held to.

tests/test_gpu_step_trace.py runs ``SCENARIOS`` and wants tests/golden/step_trace.json, which
tests/golden/make_golden_step_trace.py recorded with this same module at the commit before ``step`` and ``step_many`` got
one driver (step_mode.step_form).  The recorder patches only ``lib._call``, ``lib.run_plan``, ``torch.cuda.CUDAGraph.replay``
and the ``torch.distributed`` collectives -- nothing private to the trainer -- so it runs on any commit that keeps the
attribute names it reads afterwards (``_g_local``, ``_g_update``, ``steps_done``, ``lr_position``, ``_last_alt``,
``capture_collectives``).  No tensor value is recorded: bits are held by the trainer, data-parallel and resume tests.

Per call the trace holds
* ``events``, space separated and in order: C entry points (``nnue_`` dropped) whether a wrapper or a recorded plan issued them,
  ``replay[KEY]`` (the ``_g_local`` key or ``update``, found by identity) and ``KIND(COUNT,async|sync)`` for a collective.  What
  happens while a plan is being recorded is prefixed ``rec:``, what happens under stream capture ``cap:``;
* ``state`` after the call: the ``_g_local`` keys, whether ``_g_update`` exists, and the four counters and flags.
"""
import contextlib
import os
import socket
from typing import Dict, List

import torch

import nnue

from trainer_modes import KNOBS as MODE_KNOBS

KNOBS = tuple(MODE_KNOBS) + ("NNUE_DP_ASYNC_OP",)
OPT = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0)
SHAPES = {  # feature grid, further model arguments, batch, image side
    "main": ((10, 8), {}, 32, 32),                        # tests/test_gpu_trainer.py, test_gpu_dp.py
    "second": ((16, 32), dict(input_size=64), 64, 64),    # tests/test_gpu_update_sequence.py (two maps, factor exchange)
}
COLLECTIVES = ("all_reduce", "all_gather", "all_gather_into_tensor", "reduce_scatter_tensor", "broadcast")


def key_name(key) -> str:
    lead, kind = key
    return f"{','.join(map(str, lead)) if isinstance(lead, tuple) else lead}/{kind}"


class Recorder:
    """Context manager around ONE public call of trainer `tr`; ``events`` afterwards."""

    def __init__(self, tr):
        self.tr, self.events = tr, []

    def _add(self, what: str) -> None:
        from nnue_hip import lib
        where = "cap:" if torch.cuda.is_current_stream_capturing() else ("rec:" if lib._recording is not None else "")
        self.events.append(where + what)

    def _graph_name(self, graph) -> str:
        if graph is self.tr._g_update:
            return "update"
        for key, held in self.tr._g_local.items():
            if graph is (held[0] if isinstance(held, tuple) else held):
                return key_name(key)
        return "unknown"

    def __enter__(self):
        import torch.distributed as dist
        from nnue_hip import lib
        self._lib, self._dist = lib, dist
        self._saved = (lib._call, lib.run_plan, torch.cuda.CUDAGraph.replay, {k: getattr(dist, k) for k in COLLECTIVES})
        call, run_plan, replay, collectives = self._saved

        def log_call(name, *args):
            self._add(name[5:])
            call(name, *args)

        def log_plan(plan, stream_ptr, timers=None):
            for c in plan:
                self._add(c[0][5:])
            run_plan(plan, stream_ptr, timers)

        def log_replay(graph):
            self._add(f"replay[{self._graph_name(graph)}]")
            replay(graph)

        def logged(kind, fn):
            def collective(*args, **kw):
                # the element count on the wire's side: the gathered output, the scattered or reduced input
                t = args[1] if kind in ("all_gather", "reduce_scatter_tensor") else args[0]
                self._add(f"{kind}({t.numel()},{'async' if kw.get('async_op') else 'sync'})")
                return fn(*args, **kw)
            return collective

        lib._call, lib.run_plan, torch.cuda.CUDAGraph.replay = log_call, log_plan, log_replay
        for kind, fn in collectives.items():
            setattr(dist, kind, logged(kind, fn))
        return self

    def __exit__(self, *exc):
        self._lib._call, self._lib.run_plan, torch.cuda.CUDAGraph.replay, collectives = self._saved
        for kind, fn in collectives.items():
            setattr(self._dist, kind, fn)
        return False


def state_of(tr) -> Dict:
    return dict(keys=sorted(key_name(k) for k in tr._g_local), update_graph=tr._g_update is not None, steps_done=int(tr.steps_done),
                lr_position=int(tr.lr_position), last_alt=bool(tr._last_alt), capture_collectives=bool(tr.capture_collectives))


# ---- the scripted calls.  An op is (label, kind, arguments):
#   ("step", dict(slot=, n=, timers=, global_count=, soft=))   n: copy a batch of n images in (None: train on the slot)
#   ("many", slots, timers)      ("set", attribute, value)     ("schedule", values | None)     ("reload",)
def step(slot=0, n=None, timers=False, global_count=None, soft=False):
    return ("step", dict(slot=slot, n=n, timers=timers, global_count=global_count, soft=soft))


def many(*slots, timers=False):
    return ("many", tuple(slots), timers)


SINGLE_STEPS = [step(n="B"), step(), step(), step(slot=2), step(slot=1, n="short"), step(slot=1), step(slot=1, timers=True)]
HYPER = [("set", "lr", 5e-4), step(), ("set", "momentum", 0.8), step(), step(), ("set", "label_smoothing", 0.1), step(), step(slot=2),
         ("schedule", (1e-3, 5e-4, 2e-4)), step(), many(0, 1), ("reload",), step(slot=1), ("schedule", None), step()]
GROUPS = [many(0, 1, 2), many(0, 1, 2), many(0, 1, 2), many(1, 0), many(0, 1, 2, timers=True), ("set", "momentum", 0.8), many(0, 1, 2),
          step(slot=1), many(1, 0)]
DP_STEPS = [step(n="B"), step(), step(), step(slot=2), step(slot=1, n="short", global_count="n"), step(slot=1), step(slot=1, timers=True),
            many(0, 1), many(0, 1, timers=True)]
FORCED = {"NNUE_DP_FORCE_COLLECTIVES": "1"}
TABLE = {"NNUE_FUSE_TABLE_UPDATE": "1"}


def _both(ops):
    """The same calls with and without graphs."""
    return [(dict(use_graph=True), ops), (dict(use_graph=False), ops)]


# name -> (shape, process group, environment, [(trainer arguments, ops)])
SCENARIOS = {
    "graph": ("main", None, {}, [(dict(use_graph=True), SINGLE_STEPS + HYPER)]),
    "eager": ("main", None, {}, [(dict(use_graph=False), [many(0, 1, timers=True)] + SINGLE_STEPS + [many(0, 1, 2), many(0, 1, 2, timers=True)])]),
    "groups": ("main", None, {}, [(dict(use_graph=True), GROUPS)]),
    "two_labels": ("main", None, {}, [(dict(use_graph=True, two_labels=True),
                                         [step(n="B", soft=True), step(n="B", soft=True), step(n="short", soft=True), step(n="short"), step()])]),
    "two_maps": ("second", None, TABLE, [(dict(use_graph=True), [step(), step(slot=1)] + GROUPS),
                                         (dict(use_graph=False), [step(), many(0, 1), many(0, 1, timers=True), step()])]),
    "gloo_one_message": ("main", "gloo", FORCED, _both(DP_STEPS)),
    "gloo_one_message_async": ("main", "gloo", {**FORCED, "NNUE_DP_ASYNC_OP": "1"}, _both(DP_STEPS)),
    "gloo_two_buckets": ("main", "gloo", {**FORCED, "NNUE_DP_BUCKETS": "2"}, _both(DP_STEPS)),
    "gloo_sharded": ("main", "gloo", {**FORCED, "NNUE_DP_SHARDED_UPDATE": "1"}, _both(DP_STEPS)),
    "gloo_factors": ("second", "gloo", {**FORCED, **TABLE, "NNUE_DP_FACTOR_EXCHANGE": "1"}, _both(DP_STEPS + [many(0, 1, 2, timers=True)])),
    "rccl_captured": ("main", "nccl", FORCED, [(dict(use_graph=True), DP_STEPS[:7] + GROUPS)]),
    "rccl_captured_factors": ("second", "nccl", {**FORCED, **TABLE, "NNUE_DP_FACTOR_EXCHANGE": "1"},
                              [(dict(use_graph=True), [step(), step(), step(slot=1), many(0, 1, 2), many(0, 1), step(), many(0, 1)])]),
}


def off_form(name: str):
    """The developer knob in the environment that takes scenario `name` off its form, or None."""
    env = SCENARIOS[name][2]
    for knob in KNOBS:
        if knob in os.environ and os.environ[knob] != env.get(knob):
            return f"{knob}={os.environ[knob]} in the environment (the scenario {'sets ' + env[knob] if knob in env else 'leaves it unset'})"
    return None


@contextlib.contextmanager
def _group(backend, tmp_dir):
    """A one-rank process group, made and destroyed here (gloo over a file store; RCCL the way test_gpu_step_shapes.py's
    one_rank_rccl fixture makes it)."""
    import torch.distributed as dist
    if backend is None:
        yield
        return
    saved = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    if backend == "gloo":
        dist.init_process_group("gloo", store=dist.FileStore(os.path.join(str(tmp_dir), "store"), 1), rank=0, world_size=1)
    else:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", torch.cuda.current_device()))
    try:
        yield
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _apply(tr, op, batch):
    kind = op[0]
    if kind == "step":
        a = op[1]
        kw = dict(slot=a["slot"], timers={} if a["timers"] else None)
        if a["n"] is not None:
            n = tr.B if a["n"] == "B" else tr.B - 12
            kw.update(images=batch[0][:n], labels=batch[1][:n])
            if a["soft"]:
                kw.update(labels_b=batch[2][:n], lam=batch[3][:n])
            if a["global_count"] is not None:
                kw.update(global_count=n)
        tr.step(**kw)
    elif kind == "many":
        tr.step_many(op[1], timers={} if op[2] else None)
    elif kind == "set":
        setattr(tr, op[1], op[2])
    elif kind == "schedule":
        tr.clear_lr_schedule() if op[1] is None else tr.set_lr_schedule(list(op[1]))
    elif kind == "reload":
        tr.load_state_dict(tr.state_dict())
    else:
        raise KeyError(kind)


def label_of(op) -> str:
    if op[0] == "step":
        return "step(" + ", ".join(f"{k}={v}" for k, v in op[1].items() if v not in (None, False)) + ")"
    return f"{op[0]}({', '.join(map(str, op[1:]))})"


def run_scenario(name: str, tmp_dir) -> List[Dict]:
    """The trace of scenario `name`: one record per scripted call.  The scenario's knobs are set for its duration."""
    from nnue_hip.trainer import NnueTrainer
    shape, backend, env, trainers = SCENARIOS[name]
    grid, model_args, B, side = SHAPES[shape]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    out = []
    try:
        with _group(backend, tmp_dir):
            for t, (kw, ops) in enumerate(trainers):
                torch.manual_seed(0)
                model = nnue.NNUE(nnue.GridFeatureSet(*grid), 256, 32, 16, num_classes=10, **model_args).to("cuda")
                tr = NnueTrainer(model, B, (side, side), input_slots=3, **OPT, **kw)
                gen = torch.Generator().manual_seed(5)
                for images, labels in tr.inputs:
                    images.copy_(torch.randn(B, 3, side, side, generator=gen))
                    labels.copy_(torch.randint(0, 10, (B,), generator=gen))
                batch = (torch.randn(B, 3, side, side, generator=gen).cuda(), torch.randint(0, 10, (B,), generator=gen).cuda(),
                         torch.randint(0, 10, (B,), generator=gen).cuda(), torch.rand(B, generator=gen).cuda())
                for op in ops:
                    with Recorder(tr) as rec:
                        _apply(tr, op, batch)
                    out.append(dict(trainer=t, call=label_of(op), events=" ".join(rec.events), state=state_of(tr)))
                torch.cuda.synchronize()
                del tr
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return out
