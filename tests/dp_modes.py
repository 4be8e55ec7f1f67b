"""The data-parallel step modes of NnueTrainer (nnue_hip/step_mode.py::resolve under DpFacts, consumed by nnue_hip/trainer.py),
as a table of named configurations with the mode each must take, and the per-rank driver that holds three optimizer steps of
every row -- on EVERY rank -- to the float64 oracle of the global batch (trainer_modes.oracle_steps, unchanged) at
trainer_modes.compare_held's bars.  A helper, not a test module: tests/test_dp_modes_policy.py settles the table without a GPU,
tests/test_gpu_dp_modes.py runs it.

A row's ``batch`` is the rows PER RANK; rank r takes the contiguous rows [r * B, (r + 1) * B) of the real samples of a step, so
the short third step (B * world - 13 samples) leaves the last rank short or empty.  The rows of one group (world, backend) run
inside ONE mp.spawn: the NNUE_DP_* knobs are read in Python when a trainer is constructed, so rows can share a process (no row
may name a knob the C side reads once per process).  The parent computes each distinct oracle once and saves it; the workers
load it, run their rows and leave one record per row and rank.
"""
import hashlib
import json
import os
import socket
import time
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Tuple

import torch

from trainer_modes import A, BY_NAME as SINGLE, KNOBS, SHORT, CallLog, _ratio_grad, build_model, compare_held, differences, flags_of, \
    geometry, oracle_steps, same, snapshot, step_mode_of, trainer_for


@dataclass
class DpRow:
    name: str
    cfg: Dict = field(default_factory=dict)     # over trainer_modes.A; ``batch``: rows per rank
    world: int = 2
    backend: str = "gloo"                       # "gloo": the ranks share the GPU; "nccl": one rank, the collectives forced on
    env: Dict = field(default_factory=dict)     # NNUE_DP_* knobs only
    expect: Dict = field(default_factory=dict)  # StepMode fields the row must resolve to (with graphs)
    # eager steps, graph steps and step groups of one rank are bitwise the same (every kernel sums in a fixed order and the
    # collectives reduce in rank order); a row that is not says why here and its graph run is held to the oracle's bars instead
    bitwise: bool = True
    why_not_bitwise: str = ""

    @property
    def config(self) -> Dict:
        return {**A, **self.cfg}

    @property
    def group(self) -> Tuple[int, str]:
        return self.world, self.backend

    @property
    def global_config(self) -> Dict:
        """What the oracle is given: the same model on the global batch."""
        cfg = self.config
        return dict(cfg, batch=cfg["batch"] * self.world)

    @property
    def buckets(self) -> int:
        return 2 if self.env.get("NNUE_DP_BUCKETS") == "2" else 1

    def facts(self):
        from nnue_hip.step_mode import DpFacts
        return DpFacts(True, self.world, self.buckets, self.backend)

    def counts(self, step: int) -> List[int]:
        """Real samples per rank in oracle step `step` (0, 1: full; 2: B * world - SHORT over contiguous rank slices)."""
        b = self.config["batch"]
        n = b * self.world - (SHORT if step == 2 else 0)
        return [min((r + 1) * b, n) - min(r * b, n) for r in range(self.world)]


B12, B8, B24 = dict(batch=12), dict(batch=8), dict(batch=24)
BITS = dict(grid=5, fps=3, image=40)                    # 75 table rows: below the product kernels' shapes
T8192 = dict(grid=32, fps=8, image=96)                  # an 8192 x 256 table, P = F
FX, SHARD, FORCED = {"NNUE_DP_FACTOR_EXCHANGE": "1"}, {"NNUE_DP_SHARDED_UPDATE": "1"}, {"NNUE_DP_FORCE_COLLECTIVES": "1"}
AR = dict(ft_path="mfma", factor_exchange=False, sharded_update=False, grads_materialised=True, sq="none", sq_count=0,
          capture_collectives=False, defer_ste=False, ride_ste=False, ste_stages=3, fuse_table_update=False, fuse_next_forward=False)
SHARDED = dict(AR, sharded_update=True)
EXCHANGE = dict(AR, factor_exchange=True, grads_materialised=False, sq="gram", ride_dw1=False, ride_small=False,
                merged_backward_launch=False, phases=5, sq_count=32)  # (the Gram partials of 24 or 32 global rows at L1 256)

ROWS: List[DpRow] = [
    DpRow("ar", B12, expect=dict(AR, phases=51)),
    DpRow("ar_two_buckets", B12, env={"NNUE_DP_BUCKETS": "2"}, expect=dict(AR, phases=51)),
    DpRow("ar_adam", dict(B12, optimizer="adam"), expect=dict(AR, phases=51)),
    DpRow("ar_adam_k4", dict(B12, optimizer="adam", K=4), expect=dict(AR, phases=51)),
    DpRow("ar_adam_asks_exchange", dict(B12, optimizer="adam"), env={**FX, **SHARD}, expect=dict(AR, phases=51)),
    DpRow("ar_bits_k3", dict(B12, K=3, **BITS), expect=dict(AR, ft_path="bits", phases=5)),
    DpRow("ar_list", dict(SINGLE["g5_list"].cfg, batch=11), expect=dict(AR, ft_path="list", phases=5)),
    DpRow("shard", B12, env=SHARD, expect=dict(SHARDED, phases=51)),
    DpRow("shard_plain_w4", dict(B8, momentum=0.0), world=4, env=SHARD, expect=dict(SHARDED, phases=51)),
    DpRow("shard_bits_k3", dict(B12, K=3, **BITS), env=SHARD, expect=dict(SHARDED, ft_path="bits", phases=5)),
    DpRow("fx", B12, env=FX, expect=EXCHANGE),
    DpRow("fx_w4", B8, world=4, env=FX, expect=EXCHANGE),
    DpRow("fx_k4_clip", dict(B12, K=4, clip=1.0), env=FX, expect=EXCHANGE),
    DpRow("fx_no_sink", dict(B12, grid=8, fps=4), env=FX, expect=EXCHANGE),
    DpRow("fx_l1_72", dict(B12, l1=72), env=FX, expect=dict(EXCHANGE, sq_count=10)),
    DpRow("fx_next_forward", dict(T8192, batch=16), env=FX, expect=dict(EXCHANGE, fuse_next_forward=True)),
    DpRow("rccl_ar", B24, 1, "nccl", FORCED, dict(AR, phases=51, capture_collectives=True)),
    DpRow("rccl_ar_adam", dict(B24, optimizer="adam"), 1, "nccl", FORCED, dict(AR, phases=51, capture_collectives=True)),
    DpRow("rccl_shard", B24, 1, "nccl", {**FORCED, **SHARD}, dict(SHARDED, phases=51, capture_collectives=True)),
    DpRow("rccl_fx", B24, 1, "nccl", {**FORCED, **FX}, dict(EXCHANGE, capture_collectives=True)),
    DpRow("rccl_fx_next_forward", dict(T8192, batch=32), 1, "nccl", {**FORCED, **FX},
          dict(EXCHANGE, fuse_next_forward=True, capture_collectives=True)),
]
ROW_NAMES = [r.name for r in ROWS]
BY_NAME = {r.name: r for r in ROWS}
GROUPS: List[Tuple[int, str]] = sorted({r.group for r in ROWS})


def rows_of(group: Tuple[int, str]) -> List[DpRow]:
    return [r for r in ROWS if r.group == group]


def describe(row: DpRow, mode) -> str:
    """One line: StepMode.describe() plus the data-parallel part of the mode."""
    how = "factor exchange" if mode.factor_exchange else "sharded update" if mode.sharded_update else "all-reduce"
    if row.buckets == 2:
        how += ", two messages"
    return f"{mode.describe()} | {how}{', captured' if mode.capture_collectives else ''} | {row.world} x {row.backend}"


# ------------------------------------------------------------------------------------------------ the oracle, once per global batch
def oracle_key(row: DpRow) -> str:
    """Rows with the same model on the same global batch share one oracle (ar, shard, fx and the rccl rows of base A do)."""
    return hashlib.sha1(repr(sorted(row.global_config.items(), key=str)).encode()).hexdigest()[:12]


def oracle_of(row: DpRow) -> List[Dict]:
    cfg = row.global_config
    params = {k: v.detach().clone() for k, v in build_model(cfg).state_dict().items()}
    return list(oracle_steps(cfg, params))


# ------------------------------------------------------------------------------------------------ one rank's step against the oracle
def _pieces(layout, lo: int, hi: int, sink_rows, l1: int):
    """(name, start in the tensor, start in the range, length) of every tensor of `layout` inside [lo, hi) of the flat
    buffers; the table also as its rows below the sink (sink_rows; None: no clamp sink) on their own, as compare_held's split."""
    for k, shape, o in zip(layout.names, layout.shapes, layout.offsets):
        m = 1
        for d in shape:
            m *= d
        spans = [(k + " [shard]", o, o + m)]
        if k == "input.weight" and sink_rows is not None:
            spans.append((k + " (rows below the sink) [shard]", o, o + sink_rows * l1))
        for label, a, b in spans:
            a2, b2 = max(a, lo), min(b, hi)
            if b2 > a2:
                yield label, k, a2 - o, a2 - lo, b2 - a2


def check_rank_step(tr, ref: Dict, rank_rows: slice, was: Dict[str, torch.Tensor], loss: torch.Tensor, what: str,
                    ratios: Dict[str, float]) -> List[str]:
    """The per-rank form of trainer_modes.check_step, at compare_held's bars and no others: this rank's logits against the
    oracle's rows ``rank_rows`` of the global batch; the norm, and every gradient the mode materialises (the all-reduced flat
    buffer; this rank's reduce-scattered shard; under the factor exchange the head and tail summed from the gathered chunks --
    the table's rows are never formed), against the oracle's GLOBAL ones; parameters, update and momentum / Adam moments after
    the step.  The returned loss is rank-local (a short step: already times B * world / global_count): the caller records it
    and the parent holds the mean over the ranks to the oracle's.  Returns the failures instead of raising: a rank that stopped
    would leave the others inside the next collective."""
    B, world, n = tr.B, tr.dp.world, ref["images"].shape[0]
    n_r = rank_rows.stop - rank_rows.start
    torch.cuda.synchronize()
    fails: List[str] = []
    if n_r == B:
        counts = ref["n"][rank_rows]
        n_mean, n_max = tr.active_stats()
        if not (n_max == int(counts.max()) and abs(n_mean - float(counts.float().mean())) < 1e-2):
            fails.append(f"{what}: feature counts differ")
    sink = tr.F - 1 if tr.P > tr.F else None
    held = dict(optimizer=tr.optimizer, sink=sink, logits=tr.logits, norm=tr.grad_norm, params=tr.p, was=was)
    ref = dict(ref, logits=ref["logits"][rank_rows])
    views = tr.layout.views
    if tr.sharded_update:
        per = tr.layout.count // world
        lo = tr.dp.rank * per
        mom = tr.dp.shard_of(tr.flat_momentum) if tr.flat_momentum is not None else None
        held["grads"], g_ref, s_ref = {}, {}, {}
        if mom is not None:
            held["momentum"] = {}
        for label, k, at, at_shard, count in _pieces(tr.layout, lo, lo + per, sink, tr.L1):
            held["grads"][label], g_ref[label] = tr.grad_shard[at_shard:at_shard + count], ref["grads"][k].flatten()[at:at + count]
            if mom is not None:
                held["momentum"][label], s_ref[label] = mom[at_shard:at_shard + count], ref["state"][k].flatten()[at:at + count]
        ref.update(grads=g_ref, state=s_ref)
    else:
        if tr.factor_exchange:
            tail = min(tr.F - 1, tr.P)  # the first table row the product does not cover: it travels in the chunk's small part
            held["grads"] = {k: v for k, v in views(tr.flat_grads).items() if k != "input.weight"}
            held["grads"]["input.weight [tail rows]"] = views(tr.flat_grads)["input.weight"][tail:]
            ref["grads"] = dict(ref["grads"], **{"input.weight [tail rows]": ref["grads"]["input.weight"][tail:]})
        else:
            held["grads"] = views(tr.flat_grads)
        if tr.optimizer == "adam":
            held.update(exp_avg=views(tr.flat_exp_avg), exp_avg_sq=views(tr.flat_exp_avg_sq))
        elif tr.flat_momentum is not None:
            held["momentum"] = views(tr.flat_momentum)
    # the kernels divide by the rank's B and the ranks' sums are added: 1 / world and B * world / n make it the mean over n
    scale = tr.dp.grad_scale * (B * world / n)
    return fails + compare_held(held, ref, B, n_r, scale, what, ratios)


def state_tensors(tr) -> Dict[str, Dict[str, torch.Tensor]]:
    """optimizer_state_dict() -- a collective under the sharded update -- as {kind: {parameter name: CPU tensor}}."""
    sd = tr.optimizer_state_dict()["state"]
    index = {k: i for i, (k, _) in enumerate(tr.model.named_parameters())}
    out: Dict[str, Dict[str, torch.Tensor]] = {}
    for k in tr.layout.names:
        for kind, t in sd.get(index[k], {}).items():
            out.setdefault(kind, {})[k] = t.detach().cpu().clone()
    return out


def rank_snapshot(tr) -> List[torch.Tensor]:
    """What one rank's steps determine: trainer_modes.snapshot, or under the sharded update the parameters and this rank's
    own shard of the momentum (the other shards hold whatever the last gather left)."""
    if tr.sharded_update:
        return [tr.flat_params.clone()] + [tr.dp.shard_of(t).clone() for t in tr._optimizer_buffers()]
    return snapshot(tr)


# ------------------------------------------------------------------------------------------------ one row on one rank
FATAL = ("hip error", "hiperror", "illegal memory", "device-side", "unspecified launch failure")
FUSED_GROUP = ("nnue_ftm_backward_weight_update_forward", "nnue_ftm_backward_weight_update")


class _Abandoned(Exception):
    """Some rank failed a unit of the row: every rank leaves the row at the same point."""


def _feed(tr, row: DpRow, ref: Dict, rank: int):
    """This rank's rows of one oracle step; a short step passes global_count, as NnueTrainer.step documents."""
    B, n = tr.B, ref["images"].shape[0]
    rows = slice(min(rank * B, n), min((rank + 1) * B, n))
    tr.max_grad_norm = ref["max_grad_norm"]
    short = {} if n == B * row.world else dict(global_count=n)
    dev = tr.dev
    return rows, tr.step(ref["images"][rows].to(dev), ref["labels"][rows].to(dev), slot=ref["step"], **short)


def run_row(row: DpRow, rank: int, refs: List[Dict]) -> Dict:
    """Everything the table asks of one row on this rank; never raises for a failure of the row (it is recorded), only for
    what looks like a device fault: nothing more may run on the GPU then."""
    import contextlib
    import torch.distributed as dist
    cfg, world, t0 = row.config, row.world, time.time()
    rec = dict(row=row.name, rank=rank, fails=[], ratios={}, steps=[], done=[])
    fails = rec["fails"]
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(row.env)

    def agree(ok: bool) -> bool:  # NnueTrainer._ranks_agree's pattern
        if world <= 1:
            return ok
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device="cuda" if row.backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(int(flag.item()))

    def unit(what: str, fn):
        """One stretch in which every rank reaches the same collectives: a Python exception on this rank is the row's failure,
        and after it all ranks decide together (a MIN all-reduce) whether the row goes on."""
        out, ok = None, True
        try:
            out = fn()
        except Exception as exc:  # noqa: BLE001
            if any(s in str(exc).lower() for s in FATAL):
                raise
            fails.append(f"{row.name} {what}: {type(exc).__name__}: {exc}")
            ok = False
        if not agree(ok):
            raise _Abandoned(what)
        return out

    with contextlib.ExitStack() as stack:
        try:
            # ---- 1. the mode
            eager, _ = unit("eager trainer", lambda: stack.enter_context(trainer_for(cfg, use_graph=False, input_slots=3)))
            single, _ = unit("graph trainer", lambda: stack.enter_context(trainer_for(cfg, use_graph=True, input_slots=3)))
            group, _ = unit("group trainer", lambda: stack.enter_context(trainer_for(cfg, use_graph=True, input_slots=3)))
            for tr, graphs in ((eager, False), (single, True), (group, True)):
                want = dict(row.expect, capture_collectives=row.expect["capture_collectives"] and graphs)
                fails.extend(f"{row.name}: " + d for d in differences({k: getattr(tr.mode, k) for k in want}, want))
                sm = step_mode_of(cfg, dp=row.facts(), use_graph=graphs, count=tr.layout.count)
                if tr.mode != sm:
                    fails.append(f"{row.name}: the trainer resolved {tr.mode}, the launch-free queries {sm}")
                flags = dict(flags_of(tr), factor_exchange=tr.factor_exchange, sharded_update=tr.sharded_update,
                             capture_collectives=tr.capture_collectives, grads_materialised=tr.grads_materialised)
                stated = [k for k in flags if k in sm.__dataclass_fields__ and k not in ("sq", "ste_chunks")]
                fails.extend(f"{row.name}: the trainer's " + d for d in differences(flags, {k: getattr(sm, k) for k in stated}))
                if (tr.dp.world, tr.dp.collectives, tr.dp.buckets, tr.dp.backend) != (world, True, row.buckets, row.backend):
                    fails.append(f"{row.name}: the process group is {tr.dp.world} x {tr.dp.backend}, collectives {tr.dp.collectives}")
                plain = cfg["optimizer"] == "adam" or not cfg["momentum"]  # no momentum buffer
                if (tr.bucket_plan is not None) != (cfg["K"] > 1) or (tr.flat_momentum is None) != plain:
                    fails.append(f"{row.name}: grouped classifier / momentum buffer do not follow the configuration")
            rec["mode"] = describe(row, single.mode)
            rec["done"].append("mode")
            # ---- 2. three eager steps against the oracle
            states, losses = [], []
            for ref in refs:
                s = ref["step"]

                def eager_step(ref=ref, s=s):
                    was = {k: v.detach().clone() for k, v in eager.p.items()}
                    with CallLog() as seen:
                        rows, loss = _feed(eager, row, ref, rank)
                    if s == 1:  # steady state: the plans ran; the sharded update and the exchange issue their update through the wrappers
                        direct = eager.sharded_update or eager.factor_exchange
                        rec["launches"] = [name for route, name, _ in seen.entries if route == "plan" or direct]
                    fails.extend(check_rank_step(eager, ref, rows, was, loss, f"{row.name} rank {rank} step {s}", rec["ratios"]))
                    states.append(rank_snapshot(eager))
                    losses.append(loss.clone())
                    rec["steps"].append(dict(loss=float(loss), norm=float(eager.grad_norm), params=eager.flat_params.cpu().clone(),
                                             buffers=[] if eager.sharded_update else [t.cpu().clone() for t in eager._optimizer_buffers()],
                                             state=state_tensors(eager)))
                unit(f"eager step {s}", eager_step)
            rec["done"].append("eager")
            # ---- 3. the same steps as graph steps (gloo: local graph + eager collective + update graph; nccl: one graph)
            graph_ratios: Dict[str, float] = {}
            for ref in refs:
                s = ref["step"]

                def graph_step(ref=ref, s=s):
                    for tr in (single, group):
                        was = {k: v.detach().clone() for k, v in tr.p.items()}
                        rows, loss = _feed(tr, row, ref, rank)
                        torch.cuda.synchronize()
                        if not row.bitwise:
                            fails.extend(check_rank_step(tr, ref, rows, was, loss, f"{row.name} rank {rank} graph step {s}", graph_ratios))
                        elif not (torch.equal(loss, losses[s]) and same(rank_snapshot(tr), states[s])):
                            fails.append(f"{row.name} rank {rank} step {s}: the graph step is not bitwise the eager one")
                unit(f"graph step {s}", graph_step)
            if graph_ratios:
                rec["graph_ratios"] = graph_ratios
            rec["done"].append("graph")

            # ---- 4. the three slots once more: singly on both, as one group on the third
            def slots_again():
                want = [eager.step(slot=s).clone() for s in (0, 1, 2)]
                got_single = [single.step(slot=s).clone() for s in (0, 1, 2)]
                if row.name == "fx_next_forward":
                    # gloo cannot be captured: the group's launches issued eagerly, so that the update that also forms the next
                    # forward runs with more than one rank (tests/test_gpu_dp.py::_big_worker)
                    timers = {k: [] for k in FUSED_GROUP}
                    got_group = group.step_many((0, 1, 2), timers=timers).clone()
                    if [len(timers[k]) for k in FUSED_GROUP] != [2, 1]:
                        fails.append(f"{row.name}: {[len(timers[k]) for k in FUSED_GROUP]} fused / plain table updates in a group of three")
                else:
                    got_group = group.step_many((0, 1, 2)).clone()
                torch.cuda.synchronize()
                if row.backend == "nccl" and group.factor_exchange and ((0, 1, 2), "many") not in group._g_local:
                    fails.append(f"{row.name}: the step group was not captured as one graph")
                if not (eager.steps_done == single.steps_done == group.steps_done == 6):
                    fails.append(f"{row.name}: steps done {eager.steps_done}, {single.steps_done}, {group.steps_done}")
                if row.bitwise:
                    if not (torch.equal(torch.stack(got_single), torch.stack(want)) and same(rank_snapshot(single), rank_snapshot(eager))):
                        fails.append(f"{row.name} rank {rank}: single graph steps on the slots are not bitwise the eager ones")
                    if not (torch.equal(got_group, torch.stack(got_single)) and same(rank_snapshot(group), rank_snapshot(single))):
                        fails.append(f"{row.name} rank {rank}: the step group is not bitwise the single graph steps")
                else:
                    for tr, got in ((single, torch.stack(got_single)), (group, got_group)):  # conftest.assert_close_grad's bar
                        worst = max([_ratio_grad(got, torch.stack(want))]
                                    + [_ratio_grad(a.float(), b.float()) for a, b in zip(rank_snapshot(tr), rank_snapshot(eager))])
                        graph_ratios["slots"] = max(graph_ratios.get("slots", 0.0), worst)
                        if not worst <= 1.0:
                            fails.append(f"{row.name} rank {rank}: losses or state after the slots at {worst:.3g} x the gradient bar")
            unit("the slots again", slots_again)
            rec["done"].append("slots")
        except _Abandoned as where:
            fails.append(f"{row.name} rank {rank}: abandoned by every rank after '{where}'")
        finally:
            torch.cuda.synchronize()
    rec["seconds"] = round(time.time() - t0, 3)
    return rec


# ------------------------------------------------------------------------------------------------ one group in one spawn
def _group_worker(rank: int, port: int, out_dir: str, world: int, backend: str, names: List[str], oracle_files: Dict[str, str]):
    """Process-group set-up as tests/test_gpu_dp.py::_worker."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = rank if backend == "nccl" and torch.cuda.device_count() >= world else 0
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        loaded: Dict[str, List[Dict]] = {}
        for name in names:
            path = oracle_files[name]
            if path not in loaded:
                loaded = {path: torch.load(path, weights_only=True)}  # (one at a time: the 8192-row table's is the big one)
            rec = run_row(BY_NAME[name], rank, loaded[path])
            torch.save(rec, Path(out_dir) / f"{name}_{rank}.pt")
            brief = {k: v for k, v in rec.items() if k != "steps"}
            (Path(out_dir) / f"{name}_{rank}.json").write_text(json.dumps(brief, sort_keys=True, indent=1))
    finally:
        dist.destroy_process_group()


def run_group(group: Tuple[int, str], base_dir: Path, oracles: Dict[str, List[Dict]]) -> Dict:
    """Spawns the group's ranks once; its files go under `base_dir`.  oracles: a cache {oracle_key: steps} shared between the
    groups of one run (each is computed once, in float64 on the CPU, and saved before the spawn).  Returns {"died": why or None, "records": {row name:
    [record per rank, None where a rank left none]}, "seconds"}.  A spawn that dies is not retried."""
    import torch.multiprocessing as mp
    world, backend = group
    rows = rows_of(group)
    out_dir = Path(base_dir) / f"{backend}{world}"
    out_dir.mkdir(parents=True, exist_ok=True)
    files = {}
    for row in rows:
        key = oracle_key(row)
        path = Path(base_dir) / f"oracle_{key}.pt"
        if key not in oracles:
            oracles[key] = oracle_of(row)
        if not path.exists():
            torch.save(oracles[key], path)
        files[row.name] = str(path)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    died, t0 = None, time.time()
    try:
        mp.spawn(_group_worker, args=(port, str(out_dir), world, backend, [r.name for r in rows], files), nprocs=world, join=True)
    except Exception as exc:  # noqa: BLE001  (ProcessExitedException / ProcessRaisedException: the child's exit status or traceback)
        died = f"{type(exc).__name__}: {exc}"
    records = {}
    for row in rows:
        paths = [out_dir / f"{row.name}_{r}.pt" for r in range(world)]
        records[row.name] = [torch.load(p, weights_only=True) if p.exists() else None for p in paths]
    return dict(died=died, records=records, seconds=round(time.time() - t0, 2))


# ------------------------------------------------------------------------------------------------ the parent's checks
def _same_state(a: Dict, b: Dict) -> bool:
    return a.keys() == b.keys() and all(a[kind].keys() == b[kind].keys() and same(list(a[kind].values()), list(b[kind].values()))
                                        for kind in a)


def check_row(row: DpRow, records: List[Dict], refs: List[Dict]) -> Tuple[List[str], List[Dict[str, float]]]:
    """What only the parent can see, over the records of all ranks: every rank's own failures, the mean of the rank-local losses
    against the oracle's global loss (the loss bar), every rank's checkpointed optimizer state against the oracle's (the
    momentum / moment bars), and bitwise equal replicas after every step.  Returns (failures, worst ratio per bar per rank)."""
    cfg, world = row.config, row.world
    g = geometry(cfg)
    fails = [f for rec in records for f in rec["fails"]]
    ratios = [dict(rec["ratios"]) for rec in records]
    for rec in records:
        if rec["done"] != ["mode", "eager", "graph", "slots"]:
            fails.append(f"{row.name} rank {rec['rank']}: finished only {rec['done']}")
    if any(len(rec["steps"]) != len(refs) for rec in records):
        return fails + [f"{row.name}: {[len(rec['steps']) for rec in records]} recorded steps per rank"], ratios
    adam = cfg["optimizer"] == "adam"
    for ref in refs:
        s = ref["step"]
        steps = [rec["steps"][s] for rec in records]
        mean = sum(st["loss"] for st in steps) / world
        for r, st in enumerate(steps):
            held = dict(optimizer=cfg["optimizer"], sink=g["F"] - 1 if g["P"] > g["F"] else None, loss=mean)
            if adam:
                held.update(exp_avg=st["state"].get("exp_avg", {}), exp_avg_sq=st["state"].get("exp_avg_sq", {}))
                if not (st["state"].get("step") and all(float(v) == s + 1 for v in st["state"]["step"].values())):
                    fails.append(f"{row.name} rank {r} step {s}: the checkpointed Adam step count is not {s + 1}")
            else:
                held["momentum"] = st["state"].get("momentum_buffer", {})
            want = set(ref["state"]) if (adam or cfg["momentum"]) else set()
            for kind in ("exp_avg", "exp_avg_sq") if adam else ("momentum",):
                if set(held[kind]) != want:
                    fails.append(f"{row.name} rank {r} step {s}: the checkpoint holds {kind} of {sorted(held[kind])}")
            fails += compare_held(held, ref, cfg["batch"], 0, 1.0, f"{row.name} rank {r} step {s} (checkpoint)", ratios[r])
            if r and not (torch.equal(st["params"], steps[0]["params"]) and st["norm"] == steps[0]["norm"]
                          and same(st["buffers"], steps[0]["buffers"]) and _same_state(st["state"], steps[0]["state"])):
                fails.append(f"{row.name} step {s}: rank {r} is not bitwise rank 0 (parameters, norm or optimizer state)")
    return fails, ratios
