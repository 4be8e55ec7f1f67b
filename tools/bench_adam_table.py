"""Adam at the big-table shape (C4: GridFeatureSet(32, 64), 1024/128/32, 1000 classes, 224x224, batch 128): what the table
update in the weight-gradient product's epilogue and the fused update + next forward buy the reference's other optimizer
(train.py:465-471).  bench.py is SGD-only; this is its side tool for Adam.

NnueTrainer(optimizer="adam", lr=1e-3, weight_decay=2e-4, max_grad_norm=1.0), synthetic inputs as bench.py draws them,
step groups (NnueTrainer.step_many) replayed as one graph.  Three modes, each in a child process of its own because the
knobs are read at construction:
  materialised      NNUE_FUSE_TABLE_UPDATE=0: d_W written, read by the norm, nnue_adam_step over the whole flat buffer (the
                    baseline: the only Adam path before the fused update existed);
  fused_update      NNUE_FUSE_TABLE_UPDATE=1, NNUE_FUSE_NEXT_FORWARD=0: Gram norm, nnue_adam_step_ext on the small tensors,
                    nnue_ftm_backward_weight_update_adam; the next forward reads the table again;
  fused_update_fwd  both on: inside a group nnue_ftm_backward_weight_update_forward_adam also forms the next forward.
The three children stay alive and the parent ALTERNATES timed windows between them (--runs rounds, default 5): every window
is preceded by a warm-up of two groups, lasts at least --window seconds (default 0.25) and is device-synchronised wall
time.  Then each child issues its group eagerly with events around the named launches (step_many(timers=...)) and reports
their median duration; bytes per launch are computed here from the shapes, share = bytes / time / 8 TB/s.

  python tools/bench_adam_table.py > profiles/adam_table_update.json
  python tools/bench_adam_table.py --modes materialised          (one mode only, e.g. on the parent commit)
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_adam_table.py --child fused_update_fwd --profile-steps 3

GPU only; fails without one; reads nothing outside the repository."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))
sys.path.insert(0, str(ROOT))

MODES = {
    "materialised": {"NNUE_FUSE_TABLE_UPDATE": "0"},
    "fused_update": {"NNUE_FUSE_TABLE_UPDATE": "1", "NNUE_FUSE_NEXT_FORWARD": "0"},
    "fused_update_fwd": {"NNUE_FUSE_TABLE_UPDATE": "1", "NNUE_FUSE_NEXT_FORWARD": "1"},
}
SHAPE = dict(grid=32, fps=64, image=224, l1=1024, l2=128, l3=32, classes=1000, batch=128)
ADAM = dict(lr=1e-3, weight_decay=2e-4, max_grad_norm=1.0)
SLOTS, GROUP = 4, 20  # 20 steps per graph on slots 0 1 2 3 0 ...: every replay is the same group
HBM_PEAK_GBS = 8000.0
TIMED = ("nnue_adam_step", "nnue_adam_step_ext", "nnue_ftm_backward_weight_update_adam", "nnue_ftm_backward_weight_update_forward_adam",
         "nnue_ftm_forward", "nnue_ftm_gram_sqnorm_tail", "nnue_ftm_backward")


def launch_bytes():
    """Compulsory bytes of the new launches, from the shapes: table rows the product covers, three streams read and written,
    + the map(s) and d_out (the next forward's output and slabs are launch-sized and left out)."""
    b, l1 = SHAPE["batch"], SHAPE["l1"]
    f = SHAPE["grid"] ** 2 * SHAPE["fps"]
    p = f  # one position per feature at this shape
    rows = min(f - 1, p)
    table = rows * l1 * 4
    return {"table_rows_bytes": table,
            "nnue_ftm_backward_weight_update_adam": 6 * table + b * p + b * l1 * 4,
            "nnue_ftm_backward_weight_update_forward_adam": 6 * table + 2 * b * p + b * l1 * 4}


def child(mode: str, profile_steps: int) -> None:
    import torch
    import nnue
    from nnue_hip.trainer import NnueTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam_table.py measures on the GPU and needs one")
    dev = torch.device("cuda", 0)
    c = SHAPE
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(c["grid"], c["fps"]), c["l1"], c["l2"], c["l3"], num_classes=c["classes"],
                      input_size=c["image"]).to(dev)
    tr = NnueTrainer(model, c["batch"], (c["image"], c["image"]), use_graph=True, input_slots=SLOTS, optimizer="adam", **ADAM)
    gen = torch.Generator().manual_seed(1234)
    for images, labels in tr.inputs:
        images.copy_(torch.randn(c["batch"], 3, c["image"], c["image"], generator=gen))
        labels.copy_(torch.randint(0, c["classes"], (c["batch"],), generator=gen))
    group = tuple(j % SLOTS for j in range(GROUP))
    for i in range(SLOTS + 1):  # plans, single-step graphs
        tr.step(slot=i % SLOTS)
    tr.step_many(group)  # captures the group's graph
    torch.cuda.synchronize()
    flags = {"fuse_table_update": bool(tr.fuse_table_update), "fuse_next_forward": bool(tr.fuse_next_forward),
             "grads_materialised": bool(tr.grads_materialised)}
    if profile_steps:  # under a profiler: a few replays, nothing else
        for _ in range(profile_steps):
            tr.step_many(group)
        torch.cuda.synchronize()
        print(json.dumps({"mode": mode, **flags, "profiled_groups": profile_steps, "steps_per_group": GROUP}), flush=True)
        return
    print(json.dumps({"ready": mode, **flags}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "time":
            window = float(cmd[1])
            for _ in range(2):  # warm-up before every timed window
                tr.step_many(group)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step_many(group)
            torch.cuda.synchronize()
            groups = max(1, math.ceil(window / max(time.perf_counter() - t0, 1e-4)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(groups):
                loss = tr.step_many(group)[-1]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"ms_per_step": dt * 1e3 / (groups * GROUP), "window_s": dt, "steps": groups * GROUP,
                              "loss": float(loss)}), flush=True)
        elif cmd[0] == "events":
            per = {}
            for _ in range(int(cmd[1])):
                timers = {k: [] for k in TIMED}
                tr.step_many(group, timers=timers)
                torch.cuda.synchronize()
                for k, evs in timers.items():
                    per.setdefault(k, []).extend(a.elapsed_time(b) * 1e3 for a, b in evs)
            print(json.dumps({k: {"launches": len(v), "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
                              for k, v in per.items() if v}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=sorted(MODES))
    ap.add_argument("--profile-steps", type=int, default=0, help="with --child: replay this many groups and exit (for rocprofv3)")
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of: " + ", ".join(MODES))
    ap.add_argument("--runs", type=int, default=5, help="timed windows per mode, alternated between the modes (at least 5)")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window (at least 0.2)")
    ap.add_argument("--event-groups", type=int, default=3, help="eagerly issued groups for the per-launch event times")
    args = ap.parse_args()
    if args.child:
        for k in ("NNUE_FUSE_TABLE_UPDATE", "NNUE_FUSE_NEXT_FORWARD"):
            os.environ.pop(k, None)
        os.environ.update(MODES[args.child])
        child(args.child, args.profile_steps)
        return
    modes = [m for m in args.modes.split(",") if m]
    if any(m not in MODES for m in modes) or args.runs < 5 or args.window < 0.2:
        raise SystemExit("modes must be among " + ", ".join(MODES) + "; --runs >= 5; --window >= 0.2")
    procs = {}
    try:
        for m in modes:  # one fresh process per mode; they stay alive so that the windows can alternate
            procs[m] = subprocess.Popen([sys.executable, __file__, "--child", m], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

        def ask(m, cmd=None):
            p = procs[m]
            if cmd is not None:
                p.stdin.write(cmd + "\n")
                p.stdin.flush()
            line = p.stdout.readline()
            if not line:
                raise SystemExit(f"mode {m}: the child process ended (exit status {p.wait()})")
            return json.loads(line)

        res = {"shape": SHAPE, "optimizer": dict(ADAM, kind="adam"), "steps_per_group": GROUP, "hbm_peak_gbs": HBM_PEAK_GBS,
               "window_s_min": args.window, "modes": {}}
        for m in modes:
            res["modes"][m] = {"env": MODES[m], "flags": ask(m), "runs_ms_per_step": [], "windows_s": []}
        for _ in range(args.runs):  # alternated: one window of every mode per round
            for m in modes:
                r = ask(m, f"time {args.window}")
                res["modes"][m]["runs_ms_per_step"].append(round(r["ms_per_step"], 5))
                res["modes"][m]["windows_s"].append(round(r["window_s"], 4))
                res["modes"][m]["last_loss"] = r["loss"]
        nbytes = launch_bytes()
        res["launch_bytes"] = nbytes
        for m in modes:
            d = res["modes"][m]
            runs = d["runs_ms_per_step"]
            d["median_ms_per_step"] = round(statistics.median(runs), 5)
            d["range_ms_per_step"] = [min(runs), max(runs)]
            ev = ask(m, f"events {args.event_groups}")
            for k, v in ev.items():
                if k in nbytes:
                    v["bytes"] = nbytes[k]
                    v["hbm_peak_share"] = round(nbytes[k] / (v["median_us"] * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
            d["launches_event_timed"] = ev
        rng = lambda m: res["modes"][m]["range_ms_per_step"]  # noqa: E731
        if "materialised" in modes and "fused_update" in modes:
            res["fused_update_range_wholly_below_materialised"] = rng("fused_update")[1] < rng("materialised")[0]
        if "fused_update" in modes and "fused_update_fwd" in modes:
            res["fused_update_fwd_range_wholly_below_fused_update"] = rng("fused_update_fwd")[1] < rng("fused_update")[0]
        print(json.dumps(res, indent=1))
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:  # noqa: BLE001 -- a child that already ended
                p.kill()


if __name__ == "__main__":
    main()
