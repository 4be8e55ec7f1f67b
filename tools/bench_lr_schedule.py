"""What a per-step learning-rate schedule costs (NnueTrainer.set_lr_schedule; include/nnue_hip.h: nnue_lr_schedule_step), at
bench.py's C2 (batch 512, 800 -> 1024/128/32 -> 10) and at the 224x224 shape (C4, batch 128), SGD(0.9) with clip 1.0, single
rank, 8 input slots, groups of 8 steps.  Three forms, three trainers in ONE process, alternated block by block:
  a  groups, no schedule        step_many(0..7): the launches of the commit before the schedule existed -- the baseline;
  b  groups, device schedule    the same group with one nnue_lr_schedule_step per step inside the graph;
  c  single steps, host fill    what a per-step schedule cost before: ``trainer.lr = v`` and step(slot) for every step.
Every sample is a block of --block groups between two device events (so the host's gaps in form c count, as they do in a
run); at least --groups groups per form after a warm-up of every graph; medians with the 10th and 90th percentiles, and the
ratios b/a and b/c of the medians.  No threshold is built in.

  python tools/bench_lr_schedule.py > profiles/lr_schedule.json

GPU only; fails without one; reads nothing outside the repository."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))
sys.path.insert(0, str(ROOT))

SHAPES = {  # bench.py's WORKLOADS c2 and c4; block: groups per event-timed sample
    "c2": dict(grid=10, fps=8, image=32, l1=1024, l2=128, l3=32, classes=10, batch=512, block=10),
    "c4": dict(grid=32, fps=64, image=224, l1=1024, l2=128, l3=32, classes=1000, batch=128, block=2),
}
OPT = dict(lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0)
SLOTS = 8
GROUP = tuple(range(SLOTS))


def percentile(values, q):
    v = sorted(values)
    k = (len(v) - 1) * q
    lo, hi = int(k), min(int(k) + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (k - lo)


def measure(name: str, groups: int) -> dict:
    import torch
    import nnue
    from nnue_hip.lr_schedule import LrSchedule
    from nnue_hip.trainer import NnueTrainer
    c = SHAPES[name]
    dev = torch.device("cuda", 0)
    values = LrSchedule(learning_rate=OPT["lr"], lr_decay_iters=1 << 20).values(1 << 14)  # cosine, far from its end: rates stay useful
    host_values = [float(v) for v in values]
    trainers = {}
    for form in "abc":
        torch.manual_seed(0)
        model = nnue.NNUE(nnue.GridFeatureSet(c["grid"], c["fps"]), c["l1"], c["l2"], c["l3"], num_classes=c["classes"],
                          input_size=c["image"]).to(dev)
        tr = NnueTrainer(model, c["batch"], (c["image"], c["image"]), use_graph=True, input_slots=SLOTS, **OPT)
        gen = torch.Generator().manual_seed(1234)
        for images, labels in tr.inputs:
            images.copy_(torch.randn(c["batch"], 3, c["image"], c["image"], generator=gen))
            labels.copy_(torch.randint(0, c["classes"], (c["batch"],), generator=gen))
        if form == "b":
            tr.set_lr_schedule(values)
        trainers[form] = tr

    def run_group(form):
        tr = trainers[form]
        if form != "c":
            tr.step_many(GROUP)
            return
        for s in GROUP:
            tr.lr = host_values[tr.steps_done % len(host_values)]
            tr.step(slot=s)

    for form in "abc":  # plans, every single-step graph, the group's graph
        for s in GROUP:
            trainers[form].step(slot=s)
        for s in GROUP:
            trainers[form].step(slot=s)
        for _ in range(3):
            run_group(form)
    torch.cuda.synchronize()
    block = c["block"]
    samples = {form: [] for form in "abc"}
    events = []
    for _ in range((groups + block - 1) // block):
        for form in "abc":  # alternated: one block of every form per round
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(block):
                run_group(form)
            t1.record()
            events.append((form, t0, t1))
    torch.cuda.synchronize()
    for form, t0, t1 in events:
        samples[form].append(t0.elapsed_time(t1) / (block * SLOTS))  # ms per step
    out = {"shape": {k: v for k, v in c.items() if k != "block"}, "groups_per_form": len(samples["a"]) * block, "groups_per_sample": block,
           "steps_per_group": SLOTS, "forms": {}}
    labels = {"a": "groups, no schedule (baseline)", "b": "groups, device schedule", "c": "single steps, host fill before each"}
    for form in "abc":
        v = samples[form]
        out["forms"][form] = {"what": labels[form], "median_ms_per_step": round(statistics.median(v), 5),
                              "p10_ms_per_step": round(percentile(v, 0.1), 5), "p90_ms_per_step": round(percentile(v, 0.9), 5),
                              "samples": len(v)}
    med = {form: statistics.median(samples[form]) for form in "abc"}
    out["b_over_a"] = round(med["b"] / med["a"], 4)
    out["b_over_c"] = round(med["b"] / med["c"], 4)
    out["b_minus_a_us_per_step"] = round((med["b"] - med["a"]) * 1e3, 3)
    tr = trainers["b"]
    out["checks"] = {"schedule_position": int(tr.lr_pos), "steps_done": tr.steps_done,
                     "schedule_calls_in_update_plan": [n for n, _, _ in tr._plan_update].count("nnue_lr_schedule_step"),
                     "baseline_update_plan_has_schedule_call": "nnue_lr_schedule_step" in [n for n, _, _ in trainers["a"]._plan_update]}
    del trainers
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c4", help="comma-separated subset of: " + ", ".join(SHAPES))
    ap.add_argument("--groups", type=int, default=200, help="groups per form after warm-up (at least 200)")
    args = ap.parse_args()
    shapes = [s for s in args.shapes.split(",") if s]
    if any(s not in SHAPES for s in shapes) or args.groups < 200:
        raise SystemExit("shapes must be among " + ", ".join(SHAPES) + "; --groups >= 200")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lr_schedule.py measures on the GPU and needs one")
    res = {"optimizer": dict(OPT, kind="sgd"), "timing": "device events around blocks of groups, forms alternated in one process",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for s in shapes:
        res["shapes"][s] = measure(s, args.groups)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
