"""What the weight clip costs in the step (NnueTrainer weight_clip; include/nnue_hip.h "weight clip"), at bench.py's C2 (batch
512, 800 -> 1024/128/32 -> 10; SGD) and at the 224x224 shape (C4, batch 128; SGD and Adam), momentum 0.9 / clip norm 1.0, single
rank, 8 input slots, groups of 8 steps.  Two trainers in ONE process, alternated block by block:
  plain  step_many(0..7) of a trainer with weight_clip = 0: today's launches -- the baseline;
  clip   the same group with weight_clip = 1.0: the same launches with the clamp inside the update's stores.
Every sample is a block of --block groups between two device events; at least --groups groups per form after a warm-up of every
graph; medians with the 10th and 90th percentiles, the ratio clip / plain of the medians, and whether the clipped median lies
inside the plain form's own 10th-90th percentile band (the expectation: two compares per element inside stores the step already
makes).  No threshold is built in.

Also what the clip replaces: single steps of the plain trainer at the 224x224 shape with ``model._clip_weights()`` (nnue.py:528-539)
after each -- a separate pass that reads and writes the 268 MB table -- against the same single steps alone.  The plain trainer
launches exactly what the trainer launched before the option existed.

  python tools/bench_weight_clip.py > profiles/weight_clip.json
  python tools/bench_weight_clip.py --lr 0 > profiles/weight_clip_lr0.json     (the control: see --lr)

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
CASES = (("c2", "sgd"), ("c4", "sgd"), ("c4", "adam"))
OPT = {"sgd": dict(lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0),
       "adam": dict(optimizer="adam", lr=1e-3, weight_decay=2e-4, max_grad_norm=1.0)}
CLIP = 1.0
SLOTS = 8
GROUP = tuple(range(SLOTS))
FORMS = ("plain", "clip")


def percentile(values, q):
    v = sorted(values)
    k = (len(v) - 1) * q
    lo, hi = int(k), min(int(k) + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (k - lo)


def summary(v):
    return {"median_ms_per_step": round(statistics.median(v), 5), "p10_ms_per_step": round(percentile(v, 0.1), 5),
            "p90_ms_per_step": round(percentile(v, 0.9), 5), "samples": len(v)}


def build(c, opt, weight_clip, lr=None):
    import torch
    import nnue
    from nnue_hip.trainer import NnueTrainer
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(c["grid"], c["fps"]), c["l1"], c["l2"], c["l3"], num_classes=c["classes"],
                      input_size=c["image"]).to("cuda")
    tr = NnueTrainer(model, c["batch"], (c["image"], c["image"]), use_graph=True, input_slots=SLOTS, weight_clip=weight_clip,
                     **(OPT[opt] if lr is None else dict(OPT[opt], lr=lr)))
    gen = torch.Generator().manual_seed(1234)
    for images, labels in tr.inputs:
        images.copy_(torch.randn(c["batch"], 3, c["image"], c["image"], generator=gen))
        labels.copy_(torch.randint(0, c["classes"], (c["batch"],), generator=gen))
    return model, tr


def timed_blocks(rounds, forms, run):
    """{form: [ms per block]}: one block of every form per round, between two device events."""
    import torch
    events = []
    for _ in range(rounds):
        for form in forms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run(form)
            t1.record()
            events.append((form, t0, t1))
    torch.cuda.synchronize()
    out = {form: [] for form in forms}
    for form, t0, t1 in events:
        out[form].append(t0.elapsed_time(t1))
    return out


def measure(name: str, opt: str, groups: int, lr) -> dict:
    import torch
    c = SHAPES[name]
    trainers = {"plain": build(c, opt, 0.0, lr)[1], "clip": build(c, opt, CLIP, lr)[1]}
    for form in FORMS:  # plans, every single-step graph, the group's graph
        for _ in range(2):
            for s in GROUP:
                trainers[form].step(slot=s)
        for _ in range(3):
            trainers[form].step_many(GROUP)
    torch.cuda.synchronize()
    block = c["block"]

    def run(form):
        for _ in range(block):
            trainers[form].step_many(GROUP)
    blocks = timed_blocks((groups + block - 1) // block, FORMS, run)
    samples = {f: [ms / (block * SLOTS) for ms in blocks[f]] for f in FORMS}
    out = {"shape": {k: v for k, v in c.items() if k != "block"}, "optimizer": dict(OPT[opt], kind=opt, **({} if lr is None else {"lr": lr})), "groups_per_form": len(samples["plain"]) * block,
           "groups_per_sample": block, "steps_per_group": SLOTS, "forms": {f: summary(samples[f]) for f in FORMS}}
    plain, clip = out["forms"]["plain"], out["forms"]["clip"]
    out["clip_over_plain"] = round(clip["median_ms_per_step"] / plain["median_ms_per_step"], 4)
    out["clip_minus_plain_us_per_step"] = round((clip["median_ms_per_step"] - plain["median_ms_per_step"]) * 1e3, 3)
    out["clip_median_inside_plain_band"] = plain["p10_ms_per_step"] <= clip["median_ms_per_step"] <= plain["p90_ms_per_step"]

    # which launch accounts for a difference: the update's entry points, event-timed one by one in eager groups (a clamping
    # sibling is timed under the plain entry point's name), forms alternated group by group
    names = ["nnue_adam_step_ext", "nnue_adam_step", "nnue_ftm_backward_weight_update_adam", "nnue_ftm_backward_weight_update_forward_adam"] \
        if opt == "adam" else ["nnue_sgd_step", "nnue_ftm_backward_weight_update", "nnue_ftm_backward_weight_update_forward"]
    timers = {f: {n: [] for n in names} for f in FORMS}
    for _ in range(12):
        for f in FORMS:
            trainers[f].step_many(GROUP, timers=timers[f])
    torch.cuda.synchronize()
    out["update_launches_us"] = {}
    for n in names:
        us = {f: [t0.elapsed_time(t1) * 1e3 for t0, t1 in timers[f][n]] for f in FORMS}
        if us["plain"]:
            out["update_launches_us"][n] = {f: {"median": round(statistics.median(us[f]), 2), "p10": round(percentile(us[f], 0.1), 2),
                                                "p90": round(percentile(us[f], 0.9), 2), "launches": len(us[f])} for f in FORMS}

    diffs = {n: round(v["clip"]["median"] - v["plain"]["median"], 2) for n, v in out["update_launches_us"].items()}
    worst = max(diffs, key=diffs.get)
    out["largest_launch_difference"] = {"entry_point": worst, "clip_minus_plain_us": diffs[worst], "all": diffs}

    def update_calls(t):
        return [n for n, _, _ in (t._plan_update or [])]
    out["checks"] = {"plain_update_calls": update_calls(trainers["plain"]), "clip_update_calls": update_calls(trainers["clip"]),
                     "mode": trainers["clip"].mode.describe(), "same_mode": trainers["clip"].mode == trainers["plain"].mode,
                     "steps_done": {f: trainers[f].steps_done for f in FORMS},
                     # the kernels' time depends on the active-feature density: where the forms' parameters have drifted apart (the
                     # clamp has bitten) they no longer run on the same map
                     "same_parameters_at_the_end": bool(torch.equal(trainers["plain"].flat_params, trainers["clip"].flat_params)),
                     "mean_active_features": {f: round(trainers[f].active_stats()[0], 1) for f in FORMS}}
    del trainers
    torch.cuda.empty_cache()
    return out


def bolt_on(steps: int) -> dict:
    """Single steps of the plain trainer at the 224x224 shape (SGD), alone and with model._clip_weights() after each."""
    import torch
    c = SHAPES["c4"]
    model, tr = build(c, "sgd", 0.0)
    for _ in range(2):
        for s in GROUP:
            tr.step(slot=s)
    model._clip_weights()
    torch.cuda.synchronize()

    def run(form):
        for s in GROUP:
            tr.step(slot=s)
            if form == "steps_then_clip_weights":
                model._clip_weights()
    forms = ("steps", "steps_then_clip_weights")
    blocks = timed_blocks((steps + SLOTS - 1) // SLOTS, forms, run)
    out = {"what": "single graph steps of the plain trainer (SGD, 224x224), alone and with model._clip_weights() after every step",
           "table_bytes": int(model.input.weight.numel()) * 4,
           "forms": {f: summary([ms / SLOTS for ms in blocks[f]]) for f in forms}}
    a, b = out["forms"]["steps"]["median_ms_per_step"], out["forms"]["steps_then_clip_weights"]["median_ms_per_step"]
    out["clip_weights_us_per_step"] = round((b - a) * 1e3, 3)
    out["with_over_without"] = round(b / a, 4)
    del model, tr
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=200, help="groups per form after warm-up (at least 200)")
    ap.add_argument("--lr", type=float, default=None,
                    help="learning rate of every trainer (default: 0.01 for SGD, 1e-3 for Adam).  0 is the control: the parameters stay put, "
                         "so both forms run on the same map throughout -- the clamp executes all the same, it just changes nothing")
    ap.add_argument("--bolt-on-steps", type=int, default=400, help="single steps per form of the bolt-on comparison")
    args = ap.parse_args()
    if args.groups < 200:
        raise SystemExit("--groups >= 200")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_clip.py measures on the GPU and needs one")
    res = {"weight_clip": CLIP, "timing": "device events around blocks of groups, forms alternated in one process",
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, opt in CASES:
        res["cases"][f"{name}_{opt}"] = measure(name, opt, args.groups, args.lr)
    res["bolt_on_clip_weights_c4"] = bolt_on(args.bolt_on_steps)
    outside = [k for k, v in res["cases"].items() if not v["clip_median_inside_plain_band"]]
    res["cases_with_clip_median_outside_plain_band"] = outside
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
