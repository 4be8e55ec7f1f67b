"""What the weight average costs in the step (NnueTrainer ema_decay / ema_warmup; include/nnue_hip.h "weight average"), at
bench.py's C2 (batch 512, 800 -> 1024/128/32 -> 10; SGD) and at the 224x224 shape (C4, batch 128; SGD and Adam), momentum 0.9 /
clip norm 1.0, single rank, 8 input slots, groups of 8 steps.  Five trainers in ONE process, alternated block by block (each
single-step form has a plain trainer of its own, so every trainer takes the same number of steps and the forms run at the same
stage of training):
  plain        step_many(0..7) of a trainer with ema_decay = 0: today's launches -- the baseline of the groups;
  ema          the same group with ema_decay = 0.999: the update launches also read and write the average;
  ema_warmup   ... and ema_warmup: one more small launch per step, the warm-up's rate out of its table;
  steps        single graph steps of the plain trainer -- the baseline of what the feature replaces;
  steps_lerp   the same single steps, each followed by ``flat_ema.lerp_(flat_params, omd)`` on a buffer of the caller's.
Every sample is a block of --block groups (or as many single steps) between two device events; at least --groups groups per form
after a warm-up of every graph; medians with the 10th and 90th percentiles and the ratios ema / plain, ema_warmup / plain,
steps_lerp / steps, and (ema - plain) against (steps_lerp - steps): what the average costs inside the launches against what it
costs as a separate pass, each over its own baseline.  No threshold is built in.

  python tools/bench_ema.py > profiles/ema.json
  python tools/bench_ema.py --lr 0 > profiles/ema_lr0.json     (the control: see --lr)

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
DECAY = 0.999
SLOTS = 8
GROUP = tuple(range(SLOTS))
TRAINERS = {"plain": dict(), "ema": dict(ema_decay=DECAY), "ema_warmup": dict(ema_decay=DECAY, ema_warmup=True)}
FORMS = ("plain", "ema", "ema_warmup", "steps", "steps_lerp")


def percentile(values, q):
    v = sorted(values)
    k = (len(v) - 1) * q
    lo, hi = int(k), min(int(k) + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (k - lo)


def summary(v):
    return {"median_ms_per_step": round(statistics.median(v), 5), "p10_ms_per_step": round(percentile(v, 0.1), 5),
            "p90_ms_per_step": round(percentile(v, 0.9), 5), "samples": len(v)}


def build(c, opt, lr=None, **kw):
    import torch
    import nnue
    from nnue_hip.trainer import NnueTrainer
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(c["grid"], c["fps"]), c["l1"], c["l2"], c["l3"], num_classes=c["classes"],
                      input_size=c["image"]).to("cuda")
    tr = NnueTrainer(model, c["batch"], (c["image"], c["image"]), use_graph=True, input_slots=SLOTS,
                     **(OPT[opt] if lr is None else dict(OPT[opt], lr=lr)), **kw)
    gen = torch.Generator().manual_seed(1234)
    for images, labels in tr.inputs:
        images.copy_(torch.randn(c["batch"], 3, c["image"], c["image"], generator=gen))
        labels.copy_(torch.randint(0, c["classes"], (c["batch"],), generator=gen))
    return tr


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
    from nnue_hip import lib
    c = SHAPES[name]
    trainers = {k: build(c, opt, lr, **kw) for k, kw in TRAINERS.items()}
    single, single_lerp = build(c, opt, lr), build(c, opt, lr)  # the plain trainers of the two single-step forms
    for tr in list(trainers.values()) + [single, single_lerp]:  # plans, every single-step graph, the group's graph
        for _ in range(2):
            for s in GROUP:
                tr.step(slot=s)
        for _ in range(3):
            tr.step_many(GROUP)
    plain = trainers["plain"]
    bolt_on, omd = single_lerp.flat_params.clone(), lib.ema_omd(DECAY)  # the caller's own average of that trainer
    bolt_on.lerp_(single_lerp.flat_params, omd)
    torch.cuda.synchronize()
    block = c["block"]

    def run(form):
        for _ in range(block):
            if form in trainers:
                trainers[form].step_many(GROUP)
                continue
            if form == "steps_lerp":
                for s in GROUP:
                    single_lerp.step(slot=s)
                    bolt_on.lerp_(single_lerp.flat_params, omd)
            else:
                for s in GROUP:
                    single.step(slot=s)
    blocks = timed_blocks((groups + block - 1) // block, FORMS, run)
    samples = {f: [ms / (block * SLOTS) for ms in blocks[f]] for f in FORMS}
    out = {"shape": {k: v for k, v in c.items() if k != "block"}, "optimizer": dict(OPT[opt], kind=opt, **({} if lr is None else {"lr": lr})), "ema_decay": DECAY,
           "groups_per_form": len(samples["plain"]) * block, "groups_per_sample": block, "steps_per_group": SLOTS,
           "flat_buffer_bytes": int(plain.flat_params.numel()) * 4, "forms": {f: summary(samples[f]) for f in FORMS}}
    med = {f: out["forms"][f]["median_ms_per_step"] for f in FORMS}
    out["ema_over_plain"] = round(med["ema"] / med["plain"], 4)
    out["ema_warmup_over_plain"] = round(med["ema_warmup"] / med["plain"], 4)
    out["steps_lerp_over_steps"] = round(med["steps_lerp"] / med["steps"], 4)
    out["ema_minus_plain_us_per_step"] = round((med["ema"] - med["plain"]) * 1e3, 3)
    out["ema_warmup_minus_plain_us_per_step"] = round((med["ema_warmup"] - med["plain"]) * 1e3, 3)
    out["lerp_us_per_step"] = round((med["steps_lerp"] - med["steps"]) * 1e3, 3)
    out["ema_groups_over_steps_lerp"] = round(med["ema"] / med["steps_lerp"], 4)
    p = out["forms"]["plain"]
    out["ema_median_inside_plain_band"] = p["p10_ms_per_step"] <= med["ema"] <= p["p90_ms_per_step"]

    # which launch accounts for the difference: the update's entry points, event-timed one by one in eager groups (an averaging
    # sibling is timed under the plain entry point's name; the stand-alone pass under its own), forms alternated group by group
    names = ["nnue_adam_step_ext", "nnue_adam_step", "nnue_ftm_backward_weight_update_adam", "nnue_ftm_backward_weight_update_forward_adam"] \
        if opt == "adam" else ["nnue_sgd_step", "nnue_ftm_backward_weight_update", "nnue_ftm_backward_weight_update_forward"]
    names += ["nnue_ema_update", "nnue_lr_schedule_step"]
    timers = {f: {n: [] for n in names} for f in trainers}
    for _ in range(12):
        for f in trainers:
            trainers[f].step_many(GROUP, timers=timers[f])
    torch.cuda.synchronize()
    out["update_launches_us"] = {}
    for n in names:
        us = {f: [t0.elapsed_time(t1) * 1e3 for t0, t1 in timers[f][n]] for f in trainers}
        out["update_launches_us"][n] = {f: {"median": round(statistics.median(v), 2), "p10": round(percentile(v, 0.1), 2),
                                            "p90": round(percentile(v, 0.9), 2), "launches": len(v)} for f, v in us.items() if v}

    def update_calls(t):
        return [n for n, _, _ in (t._plan_update or [])]
    out["checks"] = {"update_calls": {f: update_calls(t) for f, t in trainers.items()}, "mode": plain.mode.describe(),
                     "same_mode": all(t.mode == plain.mode for t in trainers.values()),
                     "steps_done": dict({f: t.steps_done for f, t in trainers.items()}, single=single.steps_done),
                     "same_parameters_at_the_end": all(bool(torch.equal(t.flat_params, plain.flat_params)) for t in trainers.values()),
                     "mean_active_features": dict({f: round(t.active_stats()[0], 1) for f, t in trainers.items()},
                                                  single=round(single.active_stats()[0], 1))}
    del trainers, plain, single, single_lerp, bolt_on
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=200, help="groups per form after warm-up (at least 200)")
    ap.add_argument("--lr", type=float, default=None,
                    help="learning rate of every trainer (default: 0.01 for SGD, 1e-3 for Adam).  0 is the control: the parameters stay "
                         "put, so every form runs on the same map throughout -- the average is read and written all the same")
    args = ap.parse_args()
    if args.groups < 200:
        raise SystemExit("--groups >= 200")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py measures on the GPU and needs one")
    res = {"ema_decay": DECAY, "timing": "device events around blocks of groups, forms alternated in one process",
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, opt in CASES:
        res["cases"][f"{name}_{opt}"] = measure(name, opt, args.groups, args.lr)
    res["cases_with_ema_median_outside_plain_band"] = [k for k, v in res["cases"].items() if not v["ema_median_inside_plain_band"]]
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
