"""What distillation costs in the step (NnueTrainer distill_alpha / distill_temperature; include/nnue_hip.h "soft targets", the
teacher arm), at bench.py's C2 (batch 512, 800 -> 1024/128/32 -> 10) and at the 224x224 shape (C4, batch 128, 1000 classes),
SGD(0.9) with clip 1.0, single rank, 8 input slots, groups of 8 steps.  Four forms, four trainers in ONE process, alternated
block by block:
  a  plain groups               step_many(0..7) of a default trainer: today's launches -- the baseline;
  b  soft groups                the same group with label_smoothing = 0.1 and two_labels (the SOFT arm of the tail kernel);
  d  distill groups             like b, with distill_alpha = 0.7, T = 2 (the DISTILL arm) on teacher logits already resident in
                                ``teacher_inputs`` -- B C 4 bytes more per step;
  t  distill groups + teacher   like d, with a drop-in nnue.NNUE teacher of the same shape run on every slot ahead of each group
                                under no_grad, its logits copied into ``teacher_inputs[s]`` (what train_epoch does): for orientation,
                                the teacher is the user's.
Every sample is a block of --block groups between two device events; at least --groups groups per form after a warm-up of
every graph; medians with the 10th and 90th percentiles and the ratios b/a, d/a and t/a of the medians.  The classifier
call -- the one the arms differ in -- is also timed on its own in eager steps (device events around the recorded call), so
that a ratio that stands apart can be traced to it or away from it.  No threshold is built in.

  python tools/bench_distill.py > profiles/distill.json
  python tools/bench_distill.py --lr 0 > profiles/distill_lr0.json     (the control: see --lr)

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
SOFT = dict(label_smoothing=0.1, two_labels=True)
DISTILL = dict(distill_alpha=0.7, distill_temperature=2.0)
FORMS = "abdt"
SLOTS = 8
GROUP = tuple(range(SLOTS))


def percentile(values, q):
    v = sorted(values)
    k = (len(v) - 1) * q
    lo, hi = int(k), min(int(k) + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (k - lo)


def summary(v):
    return {"median": round(statistics.median(v), 5), "p10": round(percentile(v, 0.1), 5), "p90": round(percentile(v, 0.9), 5), "samples": len(v)}


def measure(name: str, groups: int, lr: float) -> dict:
    import torch
    import nnue
    from nnue_hip.trainer import NnueTrainer
    c = SHAPES[name]
    dev = torch.device("cuda", 0)

    def build():
        return nnue.NNUE(nnue.GridFeatureSet(c["grid"], c["fps"]), c["l1"], c["l2"], c["l3"], num_classes=c["classes"],
                         input_size=c["image"]).to(dev)
    torch.manual_seed(1)
    teacher = build().eval()
    trainers = {}
    for form in FORMS:
        torch.manual_seed(0)
        tr = NnueTrainer(build(), c["batch"], (c["image"], c["image"]), use_graph=True, input_slots=SLOTS, **dict(OPT, lr=lr),
                         **({} if form == "a" else SOFT), **(DISTILL if form in "dt" else {}))
        gen = torch.Generator().manual_seed(1234)
        for s, (images, labels) in enumerate(tr.inputs):
            images.copy_(torch.randn(c["batch"], 3, c["image"], c["image"], generator=gen))
            labels.copy_(torch.randint(0, c["classes"], (c["batch"],), generator=gen))
            if form != "a":  # a second label and a weight per sample, as a mixed batch leaves them
                tr.soft_inputs[s][0].copy_(labels.flip(0))
                tr.soft_inputs[s][1].copy_(torch.rand(c["batch"], generator=gen))
            if form in "dt":
                with torch.no_grad():
                    tr.teacher_inputs[s].copy_(teacher(images))
        trainers[form] = tr

    def run_group(form):
        tr = trainers[form]
        if form == "t":
            with torch.no_grad():
                for s in GROUP:
                    tr.teacher_inputs[s].copy_(teacher(tr.inputs[s][0]))
        tr.step_many(GROUP)

    for form in FORMS:  # plans, every single-step graph, the group's graph
        for _ in range(2):
            for s in GROUP:
                trainers[form].step(slot=s)
        for _ in range(3):
            run_group(form)
    torch.cuda.synchronize()
    block = c["block"]
    samples = {form: [] for form in FORMS}
    events = []
    for _ in range((groups + block - 1) // block):
        for form in FORMS:  # alternated: one block of every form per round
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(block):
                run_group(form)
            t1.record()
            events.append((form, t0, t1))
    torch.cuda.synchronize()
    for form, t0, t1 in events:
        samples[form].append(t0.elapsed_time(t1) / (block * SLOTS))  # ms per step
    # the classifier call on its own: eager steps from the recorded plans, device events around the one call the arms differ in
    # (the distill and soft entry points are timed under the plain call's name)
    cls_us = {}
    for form in "abd":
        tr = trainers[form]
        key = "nnue_classifier_train_step_bucketed" if tr.bucket_plan is not None else "nnue_classifier_train_step"
        timers = {key: []}
        for _ in range(5):
            for s in GROUP:
                tr.step(slot=s, timers=timers)
        torch.cuda.synchronize()
        cls_us[form] = [t0.elapsed_time(t1) * 1e3 for t0, t1 in timers[key]]
    out = {"shape": {k: v for k, v in c.items() if k != "block"}, "groups_per_form": len(samples["a"]) * block, "groups_per_sample": block,
           "steps_per_group": SLOTS, "teacher_logit_bytes_per_step": c["batch"] * c["classes"] * 4, "forms": {}}
    labels = {"a": "plain groups (baseline)", "b": "soft groups: label_smoothing 0.1, two_labels",
              "d": "distill groups: b with distill_alpha 0.7, T 2, teacher logits resident in the slots",
              "t": "distill groups + a drop-in NNUE teacher's forward on every slot ahead of each group"}
    for form in FORMS:
        s = summary(samples[form])
        out["forms"][form] = {"what": labels[form], "median_ms_per_step": s["median"], "p10_ms_per_step": s["p10"], "p90_ms_per_step": s["p90"],
                              "samples": s["samples"]}
    med = {form: statistics.median(samples[form]) for form in FORMS}
    for form in "bdt":
        out[f"{form}_over_a"] = round(med[form] / med["a"], 4)
        out[f"{form}_minus_a_us_per_step"] = round((med[form] - med["a"]) * 1e3, 3)
    out["d_over_b"] = round(med["d"] / med["b"], 4)
    out["classifier_call_us"] = {"what": "the classifier step's call alone in eager steps (every launch it makes), device events around it",
                                 **{form: summary(cls_us[form]) for form in "abd"}}

    def cls_calls(t):
        return sorted({n for n, _, _ in t._plan_local if n.startswith("nnue_classifier_train_step")})
    out["checks"] = {"classifier_calls": {form: cls_calls(trainers[form]) for form in FORMS},
                     "steps_done": {f: trainers[f].steps_done for f in FORMS}}
    del trainers
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c4", help="comma-separated subset of: " + ", ".join(SHAPES))
    ap.add_argument("--groups", type=int, default=200, help="groups per form after warm-up (at least 200)")
    ap.add_argument("--lr", type=float, default=OPT["lr"],
                    help="learning rate of all trainers.  0 is the control: the parameters stay put, so the forms run on the same map "
                         "throughout (the kernels' time depends on the active-feature density, and trainers that learn from different "
                         "targets drift apart in it)")
    args = ap.parse_args()
    shapes = [s for s in args.shapes.split(",") if s]
    if any(s not in SHAPES for s in shapes) or args.groups < 200:
        raise SystemExit("shapes must be among " + ", ".join(SHAPES) + "; --groups >= 200")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill.py measures on the GPU and needs one")
    res = {"optimizer": dict(OPT, lr=args.lr, kind="sgd"), "soft": SOFT, "distill": DISTILL,
           "timing": "device events around blocks of groups, forms alternated in one process", "device": torch.cuda.get_device_name(0),
           "shapes": {}}
    for s in shapes:
        res["shapes"][s] = measure(s, args.groups, args.lr)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
