"""What soft targets cost in the step (NnueTrainer label_smoothing / two_labels; include/nnue_hip.h "soft targets",
nnue_mix_batch), at bench.py's C2 (batch 512, 800 -> 1024/128/32 -> 10) and at the 224x224 shape (C4, batch 128), SGD(0.9)
with clip 1.0, single rank, 8 input slots, groups of 8 steps.  Three forms, three trainers in ONE process, alternated block
by block:
  a  plain groups               step_many(0..7) of a default trainer: today's launches -- the baseline;
  b  soft groups                the same group with label_smoothing = 0.1 and two_labels (the SOFT arm of the tail kernel);
  c  soft groups + mixing       like b, with one nnue_mix_batch launch per slot ahead of each group (mix_draw's CutMix boxes:
                                swapping in place, group after group, keeps the slots' pixel statistics, repeated mixup would not).
Every sample is a block of --block groups between two device events; at least --groups groups per form after a warm-up of
every graph; medians with the 10th and 90th percentiles and the ratios b/a and c/a of the medians.  nnue_mix_batch is also
timed on its own (mixup, blocks of launches on one slot) with the bytes it moves -- one read and one write of the float
batch -- over that time.  No threshold is built in; form a is expected to agree with a plain ``bench.py`` run of the same
commit within the spread reported here.

  python tools/bench_soft_targets.py > profiles/soft_targets.json
  python tools/bench_soft_targets.py --lr 0 > profiles/soft_targets_lr0.json     (the control: see --lr)

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
ALPHAS = dict(mixup_alpha=0.0, cutmix_alpha=1.0)  # form c swaps boxes only: in place, group after group, the slots keep their pixel statistics
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
    from nnue_hip import lib
    from nnue_hip.input_pipeline import mix_draw
    from nnue_hip.trainer import NnueTrainer
    c = SHAPES[name]
    dev = torch.device("cuda", 0)
    trainers = {}
    for form in "abc":
        torch.manual_seed(0)
        model = nnue.NNUE(nnue.GridFeatureSet(c["grid"], c["fps"]), c["l1"], c["l2"], c["l3"], num_classes=c["classes"],
                          input_size=c["image"]).to(dev)
        tr = NnueTrainer(model, c["batch"], (c["image"], c["image"]), use_graph=True, input_slots=SLOTS, **dict(OPT, lr=lr),
                         **({} if form == "a" else SOFT))
        gen = torch.Generator().manual_seed(1234)
        for s, (images, labels) in enumerate(tr.inputs):
            images.copy_(torch.randn(c["batch"], 3, c["image"], c["image"], generator=gen))
            labels.copy_(torch.randint(0, c["classes"], (c["batch"],), generator=gen))
            if form != "a":  # a second label and a weight per sample, as a mixed batch leaves them
                tr.soft_inputs[s][0].copy_(labels.flip(0))
                tr.soft_inputs[s][1].copy_(torch.rand(c["batch"], generator=gen))
        trainers[form] = tr
    draws = [0]

    def run_group(form):
        tr = trainers[form]
        if form == "c":
            for s in GROUP:
                draws[0] += 1
                mode, lam, y0, x0, hh, hw = mix_draw(7, draws[0], H=c["image"], W=c["image"], **ALPHAS)
                lib.mix_batch(tr.inputs[s][0], tr.inputs[s][1], mode, lam, (y0, x0, hh, hw), *tr.soft_inputs[s])
        tr.step_many(GROUP)

    for form in "abc":  # plans, every single-step graph, the group's graph
        for _ in range(2):
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
    # nnue_mix_batch alone: blocks of 50 mixup launches on slot 0 of form c
    tr = trainers["c"]
    mix_events = []
    for _ in range(40):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(50):
            lib.mix_batch(tr.inputs[0][0], tr.inputs[0][1], 1, 0.7, (0, 0, 0, 0), *tr.soft_inputs[0])
        t1.record()
        mix_events.append((t0, t1))
    torch.cuda.synchronize()
    mix_us = [t0.elapsed_time(t1) / 50 * 1e3 for t0, t1 in mix_events]
    moved = 2 * tr.inputs[0][0].numel() * 4  # every float of the batch is read once and written once
    out = {"shape": {k: v for k, v in c.items() if k != "block"}, "groups_per_form": len(samples["a"]) * block, "groups_per_sample": block,
           "steps_per_group": SLOTS, "forms": {}}
    labels = {"a": "plain groups (baseline)", "b": "soft groups: label_smoothing 0.1, two_labels",
              "c": "soft groups + one nnue_mix_batch per slot ahead of each group"}
    for form in "abc":
        s = summary(samples[form])
        out["forms"][form] = {"what": labels[form], "median_ms_per_step": s["median"], "p10_ms_per_step": s["p10"], "p90_ms_per_step": s["p90"],
                              "samples": s["samples"]}
    med = {form: statistics.median(samples[form]) for form in "abc"}
    out["b_over_a"] = round(med["b"] / med["a"], 4)
    out["c_over_a"] = round(med["c"] / med["a"], 4)
    out["b_minus_a_us_per_step"] = round((med["b"] - med["a"]) * 1e3, 3)
    out["c_minus_a_us_per_step"] = round((med["c"] - med["a"]) * 1e3, 3)
    s = summary(mix_us)
    out["mix_batch"] = {"what": "mixup launches back to back on one slot, host launch gaps included", "median_us": s["median"], "p10_us": s["p10"],
                        "p90_us": s["p90"], "bytes_moved": moved, "GB_per_s_at_median": round(moved / (s["median"] * 1e-6) / 1e9, 1)}

    def cls_calls(t):
        return sorted({n for n, _, _ in t._plan_local if n.startswith("nnue_classifier_train_step")})
    out["checks"] = {"baseline_classifier_calls": cls_calls(trainers["a"]), "soft_classifier_calls": cls_calls(trainers["b"]),
                     "steps_done": {f: trainers[f].steps_done for f in "abc"}}
    del trainers
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c4", help="comma-separated subset of: " + ", ".join(SHAPES))
    ap.add_argument("--groups", type=int, default=200, help="groups per form after warm-up (at least 200)")
    ap.add_argument("--lr", type=float, default=OPT["lr"],
                    help="learning rate of all three trainers.  0 is the control: the parameters stay put, so the three forms run on "
                         "the same map throughout (the kernels' time depends on the active-feature density, and trainers that learn "
                         "from different targets drift apart in it)")
    args = ap.parse_args()
    shapes = [s for s in args.shapes.split(",") if s]
    if any(s not in SHAPES for s in shapes) or args.groups < 200:
        raise SystemExit("shapes must be among " + ", ".join(SHAPES) + "; --groups >= 200")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_targets.py measures on the GPU and needs one")
    res = {"optimizer": dict(OPT, lr=args.lr, kind="sgd"), "soft": SOFT, "mix": ALPHAS,
           "timing": "device events around blocks of groups, forms alternated in one process", "device": torch.cuda.get_device_name(0),
           "shapes": {}}
    for s in shapes:
        res["shapes"][s] = measure(s, args.groups, args.lr)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
