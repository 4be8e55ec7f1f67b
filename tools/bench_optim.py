"""The optimizer half of the reference loop (train.py:363-366 on the optimizer of train.py:455-471) on the GPU.

For the C2 and C4 parameter sets of bench.py's WORKLOADS (the NNUE module's own parameters, random gradients) it times one
optimizer step with the clip, four forms, alternated in one process:
  ours         nnue_hip.optim.SGD / Adam(max_grad_norm=1.0): nnue_multi_*_step over the parameter list;
  torch        clip_grad_norm_ + torch.optim.SGD / Adam (torch's default: foreach on GPU tensors);
  torch_fused  clip_grad_norm_ + torch.optim.SGD / Adam(fused=True), or the error its construction / step raised;
  flat         nnue_sgd_step / nnue_adam_step on one flat buffer of the same element count (the trainer's form).
ms: device events around `steps` steps, per step; host_us: host time per step() call (the enqueue, no synchronise).  Median
over `reps` alternated repeats.  bytes: what ours must move per step (SGD with momentum: read g for the norm; read p, g, m;
write p, m = 6 passes over the parameters; Adam 8), and the share of HBM peak (8 TB/s) and of the ~6.3 TB/s achievable.

Then the whole reference loop at C2 on the module path (zero_grad, forward, cross_entropy, backward, clip + step) with
torch.optim.SGD + clip_grad_norm_ and with nnue_hip.optim.SGD: images/s and ms/step, with and without a per-step
loss.item().  GPU only; fails without one.  Prints one JSON object:  python tools/bench_optim.py > profiles/optim_step.json"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))
sys.path.insert(0, str(ROOT))

import nnue  # noqa: E402
from bench import HBM_PEAK_GBS, OPT, WORKLOADS  # noqa: E402
from nnue_hip import lib, optim  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0  # MI355X_MICROARCH.md: ~6.3 TB/s achievable
DEV = "cuda"


def model_of(name):
    c = WORKLOADS[name]
    return nnue.NNUE(nnue.GridFeatureSet(c["grid"], c["fps"]), c["l1"], c["l2"], c["l3"], num_classes=c["classes"],
                     input_size=c["image"]).to(DEV)


def timed(fn, steps):
    """(device ms per step, host us per call) over `steps` calls."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    h0 = time.perf_counter()
    for _ in range(steps):
        fn()
    h1 = time.perf_counter()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps, (h1 - h0) * 1e6 / steps


class Forms:
    """The four forms over one parameter set; each keeps its own copy of the parameters and state."""

    def __init__(self, model, kind):
        self.kind = kind
        base = [p for n, p in model.named_parameters() if n != "nnue2score"]  # the reference leaves it without a gradient
        self.tensors = len(base)
        gen = torch.Generator(device=DEV).manual_seed(0)
        self.count = sum(p.numel() for p in base)

        def clone_set():
            ps = [torch.nn.Parameter(p.detach().clone()) for p in base]
            for p in ps:
                p.grad = torch.randn(p.shape, generator=gen, device=DEV) * 1e-3
            return ps

        hyper = dict(lr=OPT["lr"], momentum=OPT["momentum"], weight_decay=OPT["weight_decay"]) if kind == "sgd" else \
            dict(lr=1e-3, weight_decay=OPT["weight_decay"])
        tcls = torch.optim.SGD if kind == "sgd" else torch.optim.Adam
        ocls = optim.SGD if kind == "sgd" else optim.Adam
        self.fns, self.errors = {}, {}
        ps = clone_set()
        ours = ocls(ps, max_grad_norm=OPT["max_grad_norm"], **hyper)
        self.fns["ours"] = ours.step
        for name, extra in (("torch", {}), ("torch_fused", {"fused": True})):
            try:
                ps = clone_set()
                opt = tcls(ps, **hyper, **extra)

                def fn(ps=ps, opt=opt):
                    torch.nn.utils.clip_grad_norm_(ps, OPT["max_grad_norm"])
                    opt.step()

                fn()
                torch.cuda.synchronize()
                self.fns[name] = fn
            except Exception as e:  # noqa: BLE001 -- recorded, not hidden: torch's fused form may not exist on this build
                self.errors[name] = f"{type(e).__name__}: {e}"
        flat_p = torch.randn(self.count, generator=gen, device=DEV)
        flat_g = torch.randn(self.count, generator=gen, device=DEV) * 1e-3
        m, v = torch.zeros_like(flat_p), torch.zeros_like(flat_p)
        scratch = torch.empty((lib.sgd_scratch_bytes(self.count),), dtype=torch.uint8, device=DEV)
        norm = torch.zeros((), device=DEV)
        counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
        if kind == "sgd":
            self.fns["flat"] = lambda: lib.sgd_step(flat_p, flat_g, m, OPT["lr"], OPT["momentum"], OPT["weight_decay"],
                                                    OPT["max_grad_norm"], 1.0, False, norm, scratch)
        else:
            self.fns["flat"] = lambda: lib.adam_step(flat_p, flat_g, m, v, counter, 1e-3, weight_decay=OPT["weight_decay"],
                                                     max_norm=OPT["max_grad_norm"], norm_out=norm, scratch=scratch)


def optimizer_steps(name, kind, steps, reps):
    model = model_of(name)
    forms = Forms(model, kind)
    del model
    for fn in forms.fns.values():  # warm-up: lazy state, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms.fns}
    for _ in range(reps):
        for k, fn in forms.fns.items():
            samples[k].append(timed(fn, steps))
    passes = 6 if kind == "sgd" else 8
    nbytes = passes * 4 * forms.count
    out = {"elements": forms.count, "tensors": forms.tensors, "bytes_ours": nbytes, "forms": {}}
    for k, s in samples.items():
        ms = statistics.median(x[0] for x in s)
        out["forms"][k] = {"ms": round(ms, 5), "host_us": round(statistics.median(x[1] for x in s), 2),
                           "ms_spread": [round(min(x[0] for x in s), 5), round(max(x[0] for x in s), 5)]}
    ours = out["forms"]["ours"]["ms"]
    out["ours_over_flat"] = round(ours / out["forms"]["flat"]["ms"], 4)
    out["ours_hbm_peak_share"] = round(nbytes / (ours * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
    out["ours_hbm_achievable_share"] = round(nbytes / (ours * 1e-3) / (HBM_ACHIEVABLE_GBS * 1e9), 4)
    if forms.errors:
        out["errors"] = forms.errors
    return out


def reference_loop(steps, reps):
    """train.py:359-366 at C2 on the module path, torch's optimizer + clip_grad_norm_ against ours."""
    c = WORKLOADS["c2"]
    gen = torch.Generator(device=DEV).manual_seed(1)
    images = torch.randn(c["batch"], 3, c["image"], c["image"], generator=gen, device=DEV)
    labels = torch.randint(0, c["classes"], (c["batch"],), generator=gen, device=DEV)
    torch.manual_seed(0)
    models = {k: model_of("c2") for k in ("torch", "ours")}
    models["ours"].load_state_dict(models["torch"].state_dict())
    hyper = dict(lr=OPT["lr"], momentum=OPT["momentum"], weight_decay=OPT["weight_decay"])
    opts = {"torch": torch.optim.SGD(models["torch"].parameters(), **hyper),
            "ours": optim.SGD(models["ours"].parameters(), max_grad_norm=OPT["max_grad_norm"], **hyper)}

    def step(k, item):
        model, opt = models[k], opts[k]
        opt.zero_grad()
        loss = F.cross_entropy(model(images), labels)
        loss.backward()
        if k == "torch":
            torch.nn.utils.clip_grad_norm_(model.parameters(), OPT["max_grad_norm"])
        opt.step()
        if item:
            loss.item()

    for k in models:
        for _ in range(5):
            step(k, False)
    torch.cuda.synchronize()
    out = {}
    for item in (False, True):
        samples = {k: [] for k in models}
        for _ in range(reps):
            for k in models:
                samples[k].append(timed(lambda: step(k, item), steps)[0])
        for k, s in samples.items():
            ms = statistics.median(s)
            out[f"{k}{'_item' if item else ''}"] = {"ms_per_step": round(ms, 4), "images_per_sec": round(c["batch"] / (ms * 1e-3), 1),
                                                    "ms_spread": [round(min(s), 4), round(max(s), 4)]}
    return {"batch": c["batch"], **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-steps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU and needs one")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "steps": args.steps, "reps": args.reps,
           "optimizer_step": {}, "hbm_peak_gbs": HBM_PEAK_GBS, "hbm_achievable_gbs": HBM_ACHIEVABLE_GBS}
    for name in ("c2", "c4"):
        for kind in ("sgd", "adam"):
            res["optimizer_step"][f"{name}_{kind}"] = optimizer_steps(name, kind, args.steps, args.reps)
            torch.cuda.empty_cache()
    res["reference_loop_c2"] = reference_loop(args.loop_steps, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
