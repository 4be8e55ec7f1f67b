"""Throughput of the GPU input pipeline alone and feeding the C2 training step.
Prints one JSON object:  python tools/bench_input_pipeline.py > input_pipeline.json

``--policies`` instead measures every form of the pipeline kernels in one process (profiles/input_pipeline_medium.json):
device-event medians of plain / light (nnue_load_batch) and none + resize / medium / medium + resize
(nnue_load_batch_policy), interleaved call by call, at the CIFAR shape and at batch 128 of 224 x 224, and the C2 step fed
in place (train_epoch) under the light and the medium policy."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nnue-vision_amd"))

import nnue  # noqa: E402
from nnue_hip.input_pipeline import GpuImageDataset, train_epoch  # noqa: E402
from nnue_hip.trainer import NnueTrainer  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    n, b = 50000, 512  # CIFAR-10 train split shape, BASELINE configs[1] batch
    rng = np.random.RandomState(0)
    ds_plain = GpuImageDataset(rng.randint(0, 256, (n, 32, 32, 3), dtype=np.uint8), rng.randint(0, 10, n))
    ds_aug = GpuImageDataset(ds_plain.images, ds_plain.labels, augment=True, seed=1)
    order = torch.randperm(n, device="cuda")
    batches = [order[i * b:(i + 1) * b] for i in range(n // b)]
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 1024, 128, 32, num_classes=10).cuda()
    tr = NnueTrainer(model, b, (32, 32), lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0, input_slots=8)
    out, lab = tr.inputs[0]
    res = {"dataset": [n, 32, 32, 3], "batch": b, "input_slots": 8}
    for name, ds in (("plain", ds_plain), ("light_aug", ds_aug)):
        fn = lambda i: ds.batch(batches[i % len(batches)], out=out, labels_out=lab)
        timed(fn, 50)
        dt = timed(fn, 500)
        res[f"load_batch_{name}_us"] = dt * 1e6
        res[f"load_batch_{name}_images_per_s"] = b / dt
        res[f"load_batch_{name}_GBps"] = b * 32 * 32 * 3 * 5 / dt / 1e9  # 1 B read + 4 B written per value

    def step_only(i):
        tr.step(slot=i & 1)

    def step_fed(i):
        s = i & 1
        ds_aug.batch(batches[i % len(batches)], out=tr.inputs[s][0], labels_out=tr.inputs[s][1])
        tr.step(slot=s)

    for name, fn in (("step_resident_input", step_only), ("step_fed_by_pipeline", step_fed)):
        timed(fn, 50)
        dt = timed(fn, 500)
        res[f"{name}_ms"] = dt * 1e3
        res[f"{name}_images_per_s"] = b / dt
    loader = ds_aug.loader(b, shuffle=True, drop_last=True)
    train_epoch(tr, loader)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    epochs = 5
    for _ in range(epochs):
        _, steps = train_epoch(tr, loader)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / (epochs * steps)
    res["train_epoch_ms"] = dt * 1e3
    res["train_epoch_images_per_s"] = b / dt
    res["epoch_seconds_cifar10"] = dt * steps
    print(json.dumps(res))


def event_medians(forms, reps=300, warm=30):
    """forms: name -> callable(i).  One timed call of each form per round, the forms interleaved; microseconds."""
    events = {name: [] for name in forms}
    for i in range(warm + reps):
        for name, fn in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn(i)
            t1.record()
            if i >= warm:
                events[name].append((t0, t1))
    torch.cuda.synchronize()
    out = {}
    for name, ev in events.items():
        us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        out[name] = {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90))}
    return out


def policy_forms(n, b, hw, stored_for_resize, out_hw_resize):
    """The five forms at one shape: batches of b images of hw; the resize forms read a dataset stored at stored_for_resize."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    images = torch.randint(0, 256, (n, hw[0], hw[1], 3), dtype=torch.uint8, device="cuda", generator=gen)
    labels = torch.randint(0, 10, (n,), device="cuda", generator=gen)
    if tuple(stored_for_resize) == tuple(hw):
        other = images
    else:
        other = torch.randint(0, 256, (n, stored_for_resize[0], stored_for_resize[1], 3), dtype=torch.uint8, device="cuda", generator=gen)
    sets = {"plain": GpuImageDataset(images, labels),
            "light": GpuImageDataset(images, labels, augment="light", seed=1),
            "none_resize": GpuImageDataset(other, labels, out_hw=out_hw_resize),
            "medium": GpuImageDataset(images, labels, augment="medium", seed=1),
            "medium_resize": GpuImageDataset(other, labels, augment="medium", seed=1, out_hw=out_hw_resize)}
    order = torch.randperm(n, device="cuda")
    batches = [order[i * b:(i + 1) * b] for i in range(n // b)]
    forms, bytes_moved = {}, {}
    for name, ds in sets.items():
        oh, ow = ds.output_hw
        out, lab = torch.empty(b, 3, oh, ow, device="cuda"), torch.empty(b, dtype=torch.int64, device="cuda")
        forms[name] = (lambda i, ds=ds, out=out, lab=lab: ds.batch(batches[i % len(batches)], out=out, labels_out=lab))
        bytes_moved[name] = b * 3 * (ds.image_hw[0] * ds.image_hw[1] + 4 * oh * ow)  # every source byte once + the float32 output
    res = event_medians(forms)
    for name in res:
        res[name]["stored_hw"], res[name]["out_hw"] = list(sets[name].image_hw), list(sets[name].output_hw)
        res[name]["GBps_at_median"] = bytes_moved[name] / res[name]["median_us"] / 1e3
    return res


def main_policies():
    res = {"method": "device events around each call, one call of every form per round (interleaved), 300 rounds after 30 warm-up",
           "cifar_b512_32x32": policy_forms(50000, 512, (32, 32), (32, 32), (96, 96)),
           "b128_224x224": policy_forms(1024, 128, (224, 224), (256, 256), (224, 224))}
    n, b = 50000, 512
    rng = np.random.RandomState(0)
    images, labels = rng.randint(0, 256, (n, 32, 32, 3), dtype=np.uint8), rng.randint(0, 10, n)
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 1024, 128, 32, num_classes=10).cuda()
    tr = NnueTrainer(model, b, (32, 32), lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0, input_slots=8)
    loaders = {name: GpuImageDataset(images, labels, augment=name, seed=1).loader(b, shuffle=True, drop_last=True)
               for name in ("light", "medium")}
    for loader in loaders.values():
        train_epoch(tr, loader)
    times = {name: [] for name in loaders}
    for _ in range(5):  # interleaved epochs
        for name, loader in loaders.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, steps = train_epoch(tr, loader)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    res["c2_train_epoch_ms_per_step"] = {name: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
                                         for name, t in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main_policies() if "--policies" in sys.argv[1:] else main()
