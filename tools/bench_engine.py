"""Throughput of the engine's integer inference on the GPU beside the reference's way of getting the
same numbers: one `nnue_inference` subprocess per image (evaluate.py:143-176), timed on this host with oracle/_ref.
Prints one JSON object:  python tools/bench_engine.py > gpurun_out/engine_bench.json"""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))

import nnue  # noqa: E402
import serialize  # noqa: E402
from nnue_hip.engine import EngineModel  # noqa: E402


STACK_SHAPES = [
    {"name": "cifar_32x32", "g": 10, "fps": 8, "l1": 1024, "l2": 128, "l3": 32, "classes": 10, "size": 32, "batch": 4096},
    {"name": "224x224", "g": 32, "fps": 64, "l1": 512, "l2": 32, "l3": 32, "classes": 10, "size": 224, "batch": 1024},
]


def _alternate(calls, warmup, repeats):
    """Runs the calls in turn, warmup + repeats rounds; median event time of each over the timed rounds."""
    return [st["median"] for st in _alternate_spread(calls, warmup, repeats)]


def _alternate_spread(calls, warmup, repeats):
    """_alternate with the spread: {"median", "p10", "p90"} in ms for each call."""
    times = [[] for _ in calls]
    for t in range(warmup + repeats):
        for i, fn in enumerate(calls):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn(t)
            t1.record()
            if t >= warmup:
                times[i].append((t0, t1))
    torch.cuda.synchronize()
    out = []
    for ts in times:
        ms = sorted(a.elapsed_time(b) for a, b in ts)
        out.append({"median": statistics.median(ms), "p10": ms[len(ms) // 10], "p90": ms[(len(ms) * 9) // 10]})
    return out


def _stack_case(shape, K):
    """The model file, engines and images of one --stacks row: (plain, auto, x)."""
    torch.manual_seed(0)
    size, B = shape["size"], shape["batch"]
    model = nnue.NNUE(nnue.GridFeatureSet(shape["g"], shape["fps"]), shape["l1"], shape["l2"], shape["l3"],
                      num_classes=shape["classes"], input_size=size, num_ls_buckets=K)
    with torch.no_grad():
        model.conv.weight.abs_()
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "m.nnue"
        with contextlib.redirect_stdout(sys.stderr):  # keep stdout to the one JSON object
            serialize.serialize_model(model, path)
        plain, auto = EngineModel.load(path), EngineModel.load(path, bucket="auto")
    n = 3 * size * size
    x = torch.randn(B, n, device="cuda") * 0.3 - 1.5
    bright = torch.arange(n, device="cuda")[None, :] < (torch.arange(B, device="cuda") * n // (B - 1))[:, None]
    x = (x + 3.0 * bright).view(B, 3, size, size).contiguous()
    return model, plain, auto, x


PATH_BATCHES = {"c2": (512, 4096, 16, 64, 128, 256, 1024, 2048), "224": (128, 1024, 1, 2, 4, 8, 16, 32, 64, 256, 512)}


def bench_paths(shape_key, only, batches, warmup, repeats, extras):
    """--shape {c2,224}: the gather form of evaluate_logits against the matrix form (path="gather" / "matrix"), in this process,
    alternating inside one loop, on the model, file and images of the --stacks rows (single-stack load, so `gather` is that row's
    plain_ms at its batch).  Per batch: median, 10th and 90th percentile of device-event-timed calls after warm-up; the first
    two batches are the headline ones, the rest the crossover sweep behind engine._MATRIX_MIN_MAP_BYTES.  --path P times that
    form alone (what a rocprofv3 --kernel-trace run of this tool wants).  With --extras: the pack launch, requantize with and
    without planes, and evaluate_engine over resident images on either form.
        python tools/bench_engine.py --shape 224 --extras > engine_matrix_224.json"""
    import evaluate
    shape = dict(STACK_SHAPES[0 if shape_key == "c2" else 1])
    batches = tuple(batches) if batches else PATH_BATCHES[shape_key]
    shape["batch"] = max(max(batches), 2)
    model, engine, _, x_all = _stack_case(shape, 8)
    F, L1 = int(engine.header["num_features"]), shape["l1"]
    res = {"device": torch.cuda.get_device_name(0), "shape": shape["name"], "F": F, "L1": L1, "planes": None, "warmup": warmup,
           "repeats": repeats, "timing": "median (p10, p90) of device-event-timed calls, gather and matrix alternating in one loop",
           "cases": []}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    engine.prepare_matrix()
    t1.record()
    torch.cuda.synchronize()
    res["planes"], res["prepare_matrix_first_ms"] = engine.table_planes, t0.elapsed_time(t1)
    for B in batches:
        x = x_all[torch.linspace(0, x_all.shape[0] - 1, B).long().cuda()].contiguous()  # the whole dark-to-bright range at any B
        g, m = engine.evaluate_logits(x, path="gather"), engine.evaluate_logits(x, path="matrix")
        assert torch.equal(g[0], m[0]) and torch.equal(g[1], m[1])
        row = {"batch": B, "map_bytes": B * F, "mean_density": float(g[1].double().mean())}
        names = [only] if only else ["gather", "matrix"]
        stats = _alternate_spread([lambda t, p=p: engine.evaluate_logits(x, path=p) for p in names], warmup, repeats)
        for p, st in zip(names, stats):
            row[p + "_ms"], row[p + "_p10_ms"], row[p + "_p90_ms"] = st["median"], st["p10"], st["p90"]
        if not only:
            row["gather_over_matrix"] = row["gather_ms"] / row["matrix_ms"]
            row["matrix_wins_beyond_spread"] = row["matrix_p90_ms"] < row["gather_p10_ms"]
            row["int8_macs_per_s"] = engine.table_planes * B * F * L1 / (row["matrix_ms"] * 1e-3)  # the whole call's time
        print(json.dumps(row), file=sys.stderr)
        res["cases"].append(row)
    if extras and not only:
        stream = torch.cuda.current_stream().cuda_stream
        st = _alternate_spread([lambda t: engine._pack_planes(stream)], warmup, repeats)[0]
        res["pack_launch_ms"] = st
        res["pack_gbs"] = (2 * F * L1 + engine._planes.numel()) / (st["median"] * 1e-3) / 1e9
        single = nnue.NNUE(nnue.GridFeatureSet(shape["g"], shape["fps"]), shape["l1"], shape["l2"], shape["l3"],
                           num_classes=shape["classes"], input_size=shape["size"]).cuda()
        live = EngineModel.from_model(single)

        def requantize_ms():
            ts = []
            for _ in range(warmup + repeats):
                torch.cuda.synchronize()
                a = time.perf_counter()
                live.requantize(single)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - a) * 1e3)
            return statistics.median(ts[warmup:])

        res["requantize_call_ms"] = requantize_ms()
        live.prepare_matrix()
        res["requantize_call_with_planes_ms"] = requantize_ms()
        # evaluate_engine over resident images, gather form against auto
        per, nb = (1000, 10) if shape_key == "224" else (500, 20)
        loader = [(x_all[:per].roll(i, 0).contiguous(), torch.randint(0, shape["classes"], (per,), device="cuda")) for i in range(nb)]
        out = {}
        for name in ("gather", "auto"):
            os.environ["NNUE_ENGINE_PATH"] = name
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                a = time.perf_counter()
                metrics = evaluate.evaluate_engine(engine, loader)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - a) * 1e3)
            out[name] = {"wall_ms": statistics.median(ts), "ms_per_sample": metrics["ms_per_sample"], "acc": metrics["acc"],
                         "latent_density": metrics["latent_density"]}
        os.environ.pop("NNUE_ENGINE_PATH", None)
        assert out["gather"]["acc"] == out["auto"]["acc"] and out["gather"]["latent_density"] == out["auto"]["latent_density"]
        res["evaluate_engine"] = dict(out, images=per * nb, batch=per)
    print(json.dumps(res))


U8_BATCHES = {"224": (128, 1024), "c2": (512, 4096)}
U8_STREAMS = 1024


def bench_u8(shape_keys, only, batches, warmup, repeats):
    """--u8: the uint8 input form against the parent's way of evaluating a resident uint8 dataset, in this process, on one
    GpuImageDataset per shape.  (a) `float`: dataset.batch(idx) then evaluate_logits -- both launches inside the timed window;
    (b) `u8`: evaluate_logits_u8(dataset.images, idx).  The two alternate inside one loop, for path="matrix" and "gather", at
    --shape 224 (batch 128 and 1024) and c2 (512 and 4096); then stream(1024).step_u8 against batch + step on frames that
    alternate between two index sets.  Per row: median, 10th and 90th percentile of device-event-timed calls after warm-up;
    the two forms' logits and densities are asserted bitwise equal on the timed inputs first.  --path P times that path
    alone (what a rocprofv3 --kernel-trace run wants: engine_conv_kernel and engine_conv_u8_kernel are both in it).
        python tools/bench_engine.py --u8 > profiles/engine_u8.json"""
    from nnue_hip.input_pipeline import GpuImageDataset
    res = {"device": torch.cuda.get_device_name(0), "warmup": warmup, "repeats": repeats,
           "timing": "median (p10, p90) of device-event-timed calls; float = dataset.batch(idx) + evaluate_logits, u8 = "
                     "evaluate_logits_u8(dataset.images, idx), alternating in one loop on one resident uint8 dataset",
           "shapes": []}
    for key in shape_keys:
        shape = dict(STACK_SHAPES[0 if key == "c2" else 1])
        sizes = tuple(batches) if batches else U8_BATCHES[key]
        shape["batch"] = 2
        _, engine, _, _ = _stack_case(shape, 1)
        size, n = shape["size"], max(max(sizes), U8_STREAMS)
        gen = torch.Generator(device="cuda").manual_seed(7)
        images = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, device="cuda", generator=gen)
        ds = GpuImageDataset(images, torch.zeros(n, dtype=torch.int64))
        engine.prepare_matrix()
        F = int(engine.header["num_features"])
        out = {"shape": shape["name"], "F": F, "L1": shape["l1"], "frame_bytes": 3 * size * size, "cases": []}
        for B in sizes:
            idx = torch.randperm(n, device="cuda", generator=gen)[:B]
            for path in ([only] if only else ["matrix", "gather"]):
                a = engine.evaluate_logits(ds.batch(idx)[0], path=path)
                b = engine.evaluate_logits_u8(ds.images, idx, path=path)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
                row = {"batch": B, "path": path, "mean_density": float(a[1].double().mean()),
                       "u8_bytes_read": B * 3 * size * size, "float_bytes_written_and_read": 2 * 4 * B * 3 * size * size}
                stats = _alternate_spread([lambda t: engine.evaluate_logits(ds.batch(idx)[0], path=path),
                                           lambda t: engine.evaluate_logits_u8(ds.images, idx, path=path)], warmup, repeats)
                for name, st in zip(("float", "u8"), stats):
                    row[name + "_ms"], row[name + "_p10_ms"], row[name + "_p90_ms"] = st["median"], st["p10"], st["p90"]
                row["float_over_u8"] = row["float_ms"] / row["u8_ms"]
                row["u8_wins_beyond_spread"] = row["u8_p90_ms"] < row["float_p10_ms"]
                row["u8_loses_beyond_spread"] = row["u8_p10_ms"] > row["float_p90_ms"]
                print(json.dumps(row), file=sys.stderr)
                out["cases"].append(row)
        if not only:
            S = U8_STREAMS
            sets = [torch.randperm(n, device="cuda", generator=gen)[:S] for _ in range(2)]
            sf, su = engine.stream(S), engine.stream(S)
            for t in range(2):
                a, b = sf.step(ds.batch(sets[t])[0]), su.step_u8(ds.images, sets[t])
                assert all(torch.equal(p, q) for p, q in zip(a, b))
            stats = _alternate_spread([lambda t: sf.step(ds.batch(sets[t & 1])[0]), lambda t: su.step_u8(ds.images, sets[t & 1])],
                                      warmup, repeats)
            row = {"streams": S}
            for name, st in zip(("float", "u8"), stats):
                row[name + "_ms"], row[name + "_p10_ms"], row[name + "_p90_ms"] = st["median"], st["p10"], st["p90"]
            row["float_over_u8"] = row["float_ms"] / row["u8_ms"]
            row["u8_wins_beyond_spread"] = row["u8_p90_ms"] < row["float_p10_ms"]
            print(json.dumps(row), file=sys.stderr)
            out["stream"] = row
        res["shapes"].append(out)
        del ds, images, engine
    print(json.dumps(res))


def bench_stacks(K, warmup, repeats):
    """--stacks K: per-image layer-stack selection (EngineModel.load(bucket="auto")) against the plain single-stack call, in
    this process, on the same K-stack file and the same images, at the CIFAR shape (10x10x8, 1024/128/32, batch 4096) and the
    224x224 shape (32x32x64, 512/32/32, batch 1024).  The conv weights are made non-negative and image b is dark noise with a
    bright prefix of b/(B-1) of its floats, so the active-feature counts spread over the stacks (`stack_counts`).  The two calls
    alternate inside one loop; times are medians of device-event-timed calls after warm-up, for evaluate_logits and for
    stream(B).step on frames that alternate between the batch and the batch rolled by one image.
        python tools/bench_engine.py --stacks 8 > profiles/engine_stacks.json"""
    res = {"device": torch.cuda.get_device_name(0), "stacks": K, "warmup": warmup, "repeats": repeats,
           "timing": "median of device-event-timed calls, plain and selected alternating in one loop", "cases": []}
    for shape in STACK_SHAPES:
        B = shape["batch"]
        _, plain, auto, x = _stack_case(shape, K)
        frames = (x, x.roll(1, 0).contiguous())
        logits, density, stack = auto.evaluate_logits(x, return_stacks=True)
        same = stack == 0  # rows of stack 0 must be the plain call's, bit for bit
        assert torch.equal(logits[same], plain.evaluate_logits(x)[0][same]) and bool((~same).any())
        row = {"shape": shape["name"], "batch": B, "F": int(auto.header["num_features"]), "L1": shape["l1"],
               "stack_counts": torch.bincount(stack.long(), minlength=K).tolist(),
               "mean_density": float(density.double().mean())}
        row["plain_ms"], row["selected_ms"] = _alternate([lambda t: plain.evaluate_logits(x), lambda t: auto.evaluate_logits(x)],
                                                         warmup, repeats)
        row["selected_over_plain"] = row["selected_ms"] / row["plain_ms"]
        sp, sa = plain.stream(B), auto.stream(B)
        row["stream_plain_ms"], row["stream_selected_ms"] = _alternate(
            [lambda t: sp.step(frames[t & 1]), lambda t: sa.step(frames[t & 1])], warmup, repeats)
        row["stream_selected_over_plain"] = row["stream_selected_ms"] / row["stream_plain_ms"]
        print(json.dumps(row), file=sys.stderr)
        res["cases"].append(row)
        del x, frames, sp, sa
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--stacks", type=int, default=0, help="K: time per-image stack selection against the plain call instead")
    ap.add_argument("--shape", choices=("c2", "224"), help="time the gather form against the matrix form at this shape instead")
    ap.add_argument("--path", choices=("gather", "matrix"), help="with --shape: time this form alone")
    ap.add_argument("--batches", type=int, nargs="*", help="with --shape: the batch sizes (default: headline pair + sweep)")
    ap.add_argument("--extras", action="store_true", help="with --shape: also pack, requantize and evaluate_engine")
    ap.add_argument("--u8", action="store_true", help="time the uint8 input form against batch + evaluate_logits (--shape: one shape)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args()
    if args.u8:
        if not torch.cuda.is_available():
            raise SystemExit("bench_engine: needs a GPU")
        return bench_u8([args.shape] if args.shape else ["224", "c2"], args.path, args.batches, args.warmup, args.repeats)
    if args.stacks:
        if not torch.cuda.is_available():
            raise SystemExit("bench_engine: needs a GPU")
        return bench_stacks(args.stacks, args.warmup, args.repeats)
    if args.shape:
        if not torch.cuda.is_available():
            raise SystemExit("bench_engine: needs a GPU")
        return bench_paths(args.shape, args.path, args.batches, args.warmup, args.repeats, args.extras)
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 1024, 128, 32, num_classes=10)
    res = {"model": "C2 architecture (800 -> 1024/128/32 -> 10), 32x32 images"}
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "m.nnue"
        serialize.serialize_model(model, path)
        engine = EngineModel.load(path)
        images = torch.randn(4096, 3, 32, 32).cuda()
        for b in (512, 4096):
            x = images[:b]
            for _ in range(3):
                engine.evaluate_logits(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 20
            for _ in range(n):
                engine.evaluate_logits(x)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            res[f"gpu_batch{b}_ms"] = dt * 1e3
            res[f"gpu_batch{b}_images_per_s"] = b / dt
        exe = ROOT / "oracle" / "_ref" / "nnue_inference"
        if exe.exists():
            img = Path(tmp) / "img.bin"
            images[0].cpu().numpy().tofile(img)
            subprocess.run([str(exe), str(path), str(img), "32", "32"], capture_output=True)
            t0 = time.perf_counter()
            n = 30
            for _ in range(n):
                subprocess.run([str(exe), str(path), str(img), "32", "32"], capture_output=True, text=True, timeout=10)
            dt = (time.perf_counter() - t0) / n
            res["reference_subprocess_ms_per_image"] = dt * 1e3
            res["reference_subprocess_images_per_s"] = 1.0 / dt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
