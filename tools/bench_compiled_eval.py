"""From live parameters to compiled metrics: the on-device quantisation (EngineModel.requantize, one launch of
nnue_engine_quantize_model) beside the file round trip it replaces (serialize_model + EngineModel.load), and
evaluate.evaluate_engine beside evaluate.evaluate_compiled_model, all in one process.

  (a) live parameters -> usable engine, at the CIFAR parameter set (10x10x8, 1024/128/32, 10 classes: 0.96 M elements) and the
      224x224 one (32x32x64, 1024/128/32, 1000 classes: 67.3 M).  The launch is timed by device events (warm-up, median of the
      repeats); the whole requantize call (scalars, launch, the counter's read-back) and the file round trip on the host clock
      with a synchronise.  For the launch: bytes moved (4 read + 2 written per table element) over its time, as a share of the
      bandwidth the project takes as achievable.
  (b) 10 000 CIFAR-shape images at batch 512, resident on the device: evaluate_engine (and requantize + evaluate_engine, what an
      epoch costs) against evaluate_compiled_model (which serialises, loads and synchronises twice per batch).

    python tools/bench_compiled_eval.py            # writes profiles/compiled_eval.json
"""
import argparse
import contextlib
import copy
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))

import evaluate  # noqa: E402
import nnue  # noqa: E402
import serialize  # noqa: E402
from nnue_hip import lib  # noqa: E402
from nnue_hip.engine import EngineModel  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0  # what tools/bench_optim.py measures the optimizer against (profiles/optim_step.json)
SHAPES = [
    {"name": "cifar_32x32", "g": 10, "fps": 8, "l1": 1024, "l2": 128, "l3": 32, "classes": 10, "size": 32},
    {"name": "224x224", "g": 32, "fps": 64, "l1": 1024, "l2": 128, "l3": 32, "classes": 1000, "size": 224},
]


def build(shape):
    torch.manual_seed(0)
    return nnue.NNUE(nnue.GridFeatureSet(shape["g"], shape["fps"]), shape["l1"], shape["l2"], shape["l3"],
                     num_classes=shape["classes"], input_size=shape["size"]).cuda()


def wall_ms(fn, warmup, repeats):
    """Median host-clock time of fn() with the device drained before and after."""
    times = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def round_trip(model, tmp):
    path = Path(tmp) / "m.nnue"
    with contextlib.redirect_stdout(sys.stderr):
        serialize.serialize_model(model, path)
    return EngineModel.load(path)


def bench_quantize(shape, warmup, repeats, file_repeats):
    model = build(shape)
    engine = EngineModel.from_model(model)
    timers = {"nnue_engine_quantize_model": []}
    for _ in range(warmup):
        engine.requantize(model, check=False)
    with lib.time_calls(timers):
        for _ in range(repeats):
            engine.requantize(model, check=False)
    torch.cuda.synchronize()
    launch_ms = statistics.median(a.elapsed_time(b) for a, b in timers["nnue_engine_quantize_model"])
    call_ms = wall_ms(lambda: engine.requantize(model), warmup, repeats)
    clamped = copy.deepcopy(model)  # serialize_model clamps and flips the model it is given
    with tempfile.TemporaryDirectory() as tmp:
        file_ms = wall_ms(lambda: round_trip(clamped, tmp), 1, file_repeats)
        loaded = round_trip(clamped, tmp)
    assert all(torch.equal(engine.tensors[k], t) for k, t in loaded.tensors.items()) and engine.header == loaded.header
    table = model.input.weight.numel()
    row = {"shape": shape["name"], "elements": sum(p.numel() for n, p in model.named_parameters() if n not in ("nnue2score", "visual_threshold")),
           "table_elements": table, "quantize_launch_ms": launch_ms, "requantize_call_ms": call_ms, "file_round_trip_ms": file_ms,
           "file_over_requantize_call": file_ms / call_ms, "table_bytes_moved": 6 * table,
           "launch_gbs": 6 * table / launch_ms / 1e6}
    row["launch_hbm_achievable_share"] = row["launch_gbs"] / HBM_ACHIEVABLE_GBS
    return row


def bench_loop(images, batch, warmup, repeats):
    shape = SHAPES[0]
    model = build(shape)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(images, 3, shape["size"], shape["size"], device="cuda", generator=gen)
    y = torch.randint(0, shape["classes"], (images,), device="cuda", generator=gen)
    loader = [(x[i:i + batch], y[i:i + batch]) for i in range(0, images, batch)]
    engine = EngineModel.from_model(model)
    clamped = copy.deepcopy(model)

    def ours_epoch():
        engine.requantize(model)
        return evaluate.evaluate_engine(engine, loader)

    def theirs():
        with contextlib.redirect_stdout(sys.stderr):
            return evaluate.evaluate_compiled_model(clamped, loader, "nnue")

    engine.requantize(clamped)  # the same weights on both sides for the comparison of the metrics
    got, want = evaluate.evaluate_engine(engine, loader), theirs()
    assert all(got[k] == want[k] for k in ("acc", "f1", "precision", "recall"))
    row = {"shape": shape["name"], "images": images, "batch": batch, "batches": len(loader),
           "evaluate_engine_ms": wall_ms(lambda: evaluate.evaluate_engine(engine, loader), warmup, repeats),
           "requantize_plus_evaluate_engine_ms": wall_ms(ours_epoch, warmup, repeats),
           "evaluate_compiled_model_ms": wall_ms(theirs, warmup, repeats),
           "engine_ms_per_sample": got["ms_per_sample"], "compiled_model_ms_per_sample": want["ms_per_sample"]}
    row["compiled_model_over_engine"] = row["evaluate_compiled_model_ms"] / row["evaluate_engine_ms"]
    row["compiled_model_over_epoch"] = row["evaluate_compiled_model_ms"] / row["requantize_plus_evaluate_engine_ms"]
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "compiled_eval.json")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--file-repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compiled_eval: needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup, "repeats": args.repeats,
           "hbm_achievable_gbs": HBM_ACHIEVABLE_GBS,
           "timing": "quantize_launch_ms: median of device-event pairs around the C call; every other time: median host clock with a "
                     "synchronise before and after", "quantize": [], "loop": None}
    optim = ROOT / "profiles" / "optim_step.json"
    if optim.exists():
        res["multi_sgd_step_224_hbm_achievable_share"] = json.loads(optim.read_text())["optimizer_step"]["c4_sgd"]["ours_hbm_achievable_share"]
    for shape in SHAPES:
        row = bench_quantize(shape, args.warmup, args.repeats, args.file_repeats)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["quantize"].append(row)
        torch.cuda.empty_cache()
    res["loop"] = bench_loop(args.images, args.batch, 2, 7)
    print(json.dumps(res["loop"]), file=sys.stderr, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
