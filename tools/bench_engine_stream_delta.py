"""Sparse add / remove updates of the engine's streams (EngineStream.update) against the two ways to hand over the same step as a
whole state: EngineStream.step_features on the new [S, F] map, and EngineModel.evaluate_features (the int8 matrix form) on it.

One process, S = 1024 streams, two shapes: the C2 engine architecture (F = 800, L1 = 1024) and (g=32, fps=64: F = 65 536, L1 = 512).
Every stream starts with half its features on (seeded).  A step flips k features per stream -- (k + 1) // 2 that were off are
added, k // 2 that were on are removed -- for k in {1, 16, 0.25 % of F, 1 % of F, 10 % of F}.  The step's two id lists (device CSR)
and its new map are made on the device outside the timed region; then the three variants run on the same step, alternated, each
between two device events, after warm-up steps of the same k.  The update stream and the step_features stream hold the same sets
throughout, and the three variants' logits are compared at every step (the run aborts if they ever differ).
Reported per (shape, k): median ms per call and the 10th / 90th percentiles, the two ratios, and per shape the smallest measured k
from which update no longer wins against each of the other two (null = it won at every measured k).
Prints one JSON object:  python tools/bench_engine_stream_delta.py > profiles/engine_stream_delta.json"""
import argparse
import contextlib
import json
import statistics
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))

import nnue  # noqa: E402
import serialize  # noqa: E402
from nnue_hip.engine import EngineModel  # noqa: E402

SHAPES = [
    {"name": "c2_32x32", "g": 10, "fps": 8, "l1": 1024, "l2": 128, "l3": 32, "classes": 10, "size": 32},
    {"name": "224x224", "g": 32, "fps": 64, "l1": 512, "l2": 32, "l3": 32, "classes": 10, "size": 224},
]
FRACTIONS = (0.0025, 0.01, 0.1)
VARIANTS = ("update", "step_features", "matrix")


def flip_counts(F):
    return sorted({1, 16} | {max(1, round(F * f)) for f in FRACTIONS})


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    return out, (t0, t1)


def _stats(pairs):
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return {"ms": statistics.median(ms), "p10": ms[len(ms) // 10], "p90": ms[len(ms) - 1 - len(ms) // 10]}


def _delta(on: torch.Tensor, k: int, gen: torch.Generator):
    """k flips per stream of the bool map `on` [S, F], applied to it in place: ((added ids, offsets), (removed ids, offsets)) as
    int32 device CSR, the ids of a stream in random order."""
    s = on.shape[0]
    keys = torch.rand(on.shape, device=on.device, generator=gen)
    lists = []
    for n, pool, value in (((k + 1) // 2, ~on, True), (k // 2, on.clone(), False)):
        if n:
            ids = torch.topk(torch.where(pool, keys, torch.full_like(keys, 2.0)), n, dim=1, largest=False, sorted=True).indices
            assert bool(pool.gather(1, ids).all()), "a stream has fewer than k / 2 features to flip"
            on.scatter_(1, ids, value)
        else:
            ids = torch.zeros((s, 0), dtype=torch.int64, device=on.device)
        offsets = torch.arange(s + 1, dtype=torch.int32, device=on.device) * n
        lists.append((ids.reshape(-1).to(torch.int32), offsets))
    return lists


def bench_shape(shape, S, warmup, repeats, seed):
    torch.manual_seed(seed)
    model = nnue.NNUE(nnue.GridFeatureSet(shape["g"], shape["fps"]), shape["l1"], shape["l2"], shape["l3"],
                      num_classes=shape["classes"], input_size=shape["size"])
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "m.nnue"
        with contextlib.redirect_stdout(sys.stderr):  # keep stdout to the one JSON line
            serialize.serialize_model(model, path)
        engine = EngineModel.load(path)
    F = int(engine.header["num_features"])
    engine.prepare_matrix()
    gen = torch.Generator(device="cuda").manual_seed(seed + F)
    on = torch.rand((S, F), device="cuda", generator=gen) < 0.5
    by_update, by_map = engine.stream(S), engine.stream(S)
    by_update.step_features(on)
    by_map.step_features(on)
    for k in flip_counts(F):
        times = {v: [] for v in VARIANTS}
        for t in range(warmup + repeats):
            (added, removed) = _delta(on, k, gen)
            active = on.to(torch.uint8)
            calls = {"update": lambda: by_update.update(added, removed), "step_features": lambda: by_map.step_features(active),
                     "matrix": lambda: engine.evaluate_features(active)}
            order = VARIANTS[t % 3:] + VARIANTS[:t % 3]  # alternated: every variant takes every place in turn
            torch.cuda.synchronize()
            outs = {}
            for v in order:
                outs[v], pair = _timed(calls[v])
                if t >= warmup:
                    times[v].append(pair)
            if not (torch.equal(outs["update"][0], outs["matrix"][0]) and torch.equal(outs["step_features"][0], outs["matrix"][0])
                    and torch.equal(outs["update"][2], outs["step_features"][2]) and int(outs["update"][2].min()) == k):
                raise SystemExit(f"bench_engine_stream_delta: the variants disagree at {shape['name']} k={k} step {t}")
        st = {v: _stats(times[v]) for v in VARIANTS}
        row = {"shape": shape["name"], "S": S, "F": F, "L1": shape["l1"], "k": k, "flip_fraction": k / F}
        for v in VARIANTS:
            row.update({f"{v}_ms": st[v]["ms"], f"{v}_p10": st[v]["p10"], f"{v}_p90": st[v]["p90"]})
        row["update_over_step_features"] = st["update"]["ms"] / st["step_features"]["ms"]
        row["update_over_matrix"] = st["update"]["ms"] / st["matrix"]["ms"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--shapes", default=",".join(s["name"] for s in SHAPES))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_engine_stream_delta: needs a GPU")
    wanted = set(args.shapes.split(","))
    res = {"device": torch.cuda.get_device_name(0), "S": args.streams, "warmup": args.warmup, "repeats": args.repeats,
           "timing": "median of per-call device-event times, the three variants alternated on the same step", "cases": [],
           "update_stops_winning_at_k": {}}
    for shape in SHAPES:
        if shape["name"] not in wanted:
            continue
        rows = bench_shape(shape, args.streams, args.warmup, args.repeats, args.seed)
        res["cases"] += rows
        res["update_stops_winning_at_k"][shape["name"]] = {
            other: next((r["k"] for r in rows if r[f"update_over_{other}"] >= 1.0), None) for other in ("step_features", "matrix")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
