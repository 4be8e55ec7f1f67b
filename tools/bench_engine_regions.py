"""The engine's stream step from dirty rectangles (EngineStream.step_u8_regions) against the two calls it joins: the whole-frame
EngineStream.step_u8(layout="hwc") on the same frames, and EngineStream.update fed the TRUE flip lists of the step -- the floor,
which no caller holding only a frame can reach.

One process, S = 1024 streams, two shapes: the C2 engine architecture at 32 x 32 (F = 800, L1 = 1024; stride 4, 8 x 8 cells)
and (g=32, fps=64) at 224 x 224 (F = 65 536, L1 = 512; stride 8, 28 x 28 cells).  The sequence is video-like: every step redraws
one square patch of random bytes per stream at a random place inside the frame, and hands that patch over as the stream's one
rectangle.  The patch side sweeps from one pixel to the whole frame, so the touched share of cells spans what the shape allows
(one cell of 64 is 1.6 % at 32 x 32; about 0.1 % to 100 % at 224 x 224).  The step's true added / removed id lists (device CSR)
are formed outside the timed region from the conv bytes of an untimed whole-frame evaluation.  Then the three variants run on
the same step, alternated so that every variant takes every place in turn, each between two device events, after warm-up steps
of the same side.  The three streams hold the same sets throughout and their logits and `changed` are compared at every step
(the run aborts if they ever differ).
Reported per (shape, side): the mean touched share of cells, the mean flips per stream, median ms per call with the 10th / 90th
percentiles, the two ratios; and per shape the smallest measured share from which the region step no longer wins against step_u8
(null = it won at every measured side).
Prints one JSON object:  python tools/bench_engine_regions.py > profiles/engine_regions.json"""
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
    {"name": "c2_32x32", "g": 10, "fps": 8, "l1": 1024, "l2": 128, "l3": 32, "classes": 10, "size": 32, "sides": (1, 4, 8, 16, 32)},
    {"name": "224x224", "g": 32, "fps": 64, "l1": 512, "l2": 32, "l3": 32, "classes": 10, "size": 224,
     "sides": (1, 8, 24, 56, 112, 160, 224)},
]
VARIANTS = ("regions", "step_u8", "update")


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


def _redraw(frames: torch.Tensor, side: int, gen: torch.Generator) -> torch.Tensor:
    """One side x side patch of random bytes per frame of [S, H, W, 3], in place; returns the patches as int32 [S, 4] rectangles."""
    s, h, w, _ = frames.shape
    dev = frames.device
    y0 = torch.randint(0, h - side + 1, (s,), device=dev, generator=gen)
    x0 = torch.randint(0, w - side + 1, (s,), device=dev, generator=gen)
    span = torch.arange(side, device=dev)
    rows, cols = (y0[:, None] + span)[:, :, None], (x0[:, None] + span)[:, None, :]
    patch = torch.randint(0, 256, (s, side, side, 3), device=dev, generator=gen, dtype=torch.uint8)
    frames[torch.arange(s, device=dev)[:, None, None], rows, cols] = patch
    return torch.stack((y0, x0, y0 + side, x0 + side), dim=1).to(torch.int32)


def _touched_share(rects: torch.Tensor, stride: int, oh: int, ow: int) -> float:
    """Mean share of the grid's cells whose 3 x 3 window meets the stream's rectangle (the definition in include/nnue_hip.h)."""
    def cells(p0, p1, n):
        lo = torch.where(p0 <= 1, torch.zeros_like(p0), (p0 - 1 + stride - 1) // stride)
        hi = torch.clamp(p1 // stride, max=n - 1)
        return torch.clamp(hi - lo + 1, min=0)
    r = rects.long()
    return float((cells(r[:, 0], r[:, 2], oh) * cells(r[:, 1], r[:, 3], ow)).double().mean()) / (oh * ow)


def _sets(engine: EngineModel, frames: torch.Tensor) -> torch.Tensor:
    """The active sets of whole frames, bool [S, F], from the conv bytes an (untimed) whole-frame evaluation leaves in the scratch."""
    s, f, oc = frames.shape[0], int(engine.header["num_features"]), int(engine._c.oc)
    engine.evaluate_logits_u8(frames, layout="hwc", path="gather")
    conv = engine._scratch[:s * f].view(torch.int8).view(s, f)
    channel = torch.arange(f, device=frames.device) % oc
    return (conv.float() > float(engine._c.threshold)) & (channel < 64)[None, :]


def _csr(mask: torch.Tensor):
    ids = mask.nonzero()  # row-major: the ids of a stream are consecutive
    offsets = torch.zeros(mask.shape[0] + 1, dtype=torch.int32, device=mask.device)
    offsets[1:] = mask.sum(dim=1).cumsum(0)
    return ids[:, 1].to(torch.int32).contiguous(), offsets


def bench_shape(shape, S, warmup, repeats, seed):
    torch.manual_seed(seed)
    model = nnue.NNUE(nnue.GridFeatureSet(shape["g"], shape["fps"]), shape["l1"], shape["l2"], shape["l3"],
                      num_classes=shape["classes"], input_size=shape["size"])
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "m.nnue"
        with contextlib.redirect_stdout(sys.stderr):  # keep stdout to the one JSON line
            serialize.serialize_model(model, path)
        engine = EngineModel.load(path)
    F, size, g = int(engine.header["num_features"]), shape["size"], shape["g"]
    stride = max(1, (size - 1 + g - 2) // (g - 1))
    oh = ow = (size - 1) // stride + 1
    gen = torch.Generator(device="cuda").manual_seed(seed + F)
    frames = torch.randint(0, 256, (S, size, size, 3), device="cuda", generator=gen, dtype=torch.uint8)
    streams = {v: engine.stream(S) for v in VARIANTS}
    for st in streams.values():
        st.step_u8(frames, layout="hwc")
    on = _sets(engine, frames)
    rows = []
    for side in shape["sides"]:
        times = {v: [] for v in VARIANTS}
        shares, flips = [], []
        for t in range(warmup + repeats):
            rects = _redraw(frames, side, gen)
            new = _sets(engine, frames)
            added, removed = _csr(new & ~on), _csr(on & ~new)
            shares.append(_touched_share(rects, stride, oh, ow))
            flips.append(float((new ^ on).sum(dim=1).double().mean()))
            on = new
            calls = {"regions": lambda: streams["regions"].step_u8_regions(frames, rects),
                     "step_u8": lambda: streams["step_u8"].step_u8(frames, layout="hwc"),
                     "update": lambda: streams["update"].update(added, removed)}
            order = VARIANTS[t % 3:] + VARIANTS[:t % 3]  # alternated: every variant takes every place in turn
            torch.cuda.synchronize()
            outs = {}
            for v in order:
                outs[v], pair = _timed(calls[v])
                if t >= warmup:
                    times[v].append(pair)
            if not all(torch.equal(outs[v][0], outs["step_u8"][0]) and torch.equal(outs[v][2], outs["step_u8"][2])
                       for v in ("regions", "update")):
                raise SystemExit(f"bench_engine_regions: the variants disagree at {shape['name']} side={side} step {t}")
        st = {v: _stats(times[v]) for v in VARIANTS}
        row = {"shape": shape["name"], "S": S, "F": F, "L1": shape["l1"], "cells": oh * ow, "side": side,
               "area_share": side * side / (size * size), "touched_cell_share": statistics.mean(shares),
               "flips_per_stream": statistics.mean(flips)}
        for v in VARIANTS:
            row.update({f"{v}_ms": st[v]["ms"], f"{v}_p10": st[v]["p10"], f"{v}_p90": st[v]["p90"]})
        row["regions_over_step_u8"] = st["regions"]["ms"] / st["step_u8"]["ms"]
        row["regions_over_update"] = st["regions"]["ms"] / st["update"]["ms"]
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
        raise SystemExit("bench_engine_regions: needs a GPU")
    wanted = set(args.shapes.split(","))
    res = {"device": torch.cuda.get_device_name(0), "S": args.streams, "warmup": args.warmup, "repeats": args.repeats,
           "timing": "median of per-call device-event times, the three variants alternated on the same step", "cases": [],
           "regions_stops_winning_against_step_u8_at": {}}
    for shape in SHAPES:
        if shape["name"] not in wanted:
            continue
        rows = bench_shape(shape, args.streams, args.warmup, args.repeats, args.seed)
        res["cases"] += rows
        lost = next((r for r in rows if r["regions_over_step_u8"] >= 1.0), None)
        res["regions_stops_winning_against_step_u8_at"][shape["name"]] = None if lost is None else {
            "side": lost["side"], "area_share": lost["area_share"], "touched_cell_share": lost["touched_cell_share"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
