"""Incremental per-stream engine evaluation (EngineModel.stream) against the batched engine (evaluate_logits) on the GPU.

Two shapes: the C2 engine architecture (800 -> 1024/128/32 -> 10) at 32x32 and (g=32, fps=64, L1=512, 32, 32, 10) at
224x224; S in {1, 64, 1024} streams.  Sequence kinds:
  (a) step_features on [S, F] maps (half the features on) where each step flips a controlled fraction of the features;
      beside it the same maps evaluated from scratch (a second stream, reset before every step; `from_scratch_ms`) and,
      for scale, evaluate_logits on the patch frames of (b) (`eval_ms`);
  (b) step(frames) where frame t+1 is frame t with one random patch per stream re-randomised (4x4 pixels at 32x32,
      16x16 at 224x224), and evaluate_logits on the same frames; `changed_fraction` is measured (changed / F);
  (c) step(frames) on unrelated random frames every step (the incremental path's worst case), and evaluate_logits on
      the same frames.
Times: median ms per step over device-event-timed repeats after warm-up.  Inputs are generated on the host, outside the
timed region.  Prints one JSON object:  python tools/bench_engine_stream.py > profiles/engine_stream.json"""
import argparse
import contextlib
import json
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))

import nnue  # noqa: E402
import serialize  # noqa: E402
from nnue_hip.engine import EngineModel  # noqa: E402

SHAPES = [
    {"name": "c2_32x32", "g": 10, "fps": 8, "l1": 1024, "l2": 128, "l3": 32, "classes": 10, "size": 32, "patch": 4},
    {"name": "224x224", "g": 32, "fps": 64, "l1": 512, "l2": 32, "l3": 32, "classes": 10, "size": 224, "patch": 16},
]
FLIP_RATES = (0.0, 0.001, 0.01, 0.1, 1.0)


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    return out, (t0, t1)


def _median_ms(pairs):
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs)


def _patch_(frames: torch.Tensor, rng: np.random.Generator, p: int) -> None:
    """Re-randomises one p x p patch per frame, at its own place (index_put of host-made noise)."""
    s, _, h, w = frames.shape
    ys, xs = rng.integers(0, h - p + 1, s), rng.integers(0, w - p + 1, s)
    si = np.arange(s)[:, None, None, None]
    ci = np.arange(3)[None, :, None, None]
    yi = (ys[:, None, None, None] + np.arange(p)[None, None, :, None])
    xi = (xs[:, None, None, None] + np.arange(p)[None, None, None, :])
    shape = (s, 3, p, p)
    idx = tuple(torch.from_numpy(np.broadcast_to(a, shape).copy()).to(frames.device) for a in (si, ci, yi, xi))
    noise = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(frames.device)
    frames.index_put_(idx, noise)


def bench_shape(shape, streams, warmup, repeats, seed):
    torch.manual_seed(seed)
    size, p = shape["size"], shape["patch"]
    model = nnue.NNUE(nnue.GridFeatureSet(shape["g"], shape["fps"]), shape["l1"], shape["l2"], shape["l3"],
                      num_classes=shape["classes"], input_size=size)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "m.nnue"
        with contextlib.redirect_stdout(sys.stderr):  # keep stdout to the one JSON line
            serialize.serialize_model(model, path)
        engine = EngineModel.load(path)
        F = int(engine.header["num_features"])
        for S in streams:
            rng = np.random.default_rng(seed + S)
            base = {"shape": shape["name"], "S": S, "F": F, "L1": shape["l1"]}
            # (b) patch sequences through the conv
            frames = torch.from_numpy(rng.standard_normal((S, 3, size, size), dtype=np.float32)).cuda()
            stream = engine.stream(S)
            step_t, eval_t, changed = [], [], []
            for t in range(warmup + repeats):
                if t:
                    _patch_(frames, rng, p)
                (_, _, ch), ts = _timed(lambda: stream.step(frames))
                _, te = _timed(lambda: engine.evaluate_logits(frames))
                if t >= warmup:
                    step_t.append(ts)
                    eval_t.append(te)
                    changed.append(ch.cpu().numpy())
            step_ms, eval_ms = _median_ms(step_t), _median_ms(eval_t)
            rows.append(dict(base, kind="frames_patch", patch=p, changed_fraction=float(np.mean(changed)) / F,
                             step_ms=step_ms, frames_per_s=S / step_ms * 1e3, eval_ms=eval_ms,
                             eval_frames_per_s=S / eval_ms * 1e3, step_over_eval=step_ms / eval_ms))
            eval_ref_ms = eval_ms
            # (c) unrelated frames every step
            step_t, eval_t, changed = [], [], []
            for t in range(warmup + repeats):
                frames.copy_(torch.from_numpy(rng.standard_normal((S, 3, size, size), dtype=np.float32)))
                (_, _, ch), ts = _timed(lambda: stream.step(frames))
                _, te = _timed(lambda: engine.evaluate_logits(frames))
                if t >= warmup:
                    step_t.append(ts)
                    eval_t.append(te)
                    changed.append(ch.cpu().numpy())
            step_ms, eval_ms = _median_ms(step_t), _median_ms(eval_t)
            rows.append(dict(base, kind="frames_new", changed_fraction=float(np.mean(changed)) / F,
                             step_ms=step_ms, frames_per_s=S / step_ms * 1e3, eval_ms=eval_ms,
                             eval_frames_per_s=S / eval_ms * 1e3, step_over_eval=step_ms / eval_ms))
            del frames
            # (a) feature maps with controlled flip rates
            for rate in FLIP_RATES:
                maps = rng.random((S, F), dtype=np.float32) < 0.5
                stream = engine.stream(S)
                step_t, fresh_t, changed = [], [], []
                scratch_stream = engine.stream(S)
                for t in range(warmup + repeats):
                    if t:
                        maps ^= rng.random((S, F), dtype=np.float32) < rate
                    active = torch.from_numpy(maps).cuda()
                    (_, _, ch), ts = _timed(lambda: stream.step_features(active))
                    scratch_stream.reset()
                    _, tf = _timed(lambda: scratch_stream.step_features(active))
                    if t >= warmup:
                        step_t.append(ts)
                        fresh_t.append(tf)
                        changed.append(ch.cpu().numpy())
                step_ms, fresh_ms = _median_ms(step_t), _median_ms(fresh_t)
                rows.append(dict(base, kind="features_flip", flip_rate=rate, changed_fraction=float(np.mean(changed)) / F,
                                 step_ms=step_ms, frames_per_s=S / step_ms * 1e3, from_scratch_ms=fresh_ms,
                                 step_over_from_scratch=step_ms / fresh_ms, eval_ms=eval_ref_ms,
                                 eval_frames_per_s=S / eval_ref_ms * 1e3, step_over_eval=step_ms / eval_ref_ms))
            print(json.dumps(rows[-1]), file=sys.stderr)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", default="1,64,1024")
    ap.add_argument("--shapes", default=",".join(s["name"] for s in SHAPES))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_engine_stream: needs a GPU")
    streams = [int(s) for s in args.streams.split(",")]
    wanted = set(args.shapes.split(","))
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
           "timing": "median of per-step device-event times", "cases": []}
    for shape in SHAPES:
        if shape["name"] in wanted:
            res["cases"] += bench_shape(shape, streams, args.warmup, args.repeats, args.seed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
