"""Generates tests/golden/engine_u8.npz: uint8 frames and the printed outputs of the REFERENCE C++ engine on the float buffers
those frames stand for under the two layouts of the u8 engine calls (include/nnue_hip.h: nnue_engine_u8_frames),

    chw  x[i] = norm(u[(i mod HW) * 3 + i div HW], i div HW)     hwc  x[i] = norm(u[i], i mod 3)
    norm(v, c) = ((float32)v - mean255[c]) * inv_std255[c],  mean255 = mean * 255, inv_std255 = 1 / (std * 255) in float32,

with the ImageNet constants.  The buffers are built here, in numpy, from that definition alone; the engine is driven through
`oracle/_ref/engine_driver` exactly as tests/golden/make_golden_engine_shapes.py drives it.

Run in the build container only (needs the reference tree for `make -C oracle`):
    python tests/golden/make_golden_engine_u8.py
The fixture holds data only.  Per case k: `case{k}/frames` uint8 [n, H, W, 3]; per layout L in (chw, hwc): `case{k}/L/logits`
float64 [n, len(stacks), C], `case{k}/L/density` float64 [n] (the printed values, ten decimals), `case{k}/L/ids` int32 +
`case{k}/L/ids_offsets` int64 [n + 1]; `index` is the JSON list of {model, h, w, count, stacks, kinds}: kinds[i] names how
frame i was drawn ("uniform": every byte uniform over 0..255; "dark": 0..39; "bright": 200..255).
A fixture must be able to see a layout bug, so the script asserts for every uniform frame that the two layouts' logits differ
and that both densities lie strictly between 0.02 and 0.95, and for the K = 4 model that its three brightness classes name,
over its cases together, at least three of the four layer stacks by the rule min(K-1, n*K // (F+1)).  A small model's logits are coarse and two layouts
may agree on a frame by chance: a case's frames are drawn again (same generator, at most MAX_DRAWS times) until the condition
holds, and the assertions then run on what is recorded.
"""
import json
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent
sys.path.insert(0, str(GOLDEN))

from make_golden_engine_shapes import EXE, run_engine  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LAYOUTS = ("chw", "hwc")

# (.nnue fixture, H, W, frame kinds, layer stack indices)
U3 = ("uniform",) * 3
CASES = [
    ("nnue_c1arch.nnue", 32, 32, U3, (0,)),
    ("nnue_c1arch.nnue", 32, 20, U3, (0,)),   # a CHW plane boundary inside flat rows (H = 32)
    ("nnue_c1arch.nnue", 33, 17, U3, (0,)),   # none (H = 33)
    ("nnue_c1arch.nnue", 10, 4, U3, (0,)),    # stride 1
    ("nnue_c1arch.nnue", 96, 100, ("uniform",), (0,)),  # stride 11, map 9x10
    ("nnue_c1arch.nnue", 32, 3, U3, (0,)),    # one column
    ("nnue_tiny4x4.nnue", 17, 11, U3, (0,)),
    ("nnue_wide96.nnue", 40, 1, U3, (0,)),
    ("nnue_wide70.nnue", 27, 14, U3, (0,)),
    ("nnue_k4.nnue", 17, 17, ("dark", "dark", "uniform", "uniform", "bright", "bright"), (0, 1, 2, 3)),
    ("nnue_k4.nnue", 17, 22, ("dark", "uniform", "bright"), (0, 1, 2, 3)),
]
RANGES = {"uniform": (0, 256), "dark": (0, 40), "bright": (200, 256)}
MAX_DRAWS = 20


def constants():
    f = np.float32
    return np.asarray(MEAN, dtype=f) * f(255.0), f(1.0) / (np.asarray(STD, dtype=f) * f(255.0))


def floats_of(frames: np.ndarray, layout: str) -> np.ndarray:
    """[n, H, W, 3] uint8 -> [n, 3*H*W] float32, the definition in the module docstring."""
    n, h, w, _ = frames.shape
    hw = h * w
    u = frames.reshape(n, 3 * hw)
    i = np.arange(3 * hw)
    mean255, inv_std255 = constants()
    if layout == "chw":
        src, ch = (i % hw) * 3 + i // hw, i // hw
    else:
        src, ch = i, i % 3
    return ((u[:, src].astype(np.float32) - mean255[ch][None, :]) * inv_std255[ch][None, :]).astype(np.float32)


def main():
    if not EXE.exists():
        sys.exit(f"{EXE} missing: run `make -C oracle` in the build container first")
    rng = np.random.RandomState(7)
    out, index = {}, []
    named = {layout: set() for layout in LAYOUTS}  # the stacks the K = 4 model's frames name by the rule
    for k, (name, h, w, kinds, stacks) in enumerate(CASES):
        for _ in range(MAX_DRAWS):
            frames = np.stack([rng.randint(*RANGES[kind], size=(h, w, 3)).astype(np.uint8) for kind in kinds])
            got = {layout: run_engine(GOLDEN / name, floats_of(frames, layout), h, w, stacks) for layout in LAYOUTS}
            if all(not np.array_equal(got["chw"][0][i], got["hwc"][0][i]) for i, kind in enumerate(kinds) if kind == "uniform"):
                break
        out[f"case{k}/frames"] = frames
        for layout in LAYOUTS:
            logits, density, ids = got[layout]
            out[f"case{k}/{layout}/logits"] = logits
            out[f"case{k}/{layout}/density"] = density
            out[f"case{k}/{layout}/ids"] = np.concatenate(ids).astype(np.int32)
            out[f"case{k}/{layout}/ids_offsets"] = np.concatenate(([0], np.cumsum([a.size for a in ids]))).astype(np.int64)
        for i, kind in enumerate(kinds):
            if kind != "uniform":
                continue
            assert not np.array_equal(got["chw"][0][i], got["hwc"][0][i]), (name, h, w, i, "the layouts give the same logits")
            for layout in LAYOUTS:
                assert 0.02 < got[layout][1][i] < 0.95, (name, h, w, i, layout, got[layout][1][i])
        if len(stacks) > 1:
            features = 256  # nnue_k4: 8 x 8 cells of 4 channels
            for layout in LAYOUTS:  # over the model's cases together
                named[layout] |= {min(len(stacks) - 1, a.size * len(stacks) // (features + 1)) for a in got[layout][2]}
        index.append({"model": name, "h": h, "w": w, "count": len(kinds), "stacks": list(stacks), "kinds": list(kinds)})
        print(name, h, w, "density chw", got["chw"][1].round(3).tolist(), "hwc", got["hwc"][1].round(3).tolist())
    assert all(len(v) >= 3 for v in named.values()), named
    print("nnue_k4 stacks named", named)
    out["index"] = np.array(json.dumps(index))
    path = GOLDEN / "engine_u8.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
