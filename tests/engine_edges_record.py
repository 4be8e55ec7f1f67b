"""Reader of tests/golden/engine_edges.npz (tests/golden/make_golden_engine_edges.py has the layout) for the two test files
that use it: the models' bytes written into a directory of the caller's, the recorded cases as plain numpy."""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # the constants of lib.load_batch


def floats_of(frames: np.ndarray, layout: str) -> np.ndarray:
    """[n, H, W, 3] uint8 -> [n, 3*H*W] float32, the buffers a uint8 case was recorded on (include/nnue_hip.h,
    nnue_engine_u8_frames):  chw  x[i] = norm(u[(i mod HW) * 3 + i div HW], i div HW),  hwc  x[i] = norm(u[i], i mod 3),
    norm(v, c) = ((float32)v - mean255[c]) * inv_std255[c].  The one definition for this fixture: the generator records with it
    (and asserts it equal to the one engine_u8.npz was recorded with), the tests read with it."""
    f = np.float32
    n, h, w, _ = frames.shape
    hw = h * w
    mean255, inv_std255 = np.asarray(MEAN, dtype=f) * f(255.0), f(1.0) / (np.asarray(STD, dtype=f) * f(255.0))
    i = np.arange(3 * hw)
    src, ch = ((i % hw) * 3 + i // hw, i // hw) if layout == "chw" else (i, i % 3)
    return ((frames.reshape(n, 3 * hw)[:, src].astype(f) - mean255[ch][None, :]) * inv_std255[ch][None, :]).astype(f)


class Case:
    """One recorded (model, H x W) pair: `images` float32 [n, 3*H*W] (of a uint8 case: what its `frames` stand for under
    `layout`), `logits` uint32 [n, len(stacks), C], `density` uint32 [n] (float32 bit patterns), `ids` per image."""

    def __init__(self, z, k, c):
        self.model, self.h, self.w, self.count = c["model"], c["h"], c["w"], c["count"]
        self.stacks, self.layout = c["stacks"], c["layout"]
        self.frames = z[f"case{k}/frames"] if self.layout else None
        self.images = floats_of(self.frames, self.layout) if self.layout else z[f"images/{self.h}x{self.w}"]
        self.logits, self.density = z[f"case{k}/logits"], z[f"case{k}/density"]
        off = z[f"case{k}/ids_offsets"]
        self.ids = [z[f"case{k}/ids"][off[i]:off[i + 1]].astype(np.int64) for i in range(self.count)]
        assert self.images.shape == (self.count, 3 * self.h * self.w) and self.logits.dtype == np.uint32

    def __repr__(self):
        return f"{self.model} {self.h}x{self.w}" + (f" {self.layout}" if self.layout else "")


def load(directory):
    """(model name -> path of its `.nnue` file under `directory`, the recorded cases in the fixture's order)."""
    with np.load(GOLDEN / "engine_edges.npz") as z:
        paths = {}
        for key in z.files:
            if key.startswith("model/"):
                paths[key[6:]] = Path(directory) / f"{key[6:]}.nnue"
                paths[key[6:]].write_bytes(z[key].tobytes())
        cases = [Case(z, k, c) for k, c in enumerate(json.loads(str(z["index"])))]
    assert {c.model for c in cases} == set(paths)
    return paths, cases
