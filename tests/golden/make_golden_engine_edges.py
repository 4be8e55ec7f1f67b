"""Generates tests/golden/engine_edges.npz: inputs and outputs of the REFERENCE C++ engine on models whose header values and
integers leave what serialize.py writes (every scale 64.0, quantized_one 127.0): scales that are no power of two and have a
fractional part (the engine truncates two of its four scales to int before dividing and divides by the other two as floats),
quantized_one of 255, 20.9, 0 and -200 (the clipped ReLU is max(0, min(v, (int16)q1)): 0 everywhere for a negative q1),
thresholds a conv byte can equal (the comparison is strict) or never pass, fractional conv scales under thresholds inside the
byte range (so that the truncated divisor shows in the ids), a table whose int16 sums wrap on most columns,
int32 biases that push the layer-1 and output sums past 2^24 (where their conversion to float rounds), and a K = 3 file whose
three layer stacks differ in weights and in all three scales.  tests/test_engine_edges_oracle.py counts, from the oracle's
intermediates, how often the recorded evaluations reach each of these edges.

The engine is driven through `oracle/_ref/engine_driver --bits` (oracle/engine_driver.cpp: this repo's own main() over the
reference's sources, compiled by oracle/Makefile where they lie), which prints every logit and the density as the float32
bit pattern: ten decimals are not exact for a quotient by 3.0 or 0.1.

Run in the build container only (needs the reference tree for `make -C oracle`):
    python tests/golden/make_golden_engine_edges.py
The models exist only inside the fixture (nnue_index.json is not touched).  The base model is a seeded `nnue.NNUE` written by
this repo's serialize.py -- grid 4, 8 channels per cell, L1 = 48, L2 = 6, L3 = 5, 3 classes, input size 32, the table
multiplied by 3, the bias uniform in (-1, 1): the smallest sizes at which both the wave-per-output loop (step 4) and the lane
loop (step 64) of the GPU tail have ragged ends -- read back with oracle.load_nnue, its first two classifier layers' integer
weights multiplied by 3 (base_model says why), edited field by field (VARIANTS) and
written with `write_nnue`, the inverse of load_nnue, which this script first proves on nnue_tiny4x4.nnue byte for byte.  The
K = 3 model is the same recipe with three layer stacks.
The fixture holds data only.  `model/{name}` uint8: the bytes of the `.nnue` file.  `images/{H}x{W}` float32 [n, 3*H*W]: the
flat buffers handed to the engine, the same for every model.  Per case k: `case{k}/logits` uint32 [n, len(stacks), C] and
`case{k}/density` uint32 [n] (float32 bit patterns), `case{k}/ids` int32 + `case{k}/ids_offsets` int64 [n + 1] (the ascending
active-feature ids of image i are ids[offsets[i]:offsets[i + 1]]); a uint8 case has `case{k}/frames` uint8 [n, H, W, 3] and
was recorded on the float buffers those frames stand for under its layout (tests/engine_edges_record.floats_of: the expression
of lib.load_batch, asserted equal here to make_golden_engine_u8.floats_of), not on `images/`.  `index` is the JSON list of
{model, h, w, count, stacks, layout}: stacks[j] is the layer stack index the engine was called with for logits[:, j], layout
None, "chw" or "hwc".  Every int32 sum of every recorded
evaluation stays inside int32 (asserted here from the oracle's intermediates: overflow is undefined in the engine).
"""
import copy
import json
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent
ROOT = GOLDEN.parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(GOLDEN.parent))

import nnue  # noqa: E402
import nnue_engine_oracle as eo  # noqa: E402
import serialize  # noqa: E402
from make_golden_engine_shapes import EXE  # noqa: E402
from engine_edges_record import floats_of  # noqa: E402  (the one definition the tests of this fixture read it with)
from make_golden_engine_u8 import floats_of as recorded_floats_of  # noqa: E402  (what engine_u8.npz was recorded with)

# grid, channels per cell, L1, L2, L3, classes, input size, seed
BASE = (4, 8, 48, 6, 5, 3, 32, 4806)
K3_SCALES = ((37.5, 100.7, 3.0), (0.3, 1.9, 0.1), (64.0, 64.0, 64.0))  # (l1_scale, l2_scale, out_scale) per stack
SIZES = ((32, 32, (0.3, 1.0, 1.0, 1.5, 3.0, 3.0)), (32, 20, (1.0, 2.0)))  # H, W, randn times these


def write_nnue(m, path) -> None:
    """The inverse of oracle.load_nnue: the version-2 container (serialize.py has the layout) from the dict it returns."""
    def dense(w, b):
        return struct.pack("<2I", *w.shape) + w.astype("i1").tobytes() + struct.pack("<I", b.size) + b.astype("<i4").tobytes()

    out = [b"NNUE", struct.pack("<6I", 2, m["num_features"], m["l1"], m["l2"], m["l3"], len(m["stacks"])),
           struct.pack("<3f", m["nnue2score"], m["quantized_one"], m["threshold"]),
           struct.pack("<If4I", 0, m["conv_scale"], m["oc"], 3, 3, 3), m["conv_w"].astype("i1").tobytes(),
           struct.pack("<I", m["conv_b"].size), m["conv_b"].astype("<i4").tobytes(),
           struct.pack("<f2I", m["ft_scale"], *m["ft_w"].shape), m["ft_w"].astype("<i2").tobytes(),
           struct.pack("<I", m["ft_b"].size), m["ft_b"].astype("<i4").tobytes()]
    for s in m["stacks"]:
        out.append(struct.pack("<4f", s["l1_scale"], s["l2_scale"], s["out_scale"], s["l1_fact_scale"]))
        out += [dense(s["l1_w"], s["l1_b"]), dense(s["l1_fact_w"], s["l1_fact_b"]), dense(s["l2_w"], s["l2_b"]),
                dense(s["out_w"], s["out_b"])]
    Path(path).write_bytes(b"".join(out))


def base_model(stacks: int):
    g, fps, l1, l2, l3, classes, size, seed = BASE
    torch.manual_seed(seed + stacks)
    model = nnue.NNUE(nnue.GridFeatureSet(g, fps), l1, l2, l3, num_classes=classes, input_size=size, num_ls_buckets=stacks)
    with torch.no_grad():
        model.input.weight.mul_(3.0)
        model.input.bias.uniform_(-1, 1)
        model.visual_threshold.fill_(-0.5)  # below zero: cells the conv never produced count as active
    with tempfile.TemporaryDirectory() as d:
        serialize.serialize_model(model, Path(d) / "m.nnue")
        m = eo.load_nnue(Path(d) / "m.nnue")
    # a fresh classifier's integer weights are a few units: three times larger in the first two layers, an accumulator clipped
    # at 20 (or wrongly at -200) still moves the logits, and no recorded edge hides behind a layer that rounds it to zero
    for s in m["stacks"]:
        for key in ("l1_w", "l2_w"):
            s[key] = np.clip(s[key].astype(np.int64) * 3, -127, 127).astype(np.int8)
    return m


def scales(m, conv, l1, l2, out):
    m["conv_scale"] = conv
    m["stacks"][0].update(l1_scale=l1, l2_scale=l2, out_scale=out)


def q255(m, rng):
    m["quantized_one"] = 255.0
    m["ft_w"] = (m["ft_w"] * 2).astype(np.int16)  # the table multiplied by 6: clipped sums above 127 are common


def wrapping(m, rng):
    m["ft_w"] = rng.randint(-3000, 3001, size=m["ft_w"].shape).astype(np.int16)
    m["ft_b"] = rng.randint(-100000, 100001, size=m["ft_b"].shape).astype(np.int32)


def big_biases(m, rng):
    """Layer-1 sums just above 2^24 and output sums around +-2^30: both beyond the 24 bits a float holds.  Layer-1 weights at
    full int8 range and l1_scale = 160500 put the layer-1 outputs at 104..115 and let the image move them by one;
    layer-2 biases that cancel the outputs' common part, l2_scale = 10.7 and output weights four times larger carry one unit
    of a layer-1 output through layer 2 (7 units for a weight of 78) into steps of the logits far above the 64 between
    neighbouring floats below 2^30.  A rounded layer-1 sum changes its quotient only next to a multiple of the scale, where
    no image lands by chance: the last layer-1 output has zero weights, the bias 112 * 160500 - 1 -- an odd number above 2^24
    that rounds up to 112 * 160500, so the engine's float division gives 112 where integer or double arithmetic gives 111,
    and so does a multiplication by the float reciprocal of the scale -- and the layer-2 weight 127 in every row."""
    s, l2 = m["stacks"][0], m["l2"]
    scale, k = 160500.0, 112
    s["l1_w"][:l2] = np.clip(np.round(s["l1_w"][:l2].astype(np.float64) * 4.7), -127, 127).astype(np.int8)
    # a clipped accumulator moves these sums by -10000 .. -70000: biases 20000 .. 50000 above a multiple of the scale let
    # that cross the multiple for about every second image
    n = s["l1_b"].size
    s["l1_b"] = (rng.randint(105, 116, size=n) * int(scale) + rng.randint(20000, 50000, size=n)).astype(np.int32)
    s["l1_w"][l2 - 1] = 0
    s["l1_b"][l2 - 1] = k * int(scale) - 1
    f = np.float32
    assert int(f(s["l1_b"][l2 - 1])) == k * int(scale) and int(f(s["l1_b"][l2 - 1]) / f(scale)) == k
    assert int(f(s["l1_b"][l2 - 1]) * (f(1) / f(scale))) == k - 1
    s["l2_w"][:, l2 - 1] = 127
    nominal = np.trunc(s["l1_b"][:l2].astype(f) / f(scale)).astype(np.int64)  # the layer-1 outputs of an all-zero accumulator
    s["l2_b"] = (rng.randint(-300, 900, size=s["l2_b"].size) - s["l2_w"][:, :l2].astype(np.int64) @ nominal).astype(np.int32)
    sign = np.where(rng.rand(s["out_b"].size) < 0.5, -1, 1)
    s["out_b"] = (sign * (2 ** 30 - rng.randint(0, 2 ** 20, size=s["out_b"].size))).astype(np.int32)
    s["out_w"] = np.clip(s["out_w"].astype(np.int64) * 4, -127, 127).astype(np.int8)
    s.update(l1_scale=scale, l2_scale=10.7, out_scale=7.0)


def conv_edge(conv, threshold):
    """A fractional conv_scale under a threshold inside the byte range: which bytes pass depends on the quotient itself, not
    only on its sign, so the record tells acc / (int)scale from a division by the scale as it stands."""
    def edit(m, rng):
        scales(m, conv, 37.5, 100.7, 3.0)
        m["threshold"] = threshold
    return edit


def k3(m, rng):
    for s, (l1, l2, out) in zip(m["stacks"], K3_SCALES):
        s.update(l1_scale=l1, l2_scale=l2, out_scale=out)
    # a conv bias below zero spreads the active counts of the images over two stacks of the rule min(K-1, n*K // (F+1))
    m["conv_b"] = np.full_like(m["conv_b"], -768)


# name -> (layer stacks of the base, edit(m, rng), layer stack indices recorded)
VARIANTS = {
    "odd_scales": (1, lambda m, rng: scales(m, 50.5, 37.5, 100.7, 3.0), (0,)),
    "small_scales": (1, lambda m, rng: scales(m, 7.0, 0.3, 1.9, 0.1), (0,)),
    "q255": (1, q255, (0,)),
    "q20_9": (1, lambda m, rng: m.update(quantized_one=20.9), (0,)),
    "q0": (1, lambda m, rng: m.update(quantized_one=0.0), (0,)),
    "qneg200": (1, lambda m, rng: m.update(quantized_one=-200.0), (0,)),
    "thr5": (1, lambda m, rng: m.update(threshold=5.0), (0,)),
    "thr_neg127": (1, lambda m, rng: m.update(threshold=-127.0), (0,)),
    "thr_neg200": (1, lambda m, rng: m.update(threshold=-200.0), (0,)),
    "thr126_5": (1, lambda m, rng: m.update(threshold=126.5), (0,)),
    "conv50_5_thr5": (1, conv_edge(50.5, 5.0), (0,)),
    "conv7_9_thr40": (1, conv_edge(7.9, 40.0), (0,)),
    "conv2_7_thr5": (1, conv_edge(2.7, 5.0), (0,)),
    "wrapping": (1, wrapping, (0,)),
    "big_biases": (1, big_biases, (0,)),
    "k3": (3, k3, (0, 1, 2, 3)),  # index 3 = stack 0
}
# model, layout, H, W, frames (every byte uniform over 0..255).  conv_scale = 50.5: the u8 front's 768-entry table truncates
# non-trivially; conv_scale = 2.7 under threshold 5: its division by (int)scale shows in the ids
U8_CASES = (("odd_scales", "chw", 32, 20, 3), ("odd_scales", "hwc", 32, 32, 3),
            ("conv2_7_thr5", "chw", 32, 32, 6), ("conv2_7_thr5", "hwc", 32, 20, 6))


def run_engine_bits(model: Path, images: np.ndarray, h: int, w: int, stacks):
    """make_golden_engine_shapes.run_engine with --bits: (logits uint32 [n, len(stacks), C], density uint32 [n], ids per image)."""
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        images.astype(np.float32).tofile(f.name)
        res = subprocess.run([str(EXE), "--bits", str(model), f.name, str(h), str(w), str(len(images))] + [str(k) for k in stacks],
                             capture_output=True, text=True, timeout=60)
    if res.returncode != 0:
        raise RuntimeError(f"engine failed: {res.stderr}")
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(images) * len(stacks), (len(lines), len(images), stacks)
    logits, density, ids = [], [], []
    for n, line in enumerate(lines):
        head, lg, dn, tail = (part.strip() for part in line.split("|"))
        i, j = divmod(n, len(stacks))
        assert [int(x) for x in head.split()] == [i, stacks[j]], (head, i, j)
        cur = np.array([int(x) for x in tail.split()], dtype=np.int32)
        if j == 0:
            logits.append([])
            density.append(int(dn, 16))
            ids.append(cur)
        assert int(dn, 16) == density[i] and np.array_equal(cur, ids[i])  # the features do not depend on the stack
        logits[i].append([int(x, 16) for x in lg.split(",")])
    return np.array(logits, dtype=np.uint32), np.array(density, dtype=np.uint32), ids


def assert_inside_int32(m, images, h, w, stacks):
    lim = 2 ** 31 - 1
    for image in images:
        acc, _ = eo.conv_accumulate(m, image, h, w)
        assert np.abs(acc).max() <= lim
        ft = eo.ft_forward(m, eo.active_features(m, eo.conv_forward(m, image, h, w)[0]))
        for k in stacks:
            t = eo.stack_trace(m["stacks"][k if k < m["buckets"] else 0], ft, m["l1"], m["l2"], m["l3"])
            assert max(np.abs(t[key]).max() for key in ("acc1", "acc2", "acc3")) <= lim, (k, "int32 overflow")


def main():
    if not EXE.exists():
        sys.exit(f"{EXE} missing: run `make -C oracle` in the build container first")
    with tempfile.TemporaryDirectory() as d:
        tiny = GOLDEN / "nnue_tiny4x4.nnue"
        write_nnue(eo.load_nnue(tiny), Path(d) / "again.nnue")
        assert (Path(d) / "again.nnue").read_bytes() == tiny.read_bytes(), "write_nnue does not invert load_nnue"

    rng = np.random.RandomState(20261019)
    out, index = {}, []
    images = {}
    for h, w, image_scales in SIZES:
        images[h, w] = (rng.randn(len(image_scales), 3 * h * w) * np.asarray(image_scales)[:, None]).astype(np.float32)
        out[f"images/{h}x{w}"] = images[h, w]
    bases = {k: base_model(k) for k in sorted({spec[0] for spec in VARIANTS.values()})}
    with tempfile.TemporaryDirectory() as d:
        def record(name, path, x, h, w, stacks, layout, frames=None):
            k = len(index)
            logits, density, ids = run_engine_bits(path, x, h, w, stacks)
            assert_inside_int32(eo.load_nnue(path), x, h, w, stacks)
            out[f"case{k}/logits"], out[f"case{k}/density"] = logits, density
            out[f"case{k}/ids"] = np.concatenate(ids).astype(np.int32)
            out[f"case{k}/ids_offsets"] = np.concatenate(([0], np.cumsum([a.size for a in ids]))).astype(np.int64)
            if frames is not None:
                out[f"case{k}/frames"] = frames
            index.append({"model": name, "h": h, "w": w, "count": len(x), "stacks": list(stacks), "layout": layout})
            print(name, h, w, layout or "", "ids", [a.size for a in ids], "logits[0] =",
                  logits[0].view(np.float32).round(3).tolist())
            return ids

        for name, (base, edit, stacks) in VARIANTS.items():
            m = copy.deepcopy(bases[base])
            edit(m, rng)
            path = Path(d) / f"{name}.nnue"
            write_nnue(m, path)
            out[f"model/{name}"] = np.frombuffer(path.read_bytes(), dtype=np.uint8)
            counts = []
            for h, w, _ in SIZES:
                counts += [a.size for a in record(name, path, images[h, w], h, w, stacks, None)]
            if base > 1:
                named = {min(base - 1, n * base // (m["num_features"] + 1)) for n in counts}
                assert len(named) >= 2, (name, counts, named)
                print(name, "stacks named by the rule", sorted(named))
        for name, layout, h, w, count in U8_CASES:
            frames = rng.randint(0, 256, size=(count, h, w, 3)).astype(np.uint8)
            assert np.array_equal(floats_of(frames, layout), recorded_floats_of(frames, layout))
            record(name, Path(d) / f"{name}.nnue", floats_of(frames, layout), h, w, VARIANTS[name][2], layout, frames)
    out["index"] = np.array(json.dumps(index))
    path = GOLDEN / "engine_edges.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
