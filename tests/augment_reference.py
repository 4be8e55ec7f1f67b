"""float64 numpy restatement of nnue_load_batch_policy (policy 0 "none" and 2 "medium"; include/nnue_hip.h defines the
stages), written from that definition and albumentations' documented formulas.  A helper for test_augment_reference.py
(which pins it against scipy and colorsys) and test_gpu_augment_policy.py; not a test.

Draws are exact: the generator is integer arithmetic, u01 is a 24-bit fraction.  Decisions that the kernel takes on
float32 values (a draw against its probability, the integer k / kind / direction / hole rectangle) are taken here on the
same float32 values, so both sides decide alike; every continuous quantity is float64."""
import math

import numpy as np

MASK = (1 << 64) - 1
INDEX_MUL = 0xD1342543DE82EF95
NOISE_OFFSET = 1 << 32
PARAMS = 32
F_FLIP, F_ROT90, F_ROTATE, F_AFFINE, F_BC, F_HSV, F_BLUR, F_NOISE, F_DROP = 1, 2, 4, 8, 16, 32, 64, 128, 256
STAGES = {"flip": F_FLIP, "rot90": F_ROT90, "rotate": F_ROTATE, "affine": F_AFFINE, "bc": F_BC, "hsv": F_HSV, "blur": F_BLUR,
          "noise": F_NOISE, "drop": F_DROP}
PROBABILITY = {"flip": .5, "rot90": .5, "rotate": .3, "affine": .3, "bc": .3, "hsv": .3, "blur": .2, "noise": .2, "drop": .3}
# slots of the per-image record
R_FLAGS, R_K, R_ROT, R_AFF_ROT, R_AFF_SCALE, R_TX, R_TY, R_M = 0, 1, 2, 3, 4, 5, 6, 7
R_ALPHA, R_BETA, R_HUE, R_SAT, R_VAL, R_KIND, R_SIGMA, R_DIR, R_NOISE, R_Y0, R_X0, R_HH, R_HW = 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
f32 = np.float32


def mix64(z: int) -> int:
    """splitmix64's finaliser on Python ints."""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix64_array(z: np.ndarray) -> np.ndarray:
    """The same on a uint64 array (wrapping arithmetic); pinned against mix64 in test_augment_reference.py."""
    z = z.astype(np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def u01(h: int) -> float:
    return (h >> 40) / 16777216.0


def base_of(seed: int, step: int, index: int) -> int:
    return mix64((seed & MASK) ^ mix64((index * INDEX_MUL + step) & MASK))


def draw_medium(seed: int, step: int, index: int, ho: int, wo: int) -> np.ndarray:
    """The medium policy's record for one image, slots 7..12 (the map) left for compose_map."""
    base = base_of(seed, step, index)
    u = lambda k: u01(mix64((base + k) & MASK))  # noqa: E731
    uf = lambda k: f32(u(k))  # noqa: E731  (exact: 24 bits)
    r = np.zeros(PARAMS)
    flags = 0
    for name, k in (("flip", 16), ("rot90", 17), ("rotate", 19), ("affine", 21), ("bc", 26), ("hsv", 29), ("blur", 33), ("noise", 37),
                    ("drop", 39)):
        if uf(k) < f32(PROBABILITY[name]):
            flags |= STAGES[name]
    r[R_FLAGS] = flags
    r[R_K] = min(3, int(uf(18) * f32(4)))
    r[R_ROT] = (u(20) * 2 - 1) * 15
    r[R_TX] = (u(22) * .2 - .1) * wo
    r[R_TY] = (u(23) * .2 - .1) * ho
    r[R_AFF_SCALE] = .9 + u(24) * .2
    r[R_AFF_ROT] = (u(25) * 2 - 1) * 15
    r[R_ALPHA] = 1 + (u(27) * .4 - .2)
    r[R_BETA] = u(28) * .4 - .2
    r[R_HUE] = (u(30) * 2 - 1) * 10
    r[R_SAT] = (u(31) * 2 - 1) * 15
    r[R_VAL] = (u(32) * 2 - 1) * 10
    r[R_KIND] = min(2, int(uf(34) * f32(3)))
    r[R_SIGMA] = .5 + u(35) * 2.5
    r[R_DIR] = min(3, int(uf(36) * f32(4)))
    r[R_NOISE] = (.01 + u(38) * .04) * 255
    side = lambda k: f32(float(uf(k)) * float(f32(.1)) + float(f32(.05)))  # noqa: E731  (one rounding: the kernel's fused multiply-add)
    hh = min(ho, max(1, int(side(40) * f32(ho))))
    hw = min(wo, max(1, int(side(41) * f32(wo))))
    r[R_HH], r[R_HW] = hh, hw
    r[R_Y0] = min(ho - hh, int(uf(42) * f32(ho - hh + 1)))
    r[R_X0] = min(wo - hw, int(uf(43) * f32(wo - hw + 1)))
    return r


def _after(a, b):
    """2x3 maps as 3x3 matrices: a after b."""
    return a @ b


def _map(a, b, c, d, e, f):
    return np.array([[a, b, c], [d, e, f], [0., 0., 1.]])


def resize_map(h, w, ho, wo):
    rx, ry = w / wo, h / ho
    return _map(rx, 0, .5 * rx - .5, 0, ry, .5 * ry - .5)  # s = (o + .5) * (src / dst) - .5


def compose_map(rec, h, w, ho, wo) -> np.ndarray:
    """Output pixel -> source pixel, [m0..m5]: resize . flip^-1 . rot90^-1 . rotate^-1 . affine^-1 (the rightmost first)."""
    flags, k = int(rec[R_FLAGS]), int(rec[R_K])
    cx, cy = (wo - 1) / 2, (ho - 1) / 2
    m = resize_map(h, w, ho, wo)
    if flags & F_FLIP:
        m = _after(m, _map(-1, 0, wo - 1, 0, 1, 0))
    if flags & F_ROT90 and k:
        # pixel -> normalised (u, v) -> turned -> pixel: u = (x + .5) / wo, v = (y + .5) / ho
        to_uv = _map(1 / wo, 0, .5 / wo, 0, 1 / ho, .5 / ho)
        from_uv = _map(wo, 0, -.5, 0, ho, -.5)
        turn = {1: _map(0, -1, 1, 1, 0, 0), 2: _map(-1, 0, 1, 0, -1, 1), 3: _map(0, 1, 0, -1, 0, 1)}[k]
        m = _after(m, from_uv @ turn @ to_uv)
    centre, back = _map(1, 0, -cx, 0, 1, -cy), _map(1, 0, cx, 0, 1, cy)
    if flags & F_ROTATE:
        t = math.radians(rec[R_ROT])
        m = _after(m, back @ _map(math.cos(t), -math.sin(t), 0, math.sin(t), math.cos(t), 0) @ centre)
    if flags & F_AFFINE:
        t, s = math.radians(rec[R_AFF_ROT]), rec[R_AFF_SCALE]
        shift = _map(1, 0, -rec[R_TX], 0, 1, -rec[R_TY])
        m = _after(m, back @ _map(math.cos(t) / s, math.sin(t) / s, 0, -math.sin(t) / s, math.cos(t) / s, 0) @ centre @ shift)
    return m[:2].reshape(6)


def sample(img, m, ho, wo, constant: bool) -> np.ndarray:
    """One bilinear sample per output pixel of img [H,W,3] (float64) through the map m; outside taps read 0 (constant) or
    the coordinate is clamped into the image."""
    h, w = img.shape[:2]
    oy, ox = np.meshgrid(np.arange(ho, dtype=np.float64), np.arange(wo, dtype=np.float64), indexing="ij")
    sx = m[0] * ox + m[1] * oy + m[2]
    sy = m[3] * ox + m[4] * oy + m[5]
    if not constant:
        sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]

    def tap(y, x):
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(ok[..., None], img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0.0)

    x1, y1 = x0 + 1, y0 + 1
    if not constant:
        x1, y1 = np.minimum(x1, w - 1), np.minimum(y1, h - 1)
    top = tap(y0, x0) * (1 - fx) + tap(y0, x1) * fx
    bot = tap(y1, x0) * (1 - fx) + tap(y1, x1) * fx
    return top * (1 - fy) + bot * fy


def rgb_to_hsv(v):
    """[...,3] levels in [0,255] -> H degrees in [0,360), S and V in [0,1] (OpenCV's float convention; H = 0 for greys)."""
    r, g, b = (v[..., c] / 255.0 for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    safe = np.where(d > 0, d, 1.0)
    h = np.where(mx == r, 60 * (g - b) / safe, np.where(mx == g, 120 + 60 * (b - r) / safe, 240 + 60 * (r - g) / safe))
    h = np.where(d > 0, h, 0.0)
    h = np.where(h < 0, h + 360, h)
    s = np.where(mx > 0, d / np.where(mx > 0, mx, 1.0), 0.0)
    return h, s, mx


def hsv_to_rgb(h, s, val):
    h6 = h / 60.0
    fl = np.floor(h6)
    f = h6 - fl
    sext = np.mod(fl.astype(np.int64), 6)
    p, q, t = val * (1 - s), val * (1 - s * f), val * (1 - s * (1 - f))
    r = np.choose(sext, [val, q, p, p, t, val])
    g = np.choose(sext, [t, val, val, q, p, p])
    b = np.choose(sext, [p, p, t, val, val, q])
    return np.stack([r, g, b], axis=-1) * 255.0


def point_chain(v, rec):
    """Stages 5-6 on sampled levels v [...,3]; also returns max - min before the HSV stage (the hue's conditioning)."""
    flags = int(rec[R_FLAGS])
    if flags & F_BC:
        v = np.clip(v * rec[R_ALPHA] + rec[R_BETA] * 255.0, 0, 255)
    spread = v.max(axis=-1) - v.min(axis=-1)
    if flags & F_HSV:
        h, s, val = rgb_to_hsv(v)
        h = h + 2 * rec[R_HUE]
        h = h - 360 * np.floor(h / 360)
        s = np.clip(s + rec[R_SAT] / 255.0, 0, 1)
        val = np.clip(val + rec[R_VAL] / 255.0, 0, 1)
        v = hsv_to_rgb(h, s, val)
    return v, spread


def blur_weights(kind: int, sigma: float, direction: int) -> np.ndarray:
    if kind == 0:
        return np.full((3, 3), 1 / 9)
    if kind == 1:
        g = np.exp(-np.array([-1., 0., 1.]) ** 2 / (2 * sigma * sigma))
        g /= g.sum()
        return np.outer(g, g)
    w = np.zeros((3, 3))
    for t in (-1, 0, 1):  # direction 0 '-', 1 '|', 2 '\', 3 '/'
        dy, dx = {0: (0, t), 1: (t, 0), 2: (t, t), 3: (-t, t)}[direction]
        w[1 + dy, 1 + dx] = 1 / 3
    return w


def reflect101(i, n):
    i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    return np.clip(i, 0, n - 1)


def neighbourhood(a, dy, dx):
    """a [Ho,Wo,...] read at (y + dy, x + dx) with reflect-101 borders."""
    ho, wo = a.shape[:2]
    return a[reflect101(np.arange(ho) + dy, ho)][:, reflect101(np.arange(wo) + dx, wo)]


def blur(v, weights):
    out = np.zeros_like(v)
    for j in range(9):
        if weights[j // 3, j % 3]:
            out += weights[j // 3, j % 3] * neighbourhood(v, j // 3 - 1, j % 3 - 1)
    return out


def gaussian_field(base: int, ho: int, wo: int) -> np.ndarray:
    """Box-Muller z [Ho,Wo,3] from the hash of (base, output pixel, channel)."""
    e = np.arange(ho * wo * 3, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64_array(np.uint64((base + NOISE_OFFSET) & MASK) + e)
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return (np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)).reshape(ho, wo, 3)


def normalize(v):
    """Levels [Ho,Wo,3] -> Normalize(ImageNet mean/std, max 255) in CHW."""
    return np.transpose((v - MEAN * 255.0) / (STD * 255.0), (2, 0, 1))


def medium_image(img_u8, rec, base: int, ho: int, wo: int, m=None):
    """One image under the record rec (flags and values; the map m defaults to the record's own).  Returns the normalised
    CHW float64 image and a mask [Ho,Wo] of pixels whose hue is ill-conditioned (HSV fired and 0 < max - min < 0.01 levels
    before it, at the pixel or, under a blur, at one of its neighbours)."""
    rec = np.asarray(rec, dtype=np.float64)
    flags = int(rec[R_FLAGS])
    m = rec[R_M:R_M + 6] if m is None else m
    v = sample(img_u8.astype(np.float64), m, ho, wo, bool(flags & (F_ROTATE | F_AFFINE)))
    v, spread = point_chain(v, rec)
    ill = (spread > 0) & (spread < 0.01) if flags & F_HSV else np.zeros((ho, wo), dtype=bool)
    if flags & F_BLUR:
        v = blur(v, blur_weights(int(rec[R_KIND]), rec[R_SIGMA], int(rec[R_DIR])))
        ill = np.any([neighbourhood(ill, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    if flags & F_NOISE:
        v = np.clip(v + rec[R_NOISE] * gaussian_field(base, ho, wo), 0, 255)
    if flags & F_DROP:
        y0, x0, hh, hw = (int(rec[s]) for s in (R_Y0, R_X0, R_HH, R_HW))
        v = v.copy()
        v[y0:y0 + hh, x0:x0 + hw] = 0.0
    return normalize(v), ill


def resize_image(img_u8, ho: int, wo: int):
    """Policy 0: the clamped bilinear resize alone, normalised."""
    h, w = img_u8.shape[:2]
    return normalize(sample(img_u8.astype(np.float64), resize_map(h, w, ho, wo)[:2].reshape(6), ho, wo, False))


def medium_record(seed: int, step: int, index: int, h: int, w: int, ho: int, wo: int) -> np.ndarray:
    """The whole record the kernel reports for (seed, step, index), drawn and composed here."""
    rec = draw_medium(seed, step, index, ho, wo)
    rec[R_M:R_M + 6] = compose_map(rec, h, w, ho, wo)
    return rec


def record_tolerance(h: int, w: int, ho: int, wo: int) -> np.ndarray:
    """Per-slot |device - restatement| bound for a record: integers exact; a drawn value is one float32 affine expression of
    an exact 24-bit fraction (a few ulp of its range); the map is some 20 float32 products and sums of terms up to the
    larger side (the translations) or the scale ratio (the linear part), plus sinf/cosf at 2 ulp."""
    eps = 2.0 ** -24
    size = float(max(h, w, ho, wo))
    ratio = max(1.0, h / ho, w / wo, ho / wo, wo / ho)
    tol = np.zeros(PARAMS)
    tol[[R_ROT, R_AFF_ROT]] = 8 * eps * 15
    tol[R_AFF_SCALE] = tol[R_ALPHA] = tol[R_BETA] = 8 * eps
    tol[[R_TX, R_TY]] = 8 * eps * size
    tol[[R_HUE, R_SAT, R_VAL]] = 8 * eps * 15
    tol[R_SIGMA] = 8 * eps * 3
    tol[R_NOISE] = 8 * eps * 255
    tol[[R_M, R_M + 1, R_M + 3, R_M + 4]] = 32 * eps * ratio
    tol[[R_M + 2, R_M + 5]] = 32 * eps * size * ratio
    return tol


# ---- the datasets the CPU and GPU tests share ----------------------------------------------------------------------------
# (stored H, W), (Ho, Wo): smaller than a tile; ragged tiles with anisotropic up- and down-scaling; more than one tile each
# way; the 96-from-32 case
CASES = (((5, 7), (5, 7)), ((17, 23), (19, 13)), ((33, 40), (33, 40)), ((32, 32), (96, 96)))
CASE_IMAGES = 64
CASE_SEED = 1     # chosen with draw_medium: every stage, k = 1, 2, 3 and each blur kind fire among indices 0..63 at step 1
STATS_IMAGES = 4000
STATS_SEED = 1    # chosen with draw_medium: every rate within 4 binomial sigma (test_augment_reference.py re-checks both)


def case_dataset(case: int):
    (h, w), _ = CASES[case]
    rng = np.random.RandomState(100 + case)
    return rng.randint(0, 256, size=(CASE_IMAGES, h, w, 3), dtype=np.uint8), rng.randint(0, 10, size=CASE_IMAGES)


def coverage(records) -> dict:
    """Which stages, quarter turns and blur kinds fired in a [n, PARAMS] array of records."""
    flags = records[:, R_FLAGS].astype(np.int64)
    seen = {name: bool(np.any(flags & bit)) for name, bit in STAGES.items()}
    for k in (1, 2, 3):
        seen[f"k={k}"] = bool(np.any(((flags & F_ROT90) != 0) & (records[:, R_K] == k)))
    for kind in (0, 1, 2):
        seen[f"blur kind {kind}"] = bool(np.any(((flags & F_BLUR) != 0) & (records[:, R_KIND] == kind)))
    return seen


RANGES = {R_K: (0, 3), R_ROT: (-15, 15), R_AFF_ROT: (-15, 15), R_AFF_SCALE: (.9, 1.1), R_ALPHA: (.8, 1.2), R_BETA: (-.2, .2),
          R_HUE: (-10, 10), R_SAT: (-15, 15), R_VAL: (-10, 10), R_KIND: (0, 2), R_SIGMA: (.5, 3), R_DIR: (0, 3),
          R_NOISE: (.01 * 255, .05 * 255)}


def check_statistics(records, ho: int, wo: int) -> None:
    """Rates within 4 binomial sigma of their p, k / blur kind / direction uniform by the same rule, values in range."""
    n = records.shape[0]
    flags = records[:, R_FLAGS].astype(np.int64)

    def within(rate, p, what):
        assert abs(rate - p) <= 4 * math.sqrt(p * (1 - p) / n), f"{what}: rate {rate:.4f} against p = {p}"

    for name, bit in STAGES.items():
        within(float(np.mean((flags & bit) != 0)), PROBABILITY[name], name)
    for slot, count, what in ((R_K, 4, "k"), (R_KIND, 3, "blur kind"), (R_DIR, 4, "motion direction")):
        for value in range(count):
            within(float(np.mean(records[:, slot] == value)), 1 / count, f"{what} = {value}")
    slack = 1e-5  # float32 rounding of a value at the end of its range
    for slot, (lo, hi) in RANGES.items():
        assert records[:, slot].min() >= lo - slack * max(1, abs(lo)) and records[:, slot].max() <= hi + slack * max(1, abs(hi)), slot
    assert np.all(np.abs(records[:, R_TX]) <= .1 * wo * (1 + slack)) and np.all(np.abs(records[:, R_TY]) <= .1 * ho * (1 + slack))
    hh, hw, y0, x0 = (records[:, s] for s in (R_HH, R_HW, R_Y0, R_X0))
    assert np.all(hh >= max(1, int(.05 * ho))) and np.all(hh <= max(1, math.ceil(.15 * ho)))
    assert np.all(hw >= max(1, int(.05 * wo))) and np.all(hw <= max(1, math.ceil(.15 * wo)))
    assert np.all(y0 >= 0) and np.all(y0 + hh <= ho) and np.all(x0 >= 0) and np.all(x0 + hw <= wo)
    assert np.all(records[:, [R_K, R_KIND, R_DIR, R_Y0, R_X0, R_HH, R_HW, R_FLAGS]] % 1 == 0)
