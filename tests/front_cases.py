"""Cases and the float64 restatement of the float front end: the 3x3 conv, StraightThroughBinary.forward and the forms its
result takes (tests/test_front_cases.py pins this file on the CPU; tests/test_gpu_front_end.py holds the kernels to it).

Not a test module and no GPU import.  ``conv64`` is an explicit sum of the 27 shifted, strided slices of the zero-padded image
times one weight each, in float64 -- no conv2d, no matrix product -- so a NaN or Inf pixel propagates by IEEE rules
(0 * inf = NaN, inf - inf = NaN).  ``front64`` adds the strict ``>`` of the reference (nnue.py:15-54) and the layouts
include/nnue_hip.h states.

Exact inputs: pixels randint(-8, 9) / 4 and weights randint(-8, 9) / 8 (times a power of two each).  Every product is a multiple
of 1/32 of magnitude at most 2; a sum of 27 of them needs under 11 bits, so float32 holds every partial sum exactly in any order,
with or without fma, and "equal to float64" means bit for bit.  thr[c] is the lower median of channel c's outputs -- an attained
value, so every channel has ties and a ``>=`` in a kernel moves bits.
"""
import torch

SUBNORMAL = 2.0 ** -149  # the smallest positive float32
FLT_MAX = float(torch.finfo(torch.float32).max)

# (B, H, W, fps, stride, F).  Gh = (H-1)//stride + 1, Gw likewise, G = Gh*Gw, P = fps*G.
# The launch rule of conv_binarize_impl, which a test cannot observe: a workgroup has 64 threads when G <= 64, 128 when
# G <= 128, else 256; a sample is split over slices = ceil(512 / B) workgroups, but no more than G // threads and between 1 and
# 16; one slice writes the counts with plain stores, more add them with atomics into counters zeroed first.  Channels run in
# register passes of 8 (fpad = fps rounded up to 8); up to fps = 16 all 27 taps are unrolled, above that nine at a time.
SHAPES = (
    (1, 5, 7, 3, 7, 2),          # G = 1 (stride wider than the image); P = 3 (no multiple of 4); everything past id 0 is sink
    (2, 1, 9, 3, 2, 10),         # a one-row image: taps above and below are all padding; P = 15
    (3, 9, 9, 4, 4, 30),         # H, W no multiple of the stride (last patch hangs over the right and bottom edges); 64 threads;
                                 # clamp sink mid-map
    (5, 10, 10, 7, 3, 40),       # channel tail inside the only pass (fps = 7)
    (2, 17, 23, 12, 2, 2000),    # non-square; stride 2; two passes with a tail of 4; 128 threads; table larger than the map
    (2, 33, 31, 20, 3, 1000),    # fps > 16: the partly unrolled body; fpad = 24
    (3, 64, 48, 64, 7, 65536),   # the 64-channel form at the stride of the 224x224 workload; G = 70
    (600, 8, 8, 8, 3, 50),       # batch past 512 (one slice per sample); ragged ldb for the transposed coefficients
    (7, 24, 24, 2, 1, 500),      # stride 1; several samples each split over 2 slices (the counters' atomics)
    (1, 40, 36, 5, 1, 4000),     # 5 slices with a ragged last trip (1440 positions over 1280 threads); sink counts in the thousands
    (1, 48, 48, 24, 1, 100),     # sliced and partly unrolled together; nearly every id is sink
)
# the two smallest shapes with P % 4 == 0 (P = 36, P = 112) at F = 1 (every id is sink), F = P and F = P + 1 (no sink)
F_VARIANTS = tuple((3, 9, 9, 4, 4, f) for f in (1, 36, 37)) + tuple((5, 10, 10, 7, 3, f) for f in (1, 112, 113))
ALL_SHAPES = SHAPES + F_VARIANTS
SCALES = ((40, 30), (-70, -70))  # (scale_img, scale_w): outputs near 2**70, and subnormal outputs (multiples of 2**-145)
SCALED_SHAPES = ((3, 9, 9, 4, 4, 30), (2, 33, 31, 20, 3, 1000))
NONFINITE_SHAPES = SCALED_SHAPES
BACKWARD_SHAPES = ((2, 17, 23, 12, 2), (2, 33, 31, 20, 3), (3, 64, 48, 64, 7), (1, 40, 36, 5, 1), (2, 1, 9, 3, 2), (1, 5, 7, 3, 7))
MAP_SHAPES = (((3, 4, 3, 3), 30, 3), ((2, 20, 11, 11), 1000, 0))  # ((B, fps, Gh, Gw), F, first threshold kind)


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def seed_of(shape):
    return sum((i + 1) * v for i, v in enumerate(shape))


def geometry(shape):
    """(B, H, W, fps, stride, F, Gh, Gw, G, P)"""
    b, h, w, fps, stride, f = shape
    gh, gw = (h - 1) // stride + 1, (w - 1) // stride + 1
    return b, h, w, fps, stride, f, gh, gw, gh * gw, fps * gh * gw


def _taps(images, stride):
    """The 27 shifted, strided slices [B, Gh, Gw] of the zero-padded image, q = ci*9 + kh*3 + kw (float64)."""
    b, _, h, w = images.shape
    gh, gw = (h - 1) // stride + 1, (w - 1) // stride + 1
    pad = torch.zeros(b, 3, h + 2, w + 2, dtype=torch.float64)
    pad[:, :, 1:h + 1, 1:w + 1] = images.double()
    return [pad[:, ci, kh:kh + (gh - 1) * stride + 1:stride, kw:kw + (gw - 1) * stride + 1:stride]
            for ci in range(3) for kh in range(3) for kw in range(3)]


def conv64(images, weight, stride):
    """nn.Conv2d(3, fps, 3, stride, padding=1, bias=False) in float64 as the sum of its 27 terms, [B, fps, Gh, Gw]."""
    w = weight.double().reshape(weight.shape[0], 27)
    out = None
    for q, tap in enumerate(_taps(images, stride)):
        term = tap.unsqueeze(1) * w[:, q].view(1, -1, 1, 1)
        out = term if out is None else out + term
    return out


def lists_of(on):
    """Ascending active ids per sample: idx [B, P] int64 padded with -1."""
    n = on.sum(1)
    order = torch.argsort((~on).to(torch.int8), dim=1, stable=True)
    return torch.where(torch.arange(on.shape[1]).unsqueeze(0) < n.unsqueeze(1), order, torch.full_like(order, -1))


def forms_of(on, f):
    """n, sink and the id lists of a bool map [B, P]."""
    b, p = on.shape
    sink = on[:, f - 1:].sum(1).float() if f - 1 < p else torch.zeros(b)
    return dict(on=on, n=on.sum(1), sink=sink, idx=lists_of(on))


def front64(images, weight, thr, stride, f):
    """conv_out float64 [B, fps, Gh, Gw]; on bool [B, P] = conv_out > thr[c]; n int64 [B]; sink float32 [B] = active ids >= F-1;
    idx int64 [B, P] (ascending ids, -1 padding); patches float64 [27, B*G] (0 off the image)."""
    conv = conv64(images, weight, stride)
    b = conv.shape[0]
    on = (conv > thr.double().view(1, -1, 1, 1)).reshape(b, -1)
    out = forms_of(on, f)
    out["conv_out"] = conv
    out["patches"] = torch.stack([t.reshape(-1) for t in _taps(images, stride)])
    return out


def exact_case(shape, seed, scale_img=0, scale_w=0):
    """Dyadic inputs (float32) whose conv is exact in float32 in any order; thr = the lower median of each channel's outputs."""
    b, h, w, fps, stride, f = shape
    gen = torch.Generator().manual_seed(seed)
    images = (torch.randint(-8, 9, (b, 3, h, w), generator=gen).double() / 4 * 2.0 ** scale_img).float()
    weight = (torch.randint(-8, 9, (fps, 3, 3, 3), generator=gen).double() / 8 * 2.0 ** scale_w).float()
    conv = conv64(images, weight, stride)
    thr = conv.transpose(0, 1).reshape(fps, -1).median(dim=1).values.float()  # torch's median is the lower one
    return dict(shape=shape, images=images, weight=weight, thr=thr, stride=stride, F=f)


def random_case(shape, seed):
    """randn pixels, 0.2 * randn weights, 0.1 * randn thresholds, and the bound of a float32 fma chain of 27 terms against the
    exact sum: gamma_27 * sum|terms| <= 27u / (1 - 27u) * sum|terms|, u = 2**-24, taken as 28 * 2**-24 * conv64(|images|, |weight|)
    (one unit of slack; the cast of the result to float32 is the chain's last rounding)."""
    b, h, w, fps, stride, f = shape
    gen = torch.Generator().manual_seed(seed)
    images = torch.randn(b, 3, h, w, generator=gen)
    weight = 0.2 * torch.randn(fps, 3, 3, 3, generator=gen)
    thr = 0.1 * torch.randn(fps, generator=gen)
    bound = 28 * 2.0 ** -24 * conv64(images.abs(), weight.abs(), stride)
    return dict(shape=shape, images=images, weight=weight, thr=thr, stride=stride, F=f, bound=bound)


def nonfinite_case(shape, seed):
    """An exact case with one NaN in a corner pixel and one +Inf on an edge of sample 0, one -Inf in the interior of another
    sample, and the last sample all zeros of both signs (with B = 2 the -Inf pixel is the only other value in it).  The three
    pixels lie under a patch at strides 3 and 4."""
    c = exact_case(shape, seed)
    img = c["images"].clone()
    img[-1] = 0.0
    img[-1, :, ::2, 1::2] = -0.0
    img[0, 0, 0, 0] = float("nan")
    img[0, 1, 0, 4] = float("inf")
    img[1, 2, 4, 4] = float("-inf")
    c["images"] = img
    return c


THR_KINDS = ("attained", "+0", "-0", "+inf", "-inf", "nan", "subnormal")


def edge_thresholds(attained, first=0):
    """Per-channel thresholds cycling through THR_KINDS from kind `first`; `attained` [fps] supplies the attained values."""
    fixed = {"+0": 0.0, "-0": -0.0, "+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "subnormal": SUBNORMAL}
    thr = attained.clone().float()
    for c in range(thr.numel()):
        kind = THR_KINDS[(first + c) % len(THR_KINDS)]
        if kind != "attained":
            thr[c] = fixed[kind]
    return thr


def edge_map(map_shape, seed, first=0):
    """A conv_out-shaped float32 map of grid values randint(-8, 9) / 4 in which every channel also holds NaN, +Inf, -Inf, +0.0,
    -0.0, the smallest subnormal, its negative and FLT_MAX, with thresholds cycling through THR_KINDS (the attained value is the
    channel's lower median of the grid values)."""
    b, fps, gh, gw = map_shape
    gen = torch.Generator().manual_seed(seed)
    grid = torch.randint(-8, 9, (b, fps, gh, gw), generator=gen).float() / 4
    attained = grid.transpose(0, 1).reshape(fps, -1).median(dim=1).values
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, SUBNORMAL, -SUBNORMAL, FLT_MAX])
    x = grid.transpose(0, 1).reshape(fps, -1).clone()
    assert x.shape[1] > 2 * special.numel()
    for c in range(fps):
        perm = torch.randperm(x.shape[1], generator=gen)
        x[c, perm[:special.numel()]] = special
        x[c, perm[special.numel()]] = attained[c]  # the specials may have replaced every copy of the median: a tie stays
    x = x.reshape(fps, b, gh, gw).transpose(0, 1).contiguous()
    return x, edge_thresholds(attained, first)
