"""Cases, the plane layout restated once and the launch helpers for the value planes of the merged FeatureTransformer backward
(tests/test_gpu_value_planes.py).  Not a test module.

The value planes (csrc/value_planes.h) hold the table rows the value gradient d_val = (d_out W^T) . A reads, split into three
bf16 planes and stored in the fragment order of the 32 x 64 value tile: nnue_ftm_conv_binarize_value_planes writes them,
nnue_ftm_backward_planes reads them.  The float64 reference, the case builder and the guard bands are those of
tests/ste_ride_cases.py; the policy floor (256 value tiles) is lowered with NNUE_FTM_VAL_PLANES_MIN_TILES=1 so that the small
shapes below reach the kernel."""
import torch

import ste_ride_cases as ride
from nnue_hip import lib

DEV = "cuda"
BLOCK = 3 * 64 * 128 * 2  # bytes of one (column tile, K tile) block
PLANE = 64 * 128 * 2

# (B, H, W, stride, L1[, F]); F = P where not given.  P = 8 * Gh * Gw.
TILE_SHAPES = (
    (1, 17, 23, 2, 64),            # one row; L1 shorter than a K tile; G = 108 (not a multiple of 8); H != W
    (31, 31, 31, 3, 128),          # a row tile's end, one K tile
    (32, 31, 31, 3, 128),
    (33, 31, 31, 3, 128),
    (37, 31, 31, 3, 136),          # a ragged last K tile at L1 % 8 == 0
    (5, 25, 25, 2, 264),           # two full K tiles plus a ragged one
    (33, 13, 29, 4, 72, 257),      # F = P + 1: no sink columns (G = 32, P = 256)
    (9, 12, 12, 1, 104, 300),      # F well below P (G = 144, P = 1152): most columns read the clamp row
    (250, 32, 32, 3, 1024, 800),   # the C2 tile count along N at a ragged batch
)
# the writer beside the forward's riders (the forward planes want L1 % 64 == 0 and more than 128 rows): (B, H, W, stride, L1, F, L2)
#   G = 121 / 108: 128-thread conv workgroups, two riders per block; G = 49: 64 threads, four; G = 144: 256 threads, one
#   L1 = 192: a ragged last K tile; F = P + 1: no clamp; F = 300 < P: the clamp row; G % 8 != 0: clamped grid positions
PLANE_SHAPES = (
    (130, 31, 31, 3, 128, 800, 16), (130, 17, 23, 2, 192, 865, 16), (130, 13, 13, 2, 64, 300, 16), (130, 12, 12, 1, 128, 300, 16),
)


def shape_id(shape):
    return "x".join(str(v) for v in shape)


# ---- the layout: byte offset of the bf16 (plane, column n of tile tile_n, j_local of K tile kt), and the table row of a column
def plane_byte(tile_n, kt, plane, n, j_local, ktiles):
    frag = 4 * (n >> 4) + (j_local >> 5)
    lane = 16 * ((j_local >> 3) & 3) + (n & 15)
    return (tile_n * ktiles + kt) * BLOCK + plane * PLANE + ((frag * 64 + lane) << 4) + (j_local & 7) * 2


def plane_row(tile_n, n, g, f):
    hw = torch.clamp(tile_n * 8 + (n & 7), max=g - 1)
    return torch.clamp((n >> 3) * g + hw, max=f - 1)


def decode_planes(planes, g, f, l1):
    """([3][tiles_n][64][ktiles * 128] float32 plane values, [tiles_n][64] table rows) read through plane_byte / plane_row."""
    tiles_n, ktiles = (g + 7) // 8, (l1 + 127) // 128
    assert planes.numel() == tiles_n * ktiles * BLOCK
    pl, tn, n, kt, jl = torch.meshgrid(torch.arange(3), torch.arange(tiles_n), torch.arange(64), torch.arange(ktiles), torch.arange(128),
                                       indexing="ij")
    at = plane_byte(tn, kt, pl, n, jl, ktiles)
    assert int(at.unique().numel()) == at.numel() == planes.numel() // 2, "the index function is a bijection onto the buffer"
    halves = planes.cpu().view(torch.int16)[at // 2]
    vals = (halves.to(torch.int32) << 16).view(torch.float32).reshape(3, tiles_n, 64, ktiles * 128)
    tn2, n2 = torch.meshgrid(torch.arange(tiles_n), torch.arange(64), indexing="ij")
    return vals, plane_row(tn2, n2, g, f)


def wide(gen, *shape, span=125):  # random sign, exponent uniform in [-span, span], full 24-bit mantissa
    mant = 1.0 + torch.rand(*shape, generator=gen, dtype=torch.float64)
    e = torch.randint(-span, span + 1, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * mant * torch.exp2(e)).float()


# ---- the tile
def supported(shape):
    b, h, w, stride, l1, f, p, _, _ = ride.geometry(shape)
    return lib.ftm_value_planes_supported(b, f, p, l1, h, w, stride)


def write_planes(c, band=None):
    """The value planes of the case's table from the conv launch's riders alone (no forward planes); 0xFF-prefilled.
    band (a ste_ride_cases.Banded): the table and the planes are guarded views."""
    wrap = band if band is not None else (lambda t: t)
    b, h, w, stride, l1, f, p, _, _ = ride.geometry(c.shape)
    vp = wrap(torch.full((lib.ftm_value_planes_bytes(b, f, p, l1),), 0xFF, dtype=torch.uint8, device=DEV))
    conv_w = torch.zeros((ride.FPS, 3, 3, 3), device=DEV)  # the planes depend on the table alone
    lib.ftm_conv_binarize_planes(c.dev["images"], conv_w, c.dev["thr"], stride, wrap(c.dev["weight"]), 0, None, val_planes=vp)
    torch.cuda.synchronize()
    return vp


def launch(c, vp, dst=True, band=None, riders=False):
    """One nnue_ftm_backward_planes launch on NaN-prefilled outputs: {"part", "d_w", "d_b", "d_v", "sq", "d_w1"}.  band: every
    tensor the launch reads or writes (but the planes, which write_planes guards) is a guarded view; riders: the launch also
    leaves the norm partials and, where the shape carries it, d_w1."""
    b, h, w, stride, l1, f, p, gh, gw = ride.geometry(c.shape)
    wrap = band if band is not None else (lambda t: t)
    d, fm = c.dev, c.fm
    if band is not None:
        fm = lib.FeatureMatrix(wrap(fm.bits), wrap(fm.n), wrap(fm.sink), wrap(fm.scratch), fm.positions, fm.num_rows)
    chunks = ride.ste_chunks(c.shape)
    nan = lambda *s: wrap(torch.full(s, float("nan"), device=DEV))  # noqa: E731
    out = dict(part=nan(ride.FPS * 28 * chunks), d_v=nan(b, p) if dst else None, d_w=nan(f, l1), d_b=nan(l1), sq=None, d_w1=None)
    n_sq = lib.ftm_backward_sq_count(b, f, p, l1)
    extra = {}
    if riders:
        out["sq"] = nan(n_sq)
        extra["sq_partial"] = out["sq"]
        if lib.ftm_backward_cw_supported(b, f, p, l1, c.l2):
            out["d_w1"] = nan(c.l2, l1)
            extra.update(ft=wrap(c.ft), d_z1=wrap(c.d_z1), d_w1=out["d_w1"])
    lib.ftm_backward(wrap(d["d_out"]), wrap(d["weight"]), fm, d_weight=out["d_w"], d_bias=out["d_b"], dst=out["d_v"],
                     ste=(wrap(d["images"]), wrap(d["conv_out"]), wrap(d["thr"]), stride, out["part"]), val_planes=vp, **extra)
    torch.cuda.synchronize()
    return out


def build_case(shape, grid=False):
    """ste_ride_cases.build_case plus the rider's operands; grid: d_out and the table on a 2^-6 grid in [-1, 1], where every
    sum of the value product (<= 1024 products that are multiples of 2^-12, |sum| <= 1024) is exact in float32 in any order
    and the three-way split is exact (hi alone), so d_conv_out must EQUAL the float64 value."""
    c = ride.build_case(shape)
    b, _, _, _, l1, f, _, _, _ = ride.geometry(shape)
    g = torch.Generator().manual_seed(17 * b + l1)
    if grid:
        c.d_out = torch.randint(-64, 65, (b, l1), generator=g).float() / 64
        c.weight = torch.randint(-64, 65, (f, l1), generator=g).float() / 64
        c.dev["d_out"], c.dev["weight"] = c.d_out.to(DEV), c.weight.to(DEV)
    c.l2 = 32
    c.ft = torch.randn(b, l1, generator=g).to(DEV)
    c.d_z1 = torch.randn(b, c.l2, generator=g).to(DEV)
    return c
