"""Shapes, operands and float64 references for tests/test_gpu_rider_planes.py: the merged FeatureTransformer backward's d_w1
rider (d_w1 = d_z1^T l0, l0 the pairwise block of ft) as six bf16 plane products (gemm_tile_bf6t in csrc/ftm_kernels.hip).

A case is (B, fps, Gh, Gw, F, L1, L2).  The small ones are the smallest shapes that reach a bf16 kernel with the rider: map
8 x 10 x 10 (P = 800), F = 800, L1 % 128 == 0.  The tile is 32 x 64 x 64:
  L1   128: one column tile per pairwise half (both fold branches run); 256: two
  L2   8 less than a row tile, 32 exactly one, 72 a ragged last row tile, 128 four full ones
  B    1, 63: a K tail inside one K tile; 64: exactly one; 65: one row into the next; 130: two tiles and a tail
and one "big"-class shape of tests/test_gpu_merged_backward_variants.py's rider rows (64 x 64 value tiles as six plane products).
"""
import torch

DEV = "cuda"
SMALL_MAP = (8, 10, 10, 800)  # fps, Gh, Gw, F
BIG = (193, 8, 23, 22, 1501, 512, 72)
SHAPES = tuple((b, *SMALL_MAP, 128, 72) for b in (1, 63, 64, 65, 130)) + \
    tuple((130, *SMALL_MAP, 256, l2) for l2 in (8, 32, 72, 128)) + ((65, *SMALL_MAP, 128, 8), BIG)
BUCKET_SHAPES = ((130, *SMALL_MAP, 128, 72), (130, *SMALL_MAP, 256, 8))
SEG = (0, 37, 37, 130)  # K = 3 stacks, the middle one empty, boundaries that are no multiple of 4
shape_id = lambda s: "x".join(map(str, s))  # noqa: E731
_CASES = {}


def geometry(shape):
    b, fps, gh, gw, f, l1, l2 = shape
    return b, f, fps * gh * gw, l1, l2


def pairwise(x):
    half = x.shape[1] // 2
    return torch.cat([x[:, :half] * x[:, half:], x[:, :half]], dim=1)


def rider_operands(shape, regime):
    """ft [B, L1], d_z1 [B, L2] as tests/test_gpu_merged_backward_variants.py::rider_operands draws them: on grids (ft k / 16 in
    [0, 1], d_z1 k / 64 in [-1, 1]) in the unit regime, where every product is a multiple of 2^-14 and every sum of <= 193 of them
    stays below 2^8: exact in float32 in any order, and the three-way split of such operands has zero mid and lo planes."""
    b, _, _, l1, l2 = geometry(shape)
    gen = torch.Generator().manual_seed(b + l1 + 7 * l2)
    if regime == "unit":
        ft = torch.randint(0, 17, (b, l1), generator=gen).float() / 16
        d_z1 = torch.randint(-64, 65, (b, l2), generator=gen).float() / 64
    else:
        ft, d_z1 = torch.rand(b, l1, generator=gen), torch.randn(b, l2, generator=gen) / b
    return ft, d_z1


def case(shape, regime):
    """The launch's own operands (built once, never modified), the rider's, and the float64 d_w1."""
    if (shape, regime) in _CASES:
        return _CASES[shape, regime]
    from nnue_hip import lib
    b, f, p, l1, l2 = geometry(shape)
    gen = torch.Generator().manual_seed(1000 * b + f + l1)
    weight, d_out = torch.randn(f, l1, generator=gen) * 0.1, torch.randn(b, l1, generator=gen) / b
    conv_out, thr = torch.randn(b, *shape[1:4], generator=gen), torch.full((shape[1],), 0.52)
    images = torch.randn(b, 3, 3 * shape[2], 3 * shape[3], generator=gen)  # stride 3: the map's grid
    ft, d_z1 = rider_operands(shape, regime)
    c = dict(shape=shape, regime=regime, weight=weight.to(DEV), d_out=d_out.to(DEV), ft=ft, d_z1=d_z1, l0=pairwise(ft.double()),
             conv_out=conv_out.to(DEV), thr=thr.to(DEV), images=images.to(DEV))
    c["ref"] = d_z1.double().t() @ c["l0"]
    if regime == "unit":
        assert torch.equal(c["ref"].float().double(), c["ref"]) and float(c["ref"].abs().max()) < 2.0 ** 8
    c["fm"] = lib.ftm_binarize(c["conv_out"], c["thr"], f, l1)
    _CASES[shape, regime] = c
    return c


class Banded:
    """Interior views (16-byte aligned) of NaN-filled buffers, 64 rows + 256 floats deep on either side: outputs whose bands must
    stay NaN, and operands (call with `of=`) a read past whose ends shows as NaN in the result."""

    def __init__(self):
        self.bufs = []

    def __call__(self, *shape, of=None):
        n = 1
        for s in shape:
            n *= s
        band = 64 * shape[-1] + 256
        buf = torch.full((n + 2 * band,), float("nan"), device=DEV)
        view = buf[band:band + n].view(shape)
        if of is not None:
            view.copy_(of)
        else:
            self.bufs.append((buf, band, n))
        return view

    def untouched(self):
        return all(bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[band + n:]).all()) for buf, band, n in self.bufs)


def launch(c, rider=True, sq=False, ste=False, ft=None, d_z1=None, buckets=None, stacks=1):
    """One lib.ftm_backward call; every output an interior view of a NaN-filled buffer.  Returns a dict of the outputs."""
    from nnue_hip import lib
    b, f, p, l1, l2 = geometry(c["shape"])
    band = Banded()
    out = dict(d_w=band(f, l1), d_b=band(l1), d_v=band(b, p), d_w1=None, sq=None, part=None)
    kw = {}
    if rider:
        out["d_w1"] = band(l2, l1) if buckets is None else band(stacks, l2, l1)
        kw.update(ft=band(*c["ft"].shape, of=c["ft"]) if ft is None else ft, d_z1=band(*c["d_z1"].shape, of=c["d_z1"]) if d_z1 is None else d_z1,
                  d_w1=out["d_w1"], buckets=buckets)
    if sq:
        n_sq = lib.ftm_backward_sq_count(b, f, p, l1)
        out["sq"] = band(n_sq)
        kw["sq_partial"] = out["sq"]
    if ste:
        chunks = lib.ftm_backward_ste_chunks(b, f, p, l1, c["images"].shape[2], c["images"].shape[3], 3)
        assert chunks > 0, "the STE ride is not taken"
        out["part"] = band(8 * 28, chunks)
        kw["ste"] = (c["images"], c["conv_out"], c["thr"], 3, out["part"])
    lib.ftm_backward(c["d_out"], c["weight"], c["fm"], d_weight=out["d_w"], d_bias=out["d_b"], dst=out["d_v"], **kw)
    torch.cuda.synchronize()
    assert band.untouched(), "a guard band of an output was written"
    return out


def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
