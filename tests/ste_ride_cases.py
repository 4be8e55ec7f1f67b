"""Cases and the float64 reference for the STE ride in the merged FeatureTransformer backward (tests/test_gpu_ste_ride.py).

Not a test module: it holds the shape list, the case builder, the float64 restatement of what the launch computes and the
check every case goes through, so that a fresh child process can run the same check with ``NNUE_FTM_RIDE_STE_V64=1`` (the
knob is read once per process).  ``python tests/ste_ride_cases.py`` is that child: it runs V64_SHAPES on the 64 x 64 value
tiles, prints one line per case and exits non-zero on the first failure.

The reference works on the launch's own inputs (images, the conv_out and map bytes handed in, thr, d_out, weight), so no
threshold decision can differ between it and the kernel:
    d_val = (d_out @ W^T)[:, clamp(arange(P), max=F-1)] * bits
    d_thr = -(d_val * ste_slope(conv_out, thr)).sum((0, 2, 3))
    d_w   = conv_weight_grad(images, d_val, stride)
The bar is 2e-5 * max|ref| per tensor, the one the stand-alone STE kernel and the value gradient are held to."""
import sys
import time
import traceback

import torch

from conftest import assert_close_grad  # also puts the package and the oracle on sys.path
import nnue_oracle as orc
from nnue_hip import lib

DEV = "cuda"
RTOL = 2e-5
FPS = 8

# (B, H, W, stride, L1[, F]); F = P where not given.  Windows that leave the image at the bottom / right ((H-1) % stride == 0:
# 31/3, 17/2, 25/2, every stride 1), H != W in both orders, grids of 1, 25, 32, 60, 63, 100, 108, 121, 130, 144, 154 and 256
# positions (multiples of 8 and not), B from 1 to 512 (ending inside a 32-row tile and not), F below P (the clamp sink: 300 < 480, 800 < 968) and equal to it.
SHAPES = (
    (5, 17, 23, 2, 64), (3, 7, 9, 1, 32), (1, 3, 3, 3, 8), (2, 5, 5, 1, 16), (7, 16, 16, 1, 64), (37, 31, 31, 3, 128),
    (64, 31, 40, 3, 256), (130, 25, 19, 2, 192), (33, 13, 29, 4, 72), (9, 12, 12, 1, 100), (65, 10, 6, 1, 36, 300),
    (16, 96, 96, 10, 1024, 800), (200, 31, 31, 3, 1024, 800), (512, 32, 32, 3, 1024, 800), (40, 32, 32, 3, 256, 800),
)
C2 = (512, 32, 32, 3, 1024, 800)
# the value regimes run at C2, at a shape whose windows leave the image and whose batch ends inside a tile, and at H != W
REGIME_SHAPES = (C2, (37, 31, 31, 3, 128), (5, 17, 23, 2, 64))
# 64 x 64 value tiles (the child process): full tiles, a ragged last row tile (1000 = 15 * 64 + 40), and L1 % 8 == 4, where the
# six-plane bf16 value tiles are not taken and the f32 instantiation runs
V64_SHAPES = ((1024, 32, 32, 3, 1024, 800), (1000, 31, 31, 3, 1024, 800), (1000, 31, 31, 3, 1020, 800))
BAND = 4096  # elements on each side of a guarded tensor: more than a sample's conv outputs or an image plane at these shapes


def geometry(shape):
    """(B, H, W, stride, L1, F, P, Gh, Gw) of a SHAPES entry."""
    b, h, w, stride, l1 = shape[:5]
    gh, gw = (h - 1) // stride + 1, (w - 1) // stride + 1
    p = FPS * gh * gw
    return b, h, w, stride, l1, (shape[5] if len(shape) > 5 else p), p, gh, gw


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def ste_chunks(shape):
    b, h, w, stride, l1, f, p, _, _ = geometry(shape)
    return lib.ftm_backward_ste_chunks(b, f, p, l1, h, w, stride)


class Case:
    """One launch's inputs: host copies for the reference, device tensors for the kernel (both forms of the pixel terms)."""


def build_case(shape, image_scale=1.0, thr_fill=None):
    b, h, w, stride, l1, f, p, gh, gw = geometry(shape)
    g = torch.Generator().manual_seed(1000 * b + 7 * h + w + l1)
    c = Case()
    c.shape, c.stride = shape, stride
    c.images = image_scale * torch.randn(b, 3, h, w, generator=g)
    conv_w = 0.3 * torch.randn(FPS, 3, 3, 3, generator=g)
    c.thr = 0.1 * torch.randn(FPS, generator=g) if thr_fill is None else torch.full((FPS,), float(thr_fill))
    c.d_out = torch.randn(b, l1, generator=g)
    c.weight = 0.05 * torch.randn(f, l1, generator=g)
    c.dev = {k: getattr(c, k).to(DEV) for k in ("images", "thr", "d_out", "weight")}
    d = c.dev
    d["conv_out"], c.fm = lib.ftm_conv_binarize(d["images"], conv_w.to(DEV), d["thr"], stride, f, l1)
    d["patches"] = torch.empty((27, b * gh * gw), device=DEV)
    d["conv_p"], c.fm_p = lib.ftm_conv_binarize(d["images"], conv_w.to(DEV), d["thr"], stride, f, l1, patches=d["patches"])
    torch.cuda.synchronize()
    assert torch.equal(d["conv_out"], d["conv_p"]) and torch.equal(c.fm.bits, c.fm_p.bits), "the two conv launches agree"
    c.conv_out, c.bits = d["conv_out"].cpu(), c.fm.bits.cpu()
    return c


def float64_reference(c):
    """(d_thr [8], d_w [8, 3, 3, 3], d_val [B, 8, Gh, Gw]) in float64 from the launch's inputs."""
    b, p = c.bits.shape
    f = c.weight.shape[0]
    rows = torch.clamp(torch.arange(p), max=f - 1)
    d_val = ((c.d_out.double() @ c.weight.double().t())[:, rows] * c.bits.double()).view(c.conv_out.shape)
    d_thr = -(d_val * orc.ste_slope(c.conv_out.double(), c.thr.double().view(1, -1, 1, 1))).sum(dim=(0, 2, 3))
    d_w = orc.conv_weight_grad(c.images.double(), d_val, c.stride, (FPS, 3, 3, 3))
    return d_thr, d_w, d_val


def ratio(got, ref):
    """max|got - ref| / max|ref|: the quantity assert_close_grad bounds."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)


def partial_sums(part, chunks):
    """(d_thr, d_w) as the chunk sums of the partials [8 * 28][chunks], in float64."""
    sums = part.view(FPS * 28, chunks).double().sum(1).view(FPS, 28).cpu()
    return -sums[:, 27], sums[:, :27].reshape(FPS, 3, 3, 3)


class Banded:
    """Tensors as interior views of larger buffers whose surroundings hold NaN (floats) or 0xFF (bytes / ints); the views start
    at a multiple of 16 bytes.  untouched() says whether every band still holds its fill."""

    def __init__(self):
        self.bufs = []

    def __call__(self, t):
        n = t.numel()
        buf = torch.empty((n + 2 * BAND,), dtype=t.dtype, device=t.device)
        if t.dtype.is_floating_point:
            buf.fill_(float("nan"))
        else:
            buf.view(torch.uint8).fill_(0xFF)
        view = buf[BAND:BAND + n].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 0
        self.bufs.append((buf, n))
        return view

    def untouched(self):
        for buf, n in self.bufs:
            for band in (buf[:BAND], buf[BAND + n:]):
                ok = torch.isnan(band).all() if buf.dtype.is_floating_point else (band.view(torch.uint8) == 0xFF).all()
                if not bool(ok):
                    return False
        return True


def launch(c, patches=False, dst=True, ste=True, band=None):
    """One nnue_ftm_backward launch on the case; the STE partials and dst are NaN-prefilled.  band (a Banded): every tensor the
    launch reads or writes is a guarded view.  Returns (partial, d_weight, d_bias, d_conv_out)."""
    b, h, w, stride, l1, f, p, gh, gw = geometry(c.shape)
    wrap = band if band is not None else (lambda t: t)
    d, fm = c.dev, (c.fm_p if patches else c.fm)
    if band is not None:
        fm = lib.FeatureMatrix(wrap(fm.bits), wrap(fm.n), wrap(fm.sink), wrap(fm.scratch), fm.positions, fm.num_rows)
    chunks = ste_chunks(c.shape)
    part = wrap(torch.full((FPS * 28 * chunks,), float("nan"), device=DEV))
    out_v = wrap(torch.full((b, p), float("nan"), device=DEV)) if dst else None
    d_w = wrap(torch.full((f, l1), float("nan"), device=DEV))
    d_b = wrap(torch.full((l1,), float("nan"), device=DEV))
    args = None
    if ste:
        args = (wrap(d["images"]), wrap(d["conv_p" if patches else "conv_out"]), wrap(d["thr"]), stride, part)
        if patches:
            args += (wrap(d["patches"]),)
    res = lib.ftm_backward(wrap(d["d_out"]), wrap(d["weight"]), fm, d_weight=d_w, d_bias=d_b, dst=out_v, ste=args)
    torch.cuda.synchronize()
    assert res[2] is out_v
    return part, d_w, d_b, out_v


def check_case(c, rtol=RTOL):
    """The whole check of one case; returns the measured ratios {"d_thr", "d_w", "d_conv_out"} against float64."""
    chunks = ste_chunks(c.shape)
    assert chunks > 0, f"{c.shape}: the merged launch does not take the ride"
    ref_thr, ref_w, ref_val = float64_reference(c)
    active = c.bits.bool()
    _, plain_w, plain_b, plain_v = launch(c, ste=False)
    assert bool(torch.isfinite(plain_w).all()) and bool(torch.isfinite(plain_v).all())
    part, d_w, d_b, d_v = launch(c)
    # every slot written; the launch's other outputs keep their bits
    assert bool(torch.isfinite(part).all()), "every partial slot is written"
    assert torch.equal(d_w, plain_w) and torch.equal(d_b, plain_b), "d_weight / d_bias are those of the launch without ste="
    assert torch.equal(d_v, plain_v), "d_conv_out is that of the launch without ste="
    got_thr, got_w = partial_sums(part, chunks)
    out = {"d_thr": ratio(got_thr, ref_thr), "d_w": ratio(got_w, ref_w), "d_conv_out": ratio(d_v.view(ref_val.shape), ref_val)}
    assert bool(torch.isfinite(d_v).all()) and not bool(d_v.cpu()[~active].any()), "d_conv_out: exact zeros at inactive positions"
    assert_close_grad(d_v.view(ref_val.shape), ref_val, "d_conv_out", rtol=rtol)
    assert_close_grad(got_w, ref_w, "d_weight (conv)", rtol=rtol)
    assert_close_grad(got_thr, ref_thr, "d_thr", rtol=rtol)
    # without dst the value gradient is not stored; a second run is bitwise the first
    again, _, _, none = launch(c, dst=False)
    assert none is None and torch.equal(again, part), "a second run is bitwise equal"
    # the pixel terms from the im2col patches: the same bits
    part_p, w_p, b_p, v_p = launch(c, patches=True)
    assert torch.equal(part_p, part), "partials from the patches are bitwise those from the pixels"
    assert torch.equal(w_p, plain_w) and torch.equal(b_p, plain_b) and torch.equal(v_p, plain_v)
    return out


def check_guard_bands(c):
    """Every operand an interior view of a NaN / 0xFF-surrounded buffer: the results are bitwise those of the plain allocation
    and the bands stay untouched (a clamp that is off by a row or a position reads or writes a band without faulting)."""
    for patches in (False, True):
        part, d_w, d_b, d_v = launch(c, patches=patches)
        band = Banded()
        g_part, g_w, g_b, g_v = launch(c, patches=patches, band=band)
        assert bool(torch.isfinite(g_part).all()) and torch.equal(g_part, part), f"patches={patches}: partials differ behind guard bands"
        assert torch.equal(g_v, d_v) and torch.equal(g_w, d_w) and torch.equal(g_b, d_b), f"patches={patches}: outputs differ behind guard bands"
        assert band.untouched(), f"patches={patches}: a guard band was written"


def main():
    """The child process of test_the_64_row_value_tiles_against_float64: V64_SHAPES with the knob set."""
    import os
    assert os.environ.get("NNUE_FTM_RIDE_STE_V64") == "1", "start this with NNUE_FTM_RIDE_STE_V64=1"
    worst = 0.0
    for shape in V64_SHAPES:
        t0 = time.time()
        try:
            b, _, _, _, l1, _, _, gh, gw = geometry(shape)
            chunks = ste_chunks(shape)
            assert chunks == ((b + 63) // 64) * ((gh * gw + 7) // 8), f"{shape}: {chunks} chunks are not those of 64-row value tiles"
            got = check_case(build_case(shape))
        except Exception:  # one line for the case, the traceback behind it
            print(f"FAIL {shape_id(shape)}", flush=True)
            traceback.print_exc()
            return 1
        worst = max(worst, *got.values())
        print(f"ok {shape_id(shape)} chunks {chunks} " + " ".join(f"{k} {v:.2e}" for k, v in got.items()) + f" ({time.time() - t0:.1f} s)", flush=True)
    print(f"worst ratio {worst:.2e} (bar {RTOL:.0e})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
