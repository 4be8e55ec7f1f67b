"""The bf16-split tiles (gemm_tile_bf / gemm_tile_bf64) at every tile height and both K depths, at shapes with tails on M, N
and K.  The operands are multiples of 2^-20 below 1 and every sum the kernels form has at most six terms, so each sum is
exact in float32 in ANY order: results are compared for equality with the float64 value, not against a tolerance.  ``-m gpu``."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [  # B, fps, Gh, Gw, F, L1
    (200, 4, 7, 7, 150, 72),  # clamp sink, two K tiles of the weight gradient, ragged everything
    (70, 4, 7, 7, 300, 72),   # table larger than the map, one ragged K tile
]
_CASES = {}


def _case(shape):
    """Inputs and float64 references of a shape, computed once and shared (never modified)."""
    if shape in _CASES:
        return _CASES[shape]
    b, fps, gh, gw, f, l1 = shape
    p = fps * gh * gw
    gen = torch.Generator().manual_seed(1000 * b + f)
    q = lambda *size: torch.randint(-(2 ** 20) + 1, 2 ** 20, size, generator=gen).double() / 2 ** 20  # k / 2^20, |k| < 2^20
    weight, bias, d_out = q(f, l1), q(l1), q(b, l1)
    pos = (5 * torch.arange(b).view(b, 1) + torch.arange(5).view(1, 5)) % p  # sample b is active at (5 b + j) mod P, j = 0..4
    bits = torch.zeros(b, p, dtype=torch.float64)
    bits.scatter_(1, pos, 1.0)
    conv_out = (2.0 * bits - 1.0).float().reshape(b, fps, gh, gw)  # +1 where active, -1 elsewhere; threshold 0
    rows = torch.clamp(torch.arange(p), max=f - 1)
    a = torch.zeros(b, f, dtype=torch.float64)
    a.index_add_(1, rows, bits)  # positions >= F-1 pile up on row F-1
    direct = min(f - 1, p)
    d_w = a.t() @ d_out
    ref = dict(out=a @ weight + bias, d_w=d_w[:direct], w_new=weight[:direct] - 0.5 * d_w[:direct], direct=direct)
    for k in ("out", "d_w", "w_new"):  # the float64 values are float32 numbers: equality below is meaningful
        assert torch.equal(ref[k].float().double(), ref[k]), k
    _CASES[shape] = (conv_out, weight.float(), bias.float(), d_out.float(), ref)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bm", (32, 64, 128))
def test_bf16_split_tiles_are_exact(monkeypatch, shape, bm):
    if os.environ.get("NNUE_FTM_BF16") == "0":
        pytest.skip("NNUE_FTM_BF16=0: the bf16-split tiles are switched off")
    from nnue_hip import lib
    L = lib.load()
    b, fps, gh, gw, f, l1 = shape
    p = fps * gh * gw
    conv_out, weight, bias, d_out, ref = _case(shape)
    direct = ref["direct"]
    monkeypatch.setenv("NNUE_FTM_BF_BM", str(bm))  # read per call
    assert L.nnue_ftm_uses_bf16(0, b, f, p, l1) == 1 and L.nnue_ftm_uses_bf16(1, b, f, p, l1) == 1  # not the f32 tiles
    g = lambda t: t.to(DEV)
    same = lambda got, want: torch.equal(got.cpu().double(), want)
    fm = lib.ftm_binarize(g(conv_out), torch.zeros(fps, device=DEV), f, l1)
    w_dev, bias_dev, d_dev = g(weight), g(bias), g(d_out)

    out = lib.ftm_forward(w_dev, bias_dev, fm)
    assert same(out, ref["out"])
    # with the bucket grouping riding along: at 128 rows the K-tile-128 path (the plain forward takes the K-tile-64 one)
    out_g = lib.ftm_forward(w_dev, bias_dev, fm, group=lib.BucketPlan(b, 2, DEV))
    assert same(out_g, ref["out"])

    d_w, _ = lib.ftm_backward_weight(d_dev, fm)  # d_bias and row F-1 come from another kernel and sum B terms: not checked here
    assert same(d_w[:direct], ref["d_w"])

    w_upd = w_dev.clone()
    lib.ftm_backward_weight_update(d_dev, fm, w_upd, None, torch.ones((), device=DEV), 0.5, 0.0, 0.0, 1.0, False)
    assert same(w_upd[:direct], ref["w_new"])
    assert torch.equal(w_upd[direct:], w_dev[direct:])  # rows from `direct` on are untouched

    # the f32 tiles give the same bits where the call has an f32 form
    monkeypatch.setenv("NNUE_FTM_BF16", "0")
    assert L.nnue_ftm_uses_bf16(0, b, f, p, l1) == 0 and L.nnue_ftm_uses_bf16(1, b, f, p, l1) == 0
    assert torch.equal(lib.ftm_forward(w_dev, bias_dev, fm), out)
    assert torch.equal(lib.ftm_backward_weight(d_dev, fm)[0][:direct], d_w[:direct])
