"""The fused FeatureTransformer forward fed the table as pre-split bf16 planes: nnue_ftm_conv_binarize_planes (the conv launch
whose rider workgroups write the planes) + nnue_ftm_forward_l1_planes (the 32-row bf16 tiles reading them).  ``-m gpu``.

The reference is a kernel already in the tree: the stand-alone nnue_ftm_forward_l1 under NNUE_FTM_BF_BM=32 stages the same
three images from the table itself and contracts them with the same code, so ``out`` and the layer-1 slabs must be equal bit
for bit; conv_out, bits, n and sink must be those of nnue_ftm_conv_binarize.  The policy takes the path from 256 workgroups up
(the CIFAR batch-512 shape); NNUE_FTM_FWD_PLANES_MIN_WG=1 (read per call) lets the small shapes below reach the same kernels.

Shapes (B, F, L1, L2, fps, H = W, stride); P = fps * Gh * Gw:
  (256, 801, 128, 128, 8, 10, 1)  P 800: K tail of 32 rows, a single column tile, 128-thread conv workgroups (two riders per block)
  (250, 300, 256, 128, 8,  7, 1)  P 392: ragged last row tile, clamp sink, direct = 299 ends inside a 16-byte chunk of 8 k;
                                  64-thread conv workgroups (four riders per block)
  (512, 129, 256, 128, 8,  4, 1)  P 128: one full K tile plus one row
  (160, 200, 128,  64, 2, 24, 1)  P 1152: 256-thread conv workgroups (one rider per block) and two slices per sample (added:
                                  the flat grid's sample / slice arithmetic and the one-rider form are not reached by the others)
"""
import os

import pytest
import torch

import nnue
import nnue_oracle as orc
from conftest import assert_close_grad, assert_close_logits
from nnue_hip import lib
from nnue_hip.trainer import NnueTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = ((256, 801, 128, 128, 8, 10, 1), (250, 300, 256, 128, 8, 7, 1), (512, 129, 256, 128, 8, 4, 1), (160, 200, 128, 64, 2, 24, 1))
BLOCK = 3 * 64 * 128 * 2  # bytes of one (column tile, K tile) block
BAND = 4096
_CASES = {}


@pytest.fixture(autouse=True)
def small_shapes_take_the_path(monkeypatch):
    monkeypatch.setenv("NNUE_FTM_FWD_PLANES_MIN_WG", "1")
    monkeypatch.delenv("NNUE_FTM_FWD_PLANES", raising=False)
    monkeypatch.delenv("NNUE_FTM_BF_BM", raising=False)


def geometry(shape):
    b, f, l1, l2, fps, hw, stride = shape
    g = (hw - 1) // stride + 1
    p = fps * g * g
    return b, f, p, l1, l2, fps, hw, stride, min(f - 1, p)


# ---- the layout, restated once: byte offset of bf16 (plane, column n of tile_n, row k_local of K tile kt) and its table column
def plane_byte(tile_n, kt, plane, n, k_local, ktiles):
    return ((tile_n * ktiles + kt) * 3 + plane) * 16384 + n * 256 + (((k_local >> 3) ^ (n & 15)) << 4) + (k_local & 7) * 2


def plane_col(tile_n, n, l1):
    return 32 * tile_n + (n & 31) + (l1 // 2) * ((n >> 5) & 1)


def decode_planes(planes, direct, l1):
    """[3][ktiles * 128][L1] float32: plane p of table element (k, c), read through plane_byte / plane_col."""
    ktiles, tiles_n = (direct + 127) // 128, l1 // 64
    assert planes.numel() == tiles_n * ktiles * BLOCK
    tn, kt, pl, n, kl = torch.meshgrid(torch.arange(tiles_n), torch.arange(ktiles), torch.arange(3), torch.arange(64), torch.arange(128),
                                       indexing="ij")
    halves = planes.cpu().view(torch.int16)[plane_byte(tn, kt, pl, n, kl, ktiles) // 2]
    vals = (halves.to(torch.int32) << 16).view(torch.float32)
    out = torch.full((3, ktiles * 128, l1), float("nan"))
    out[pl, kt * 128 + kl, plane_col(tn, n, l1)] = vals
    assert not bool(torch.isnan(out).any()), "the index function reaches every (plane, row, column)"
    return out


def wide(gen, *shape, span=100):  # random sign, exponent uniform in [-span, span], full 24-bit mantissa
    mant = 1.0 + torch.rand(*shape, generator=gen, dtype=torch.float64)
    e = torch.randint(-span, span + 1, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * mant * torch.exp2(e)).float()


def case(shape):
    """Device inputs of a shape and the reference results of the kernels already in the tree; built once, never modified."""
    if shape in _CASES:
        return _CASES[shape]
    b, f, p, l1, l2, fps, hw, stride, direct = geometry(shape)
    gen = torch.Generator().manual_seed(1000 * b + f)
    c = dict(images=torch.randn(b, 3, hw, hw, generator=gen), conv_w=0.3 * torch.randn(fps, 3, 3, 3, generator=gen),
             thr=0.1 * torch.randn(fps, generator=gen), table=0.05 * torch.randn(f, l1, generator=gen), bias=torch.randn(l1, generator=gen),
             w1=0.1 * torch.randn(l2, l1, generator=gen))
    c = {k: v.to(DEV) for k, v in c.items()}
    assert lib.ftm_forward_l1_planes_supported(b, f, p, l1, l2), shape
    c["conv_ref"], c["fm_ref"] = lib.ftm_conv_binarize(c["images"], c["conv_w"], c["thr"], stride, f, l1)
    old = os.environ.get("NNUE_FTM_BF_BM")
    os.environ["NNUE_FTM_BF_BM"] = "32"  # read per call: the 32-row bf16 tiles of the stand-alone fused forward
    try:
        assert lib.load().nnue_ftm_uses_bf16(0, b, f, p, l1) == 1
        c["part_ref"] = torch.full(((l1 // 64) * b * l2,), float("nan"), device=DEV)
        c["out_ref"] = lib.ftm_forward_l1(c["table"], c["bias"], c["fm_ref"], c["w1"], c["part_ref"])
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ["NNUE_FTM_BF_BM"]
        else:
            os.environ["NNUE_FTM_BF_BM"] = old
    assert bool(torch.isfinite(c["out_ref"]).all()) and bool(torch.isfinite(c["part_ref"]).all())
    _CASES[shape] = c
    return c


class Banded:
    """Tensors as interior views (16-byte aligned) of buffers whose surroundings hold NaN (floats) or 0xFF (bytes / ints)."""

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


def run(shape, c, wrap=lambda t: t, table=None):
    """conv_binarize_planes + forward_l1_planes on fresh NaN / 0xFF-prefilled outputs; returns (conv_out, fm, planes, out, part)."""
    b, f, p, l1, l2, fps, hw, stride, direct = geometry(shape)
    g = (hw - 1) // stride + 1
    table = wrap(c["table"] if table is None else table)
    planes = wrap(torch.full((lib.ftm_forward_planes_bytes(b, f, p, l1),), 0xFF, dtype=torch.uint8, device=DEV))
    conv_out = wrap(torch.full((b, fps, g, g), float("nan"), device=DEV))
    fm0 = lib.FeatureMatrix.empty(b, p, f, l1, DEV)
    fm0.bits.fill_(0xFF)
    fm = lib.FeatureMatrix(wrap(fm0.bits), wrap(fm0.n), wrap(fm0.sink), fm0.scratch, p, f)
    out = wrap(torch.full((b, l1), float("nan"), device=DEV))
    part = wrap(torch.full(((l1 // 64) * b * l2,), float("nan"), device=DEV))
    w1, bias = wrap(c["w1"]), wrap(c["bias"])
    lib.ftm_conv_binarize_planes(wrap(c["images"]), wrap(c["conv_w"]), wrap(c["thr"]), stride, table, l2, planes, conv_out=conv_out, fm=fm)
    lib.ftm_forward_l1_planes(table, bias, fm, planes, w1, part, out=out)
    torch.cuda.synchronize()
    return conv_out, fm, planes, out, part


def assert_is_reference(c, got):
    conv_out, fm, _, out, part = got
    ref = c["fm_ref"]
    assert torch.equal(conv_out, c["conv_ref"]) and torch.equal(fm.bits, ref.bits), "conv_out / bits are nnue_ftm_conv_binarize's"
    assert torch.equal(fm.n, ref.n) and torch.equal(fm.sink, ref.sink), "n / sink are nnue_ftm_conv_binarize's"
    assert torch.equal(out, c["out_ref"]), f"out: max diff {float((out - c['out_ref']).abs().max()):.3e}"
    assert torch.equal(part, c["part_ref"]), f"layer-1 slabs: max diff {float((part - c['part_ref']).abs().max()):.3e}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bitwise_the_kernels_in_the_tree_twice_and_behind_guard_bands(shape):
    c = case(shape)
    first = run(shape, c)
    assert_is_reference(c, first)
    again = run(shape, c)  # determinism: a second run is bitwise the first, the plane buffer included
    assert_is_reference(c, again)
    assert torch.equal(again[2], first[2])
    band = Banded()
    guarded = run(shape, c, wrap=band)
    assert_is_reference(c, guarded)
    assert torch.equal(guarded[2], first[2]), "the planes behind guard bands are those of the plain allocation"
    assert band.untouched(), "a guard band was written"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plane_contents(shape):
    """hi + mid + lo (added smallest first) is the table element exactly, over the exponent range; rows k >= direct are zero."""
    b, f, p, l1, l2, fps, hw, stride, direct = geometry(shape)
    c = case(shape)
    table = wide(torch.Generator().manual_seed(f), f, l1)
    _, _, planes, _, _ = run(shape, c, table=table.to(DEV))
    pl = decode_planes(planes, direct, l1)
    total = (pl[2] + pl[1]) + pl[0]
    assert torch.equal(total[:direct], table[:direct]), "the three planes add up to the table element exactly"
    assert not bool(pl[:, direct:].any()), "rows from `direct` on are zeros in every plane"
    # each plane is a truncation: hi carries the element's top 16 bits
    assert torch.equal(pl[0][:direct].view(torch.int32), table[:direct].view(torch.int32) & -65536)


def test_argument_checks_return_codes_without_launching():
    shape = SHAPES[1]
    b, f, p, l1, l2, fps, hw, stride, direct = geometry(shape)
    c = case(shape)
    L = lib.load()
    g = (hw - 1) // stride + 1
    need = lib.ftm_forward_planes_bytes(b, f, p, l1)
    planes = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    conv_out = torch.full((b, fps, g, g), float("nan"), device=DEV)
    fm = lib.FeatureMatrix.empty(b, p, f, l1, DEV)
    fm.bits.fill_(0xFF)
    out = torch.full((b, l1), float("nan"), device=DEV)
    part = torch.full(((l1 // 64) * b * l2,), float("nan"), device=DEV)
    ptr = lambda t: t.data_ptr()  # noqa: E731

    def conv(planes_ptr, planes_bytes, bb=b):
        return L.nnue_ftm_conv_binarize_planes(ptr(c["images"]), ptr(c["conv_w"]), ptr(c["thr"]), bb, hw, hw, fps, stride, f, ptr(c["table"]), l1, l2,
                                               planes_ptr, planes_bytes, ptr(conv_out), ptr(fm.bits), ptr(fm.n), ptr(fm.sink), None)

    def fwd(planes_ptr, planes_bytes, bb=b, table_ptr=None):
        return L.nnue_ftm_forward_l1_planes(ptr(fm.bits), ptr(fm.sink), planes_ptr, planes_bytes, table_ptr or ptr(c["table"]), ptr(c["bias"]),
                                            ptr(c["w1"]), bb, f, p, l1, l2, ptr(out), ptr(part), None)

    # a plane buffer one block short
    assert conv(ptr(planes), need - BLOCK) == -4 and b"plane buffer" in L.nnue_hip_last_error()
    assert fwd(ptr(planes), need - BLOCK) == -4 and b"plane buffer" in L.nnue_hip_last_error()
    # a misaligned pointer
    assert conv(ptr(planes) + 4, need) == -1 and b"aligned" in L.nnue_hip_last_error()
    assert fwd(ptr(planes) + 4, need) == -1 and b"aligned" in L.nnue_hip_last_error()
    assert fwd(ptr(planes), need, table_ptr=ptr(c["table"]) + 4) == -1
    # an unsupported shape: a batch one 128-row tile covers is a split-K forward
    assert not lib.ftm_forward_l1_planes_supported(64, f, p, l1, l2)
    assert conv(ptr(planes), need, bb=64) == -2 and fwd(ptr(planes), need, bb=64) == -2
    # null pointers
    assert conv(None, need) == -1 and fwd(None, need) == -1
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((planes == 0xFF).all()) and bool((fm.bits == 0xFF).all())
    assert bool(torch.isnan(conv_out).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(part).all())


def test_the_policy_floor_without_the_override(monkeypatch):
    monkeypatch.delenv("NNUE_FTM_FWD_PLANES_MIN_WG")
    assert lib.ftm_forward_l1_planes_supported(512, 800, 968, 1024, 128)       # the CIFAR batch-512 shape
    assert not lib.ftm_forward_l1_planes_supported(256, 801, 800, 128, 128)    # 16 workgroups


# ------------------------------------------------------------------ trainer
TR = dict(grid=10, fps=8, image=32, l1=256, l2=32, l3=16, classes=10, batch=256)
OPT = dict(lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0)


def fresh_trainer(use_graph, slots=3):
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(TR["grid"], TR["fps"]), TR["l1"], TR["l2"], TR["l3"], num_classes=TR["classes"], input_size=TR["image"])
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return params, NnueTrainer(model.to(DEV), TR["batch"], (TR["image"], TR["image"]), use_graph=use_graph, input_slots=slots, **OPT)


def test_trainer_takes_the_planes_path_and_follows_the_oracle(monkeypatch):
    """Three optimizer steps with the knob on against oracle.loss_and_grads_explicit + oracle.sgd_step (the bars of
    tests/conftest.py; batches drawn away from the step's discontinuities as tests/test_gpu_step_shapes.py does), then the same
    three batches eagerly, as single-step graphs and as step + step_many: bitwise each other."""
    from test_gpu_step_shapes import clean_batch
    for knob in ("NNUE_FT_PATH", "NNUE_FUSE_L1", "NNUE_CONV_PATCHES"):  # the default path, whatever the environment holds
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("NNUE_FTM_FWD_PLANES", "0")
    assert not fresh_trainer(False, 1)[1].fwd_planes, "NNUE_FTM_FWD_PLANES=0 keeps the two plain calls"
    monkeypatch.setenv("NNUE_FTM_FWD_PLANES", "1")
    params, tr = fresh_trainer(True)
    assert tr.fuse_l1 and tr.fwd_planes and tr.planes.numel() == lib.ftm_forward_planes_bytes(tr.B, tr.F, tr.P, tr.L1)
    stride = orc.conv_stride(TR["image"], TR["grid"])
    gen = torch.Generator().manual_seed(79)
    bufs, batches = {}, []
    for s in range(3):
        images, labels = clean_batch(TR, params, stride, gen)
        batches.append((images, labels))
        ref_logits, ref_loss, ref_grads, keep = orc.loss_and_grads_explicit(params, images, labels, stride, None)
        orc.sgd_step(params, ref_grads, bufs, OPT["lr"], OPT["momentum"], OPT["weight_decay"], OPT["max_grad_norm"])
        loss = tr.step(images.to(DEV), labels.to(DEV), slot=s)
        torch.cuda.synchronize()
        assert "nnue_ftm_forward_l1_planes" in [c[0] for c in tr._plan_seg["forward"]]
        assert "nnue_ftm_conv_binarize_planes" in [c[0] for c in tr._plan_seg["front"]]
        assert tr.active_stats()[1] == int(keep["n"].max()), "feature counts differ"
        assert_close_logits(tr.logits, ref_logits, f"step {s} logits")
        assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss))), (s, float(loss), float(ref_loss))
        got = tr.layout.views(tr.flat_grads)
        for k, ref in ref_grads.items():
            assert_close_grad(got[k], ref, f"step {s} grad {k}")
        for k in orc.TRAINABLE_KEYS:
            assert_close_grad(tr.p[k], params[k], f"step {s} {k}")
    graph_params = tr.flat_params.clone()
    _, eager = fresh_trainer(False)
    for s, (images, labels) in enumerate(batches):
        eager.step(images.to(DEV), labels.to(DEV), slot=s)
    _, many = fresh_trainer(True)
    for s, (images, labels) in enumerate(batches):
        many.inputs[s][0].copy_(images)
        many.inputs[s][1].copy_(labels)
    many.step(slot=0)
    many.step_many((1, 2))
    torch.cuda.synchronize()
    assert ((1, 2), "many") in many._g_local and eager.fwd_planes and many.fwd_planes
    assert torch.equal(eager.flat_params, graph_params), "eager and single-step graphs differ"
    assert torch.equal(many.flat_params, graph_params), "step_many and single-step graphs differ"
