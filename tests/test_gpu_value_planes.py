"""The merged FeatureTransformer backward's 32 x 64 value tiles fed the table as pre-split bf16 planes: the writer
(nnue_ftm_conv_binarize_value_planes: rider workgroups of the conv launch) and the reader (nnue_ftm_backward_planes:
gemm_tile_val_planes in ftm_backward_bf_kernel<64, 32, 64, 128, false, true, ValStePlanesEpi>).  ``-m gpu``.

References: the plane contents against the table itself (the split is exact); the tile against float64 restated from the
launch's own inputs (tests/ste_ride_cases.py) at the ride's bar, 2e-5 * max|ref| per tensor, and against the same call with
NNUE_FTM_VAL_PLANES=0 (today's f32 tiles) for the outputs whose tile families are unchanged.  Shapes and helpers:
tests/value_planes_cases.py."""
import ctypes

import pytest
import torch

import nnue
import nnue_oracle as orc
import ste_ride_cases as ride
import value_planes_cases as vpc
from conftest import assert_close_grad
from nnue_hip import lib
from nnue_hip.trainer import NnueTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLANES_KERNEL = "ftm_backward_bf_kernel<64, 32, 64, 128, false, true, (anonymous namespace)::ValStePlanesEpi>"
F32_KERNEL = "ftm_backward_bf_kernel<64, 32, 64, 128, false, true, (anonymous namespace)::ValSteEpi>"
_CASES = {}


@pytest.fixture(autouse=True)
def small_shapes_take_the_path(monkeypatch):
    monkeypatch.setenv("NNUE_FTM_VAL_PLANES_MIN_TILES", "1")
    monkeypatch.setenv("NNUE_FTM_FWD_PLANES_MIN_WG", "1")
    for knob in ("NNUE_FTM_VAL_PLANES", "NNUE_FTM_FWD_PLANES", "NNUE_FTM_BF16", "NNUE_FTM_BF_WM", "NNUE_FTM_BF_BM"):
        monkeypatch.delenv(knob, raising=False)


def case(shape, grid=False):
    """A case, its planes and the results of the f32 tiles (knob 0) on it: built once, never modified."""
    key = (shape, grid)
    if key not in _CASES:
        import os
        c = vpc.build_case(shape, grid)
        assert vpc.supported(shape), f"{shape}: the value planes are not taken"
        c.vp = vpc.write_planes(c)
        os.environ["NNUE_FTM_VAL_PLANES"] = "0"  # read per call
        try:
            c.f32 = vpc.launch(c, c.vp, riders=True)
        finally:
            del os.environ["NNUE_FTM_VAL_PLANES"]
        c.ref_thr, c.ref_w, c.ref_val = ride.float64_reference(c)
        _CASES[key] = c
    return _CASES[key]


# ------------------------------------------------------------------ 1. plane contents
@pytest.mark.parametrize("shape", vpc.PLANE_SHAPES, ids=vpc.shape_id)
def test_plane_contents_and_the_rest_of_the_conv_launch(shape):
    b, h, w, stride, l1, f, l2 = shape
    gh, gw = (h - 1) // stride + 1, (w - 1) // stride + 1
    g, p = gh * gw, 8 * gh * gw
    assert lib.ftm_value_planes_supported(b, f, p, l1, h, w, stride) and lib.ftm_forward_l1_planes_supported(b, f, p, l1, l2), shape
    gen = torch.Generator().manual_seed(1000 * b + f)
    images, conv_w, thr = torch.randn(b, 3, h, w, generator=gen).to(DEV), (0.3 * torch.randn(8, 3, 3, 3, generator=gen)).to(DEV), \
        (0.1 * torch.randn(8, generator=gen)).to(DEV)
    table = vpc.wide(gen, f, l1)  # exponents over [-125, 125]: to the edge of the normal range

    def run(wrap=lambda t: t, value=True):
        planes = wrap(torch.full((lib.ftm_forward_planes_bytes(b, f, p, l1),), 0xFF, dtype=torch.uint8, device=DEV))
        vp = wrap(torch.full((lib.ftm_value_planes_bytes(b, f, p, l1),), 0xFF, dtype=torch.uint8, device=DEV)) if value else None
        conv_out = wrap(torch.full((b, 8, gh, gw), float("nan"), device=DEV))
        fm0 = lib.FeatureMatrix.empty(b, p, f, l1, DEV)
        fm0.bits.fill_(0xFF)
        fm = lib.FeatureMatrix(wrap(fm0.bits), wrap(fm0.n), wrap(fm0.sink), fm0.scratch, p, f)
        lib.ftm_conv_binarize_planes(wrap(images), wrap(conv_w), wrap(thr), stride, wrap(table.to(DEV)), l2, planes, conv_out=conv_out, fm=fm,
                                     val_planes=vp)
        torch.cuda.synchronize()
        return conv_out, fm, planes, vp

    conv_ref, fm_ref, planes_ref, _ = run(value=False)  # nnue_ftm_conv_binarize_planes
    conv_out, fm, planes, vp = run()
    assert torch.equal(conv_out, conv_ref) and torch.equal(fm.bits, fm_ref.bits) and torch.equal(fm.n, fm_ref.n) and torch.equal(fm.sink, fm_ref.sink)
    assert torch.equal(planes, planes_ref), "the forward planes are those of nnue_ftm_conv_binarize_planes"
    vals, rows = vpc.decode_planes(vp, g, f, l1)
    k_pad = vals.shape[-1]
    want = torch.zeros((rows.shape[0], 64, k_pad))
    want[:, :, :l1] = table[rows]
    total = (vals[2] + vals[1]) + vals[0]
    big = want.abs() >= 2.0 ** -100  # below it a part is a bf16 denormal the truncation cuts: less than the smallest normal float is lost
    assert torch.equal(total[big], want[big]), "hi + mid + lo is the table element of the clamped row, bit for bit"
    assert float((total.double() - want.double()).abs().max()) < 2.0 ** -126
    assert not bool(vals[:, :, :, l1:].any()), "j >= L1 are zeros in every plane"
    assert torch.equal(vals[0].view(torch.int32)[big], want.view(torch.int32)[big] & -65536), "hi is the truncation to bf16"
    # the clamps, stated on their own: grid positions past G read position G - 1, map positions from F - 1 on row F - 1
    tn, n = torch.meshgrid(torch.arange(rows.shape[0]), torch.arange(64), indexing="ij")
    past = tn * 8 + (n & 7) >= g
    assert torch.equal(rows[past], torch.clamp((n[past] >> 3) * g + g - 1, max=f - 1))
    assert bool((rows[(n >> 3) * g + torch.clamp(tn * 8 + (n & 7), max=g - 1) >= f - 1] == f - 1).all()) and int(rows.max()) <= f - 1
    # a second launch is bitwise the first; behind guard bands nothing else is written
    assert torch.equal(run()[3], vp)
    band = ride.Banded()
    g_conv, g_fm, g_planes, g_vp = run(wrap=band)
    assert torch.equal(g_vp, vp) and torch.equal(g_planes, planes) and torch.equal(g_conv, conv_out) and torch.equal(g_fm.bits, fm.bits)
    assert band.untouched(), "a guard band round the table, the planes or the conv launch's outputs was written"


# ------------------------------------------------------------------ 2. the tile
@pytest.mark.parametrize("shape", vpc.TILE_SHAPES, ids=vpc.shape_id)
def test_randn_operands_against_float64_and_the_f32_tiles(shape, capsys):
    c = case(shape)
    chunks = ride.ste_chunks(shape)
    got = vpc.launch(c, c.vp, riders=True)
    assert bool(torch.isfinite(got["part"]).all()), "every partial slot is written"
    d_thr, d_w = ride.partial_sums(got["part"], chunks)
    ratios = {"d_thr": ride.ratio(d_thr, c.ref_thr), "d_w": ride.ratio(d_w, c.ref_w), "d_conv_out": ride.ratio(got["d_v"].view(c.ref_val.shape), c.ref_val)}
    with capsys.disabled():
        print(f"\n  {vpc.shape_id(shape)}: " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()) + f" (bar {ride.RTOL:.0e})", end="")
    assert bool(torch.isfinite(got["d_v"]).all()) and not bool(got["d_v"].cpu()[~c.bits.bool()].any()), "exact zeros at inactive positions"
    assert_close_grad(got["d_v"].view(c.ref_val.shape), c.ref_val, "d_conv_out", rtol=ride.RTOL)
    assert_close_grad(d_w, c.ref_w, "d_weight (conv)", rtol=ride.RTOL)
    assert_close_grad(d_thr, c.ref_thr, "d_thr", rtol=ride.RTOL)
    # the tile families that did not change: bitwise the launch with the knob at 0
    for k in ("d_w", "d_b", "sq", "d_w1"):
        assert (got[k] is None) == (c.f32[k] is None)
        if got[k] is not None:
            assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], c.f32[k]), f"{k} differs from the launch with NNUE_FTM_VAL_PLANES=0"
    # without dst the partials keep their bits; a second run is bitwise the first
    again = vpc.launch(c, c.vp, dst=False)
    assert again["d_v"] is None and torch.equal(again["part"], got["part"])
    # guard bands round every operand, the planes and every output
    band = ride.Banded()
    vp_g = vpc.write_planes(c, band)
    assert torch.equal(vp_g, c.vp)
    guarded = vpc.launch(c, vp_g, band=band, riders=True)
    for k, v in got.items():
        assert v is None or torch.equal(guarded[k], v), f"{k} differs behind guard bands"
    assert band.untouched(), "a guard band was written"


@pytest.mark.parametrize("shape", vpc.TILE_SHAPES, ids=vpc.shape_id)
def test_grid_operands_equal_float64(shape):
    """d_out and the table on a 2^-6 grid: every sum of the value product is exact in float32 in any order and the split is
    exact, so d_conv_out equals the float64 value (the partials also contract pixels and the sigmoid's slope: not exact)."""
    c = case(shape, grid=True)
    assert float(c.ref_val.abs().max()) * 4096 < 2 ** 24 and bool((c.ref_val * 4096 == (c.ref_val * 4096).round()).all())
    got = vpc.launch(c, c.vp)
    wrong = got["d_v"].view(c.ref_val.shape).cpu().double() != c.ref_val
    assert not bool(wrong.any()), f"d_conv_out: {int(wrong.sum())} of {wrong.numel()} elements differ from float64"
    assert torch.equal(got["d_v"], c.f32["d_v"]), "the f32 tiles give the same exact values"
    assert bool(torch.isfinite(got["part"]).all())


# ------------------------------------------------------------------ 3. which kernel ran
def backward_kernels(c):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        vpc.launch(c, c.vp)
    found = []
    for name in (e.name for e in prof.events()):
        at = name.find("ftm_backward_bf_kernel<")
        if at < 0:
            continue
        depth, end = 0, at
        for end in range(at, len(name)):
            depth += (name[end] == "<") - (name[end] == ">")
            if name[end] == ">" and depth == 0:
                break
        found.append(name[at:end + 1])
    return found


def test_which_kernel_serves_the_call(monkeypatch):
    shape = (37, 31, 31, 3, 136)
    c = case(shape)
    assert backward_kernels(c) == [PLANES_KERNEL]
    monkeypatch.setenv("NNUE_FTM_VAL_PLANES", "0")
    assert not vpc.supported(shape) and backward_kernels(c) == [F32_KERNEL]
    monkeypatch.delenv("NNUE_FTM_VAL_PLANES")
    odd = (37, 31, 31, 3, 132)  # L1 % 8 == 4
    assert not vpc.supported(odd) and ride.ste_chunks(odd) > 0
    c4 = vpc.build_case(odd)
    c4.vp = c.vp  # a valid buffer the launch must not read
    assert backward_kernels(c4) == [F32_KERNEL]
    monkeypatch.delenv("NNUE_FTM_VAL_PLANES_MIN_TILES")  # the policy floor: one value tile per CU
    assert not vpc.supported(shape) and vpc.supported(ride.C2) and backward_kernels(c) == [F32_KERNEL]
    assert lib.load().nnue_ftm_uses_bf16(5, 512, 800, 968, 1024) == 1 and lib.load().nnue_ftm_uses_bf16(5, 37, 968, 968, 136) == 0


# ------------------------------------------------------------------ 4. argument checks
def test_argument_checks_return_codes_without_launching():
    shape = (37, 31, 31, 3, 136)
    c = case(shape)
    b, h, w, stride, l1, f, p, gh, gw = ride.geometry(shape)
    L, d = lib.load(), c.dev
    need = lib.ftm_value_planes_bytes(b, f, p, l1)
    assert need == 16 * 2 * vpc.BLOCK
    vp = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    conv_out = torch.full((b, 8, gh, gw), float("nan"), device=DEV)
    fm = lib.FeatureMatrix.empty(b, p, f, l1, DEV)
    fm.bits.fill_(0xFF)
    part = torch.full((8 * 28 * ride.ste_chunks(shape),), float("nan"), device=DEV)
    d_w, d_b = torch.full((f, l1), float("nan"), device=DEV), torch.full((l1,), float("nan"), device=DEV)
    ptr = lambda t: t.data_ptr()  # noqa: E731

    def conv(vp_ptr, vp_bytes, ll1=l1):
        return L.nnue_ftm_conv_binarize_value_planes(ptr(d["images"]), ptr(d["images"]), ptr(d["thr"]), b, h, w, 8, stride, f, ptr(d["weight"]), ll1, 0,
                                                     None, 0, vp_ptr, vp_bytes, ptr(conv_out), ptr(fm.bits), ptr(fm.n), ptr(fm.sink), None)

    def bwd(vp_ptr, vp_bytes):
        return L.nnue_ftm_backward_planes(ptr(c.fm.bits), ptr(c.fm.sink), ptr(d["d_out"]), ptr(d["weight"]), b, f, p, l1, ptr(d_w), ptr(d_b), None,
                                          None, None, 0, None, None, None, ptr(d["images"]), None, ptr(d["conv_out"]), ptr(d["thr"]), h, w, stride,
                                          ptr(part), part.numel() * 4, vp_ptr, vp_bytes, None)

    assert conv(None, need) == -1 and b"null pointer" in L.nnue_hip_last_error()
    assert bwd(None, need) == -1 and b"null pointer" in L.nnue_hip_last_error()
    assert conv(ptr(vp), need - vpc.BLOCK) == -4 and b"value-plane buffer" in L.nnue_hip_last_error()
    assert bwd(ptr(vp), need - vpc.BLOCK) == -4 and b"value-plane buffer" in L.nnue_hip_last_error()
    assert conv(ptr(vp) + 4, need) == -1 and b"aligned" in L.nnue_hip_last_error()
    assert bwd(ptr(vp) + 4, need) == -1 and b"aligned" in L.nnue_hip_last_error()
    assert conv(ptr(vp), need, ll1=132) == -2 and b"value-planes shape" in L.nnue_hip_last_error()  # a shape not taken
    torch.cuda.synchronize()
    assert bool((vp == 0xFF).all()) and bool((fm.bits == 0xFF).all()) and bool(torch.isnan(conv_out).all())
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(d_w).all()) and bool(torch.isnan(d_b).all())
    assert isinstance(ctypes.c_void_p(ptr(vp)).value, int)


# ------------------------------------------------------------------ 5. the trainer
OPT = dict(lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0)
SMALL = tuple(f"classifier.classifier.{i}.{n}" for i in (0, 2, 4) for n in ("weight", "bias")) + ("input.weight", "input.bias")


def fresh_trainer(batch, use_graph):
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 1024, 128, 32, num_classes=10, input_size=32)  # the C2 architecture
    return NnueTrainer(model.to(DEV), batch, (32, 32), use_graph=use_graph, input_slots=3, **OPT)


def three_steps(batch, form, batches):
    tr = fresh_trainer(batch, form != "eager")
    first = None
    if form == "many":
        for s, (images, labels) in enumerate(batches):
            tr.inputs[s][0].copy_(images)
            tr.inputs[s][1].copy_(labels)
        tr.step(slot=0)
        first = {k: v.clone() for k, v in tr.layout.views(tr.flat_grads).items()}
        tr.step_many((1, 2))
    else:
        for s, (images, labels) in enumerate(batches):
            tr.step(images.to(DEV), labels.to(DEV), slot=s)
            if s == 0:
                first = {k: v.clone() for k, v in tr.layout.views(tr.flat_grads).items()}
    torch.cuda.synchronize()
    return tr, first


@pytest.mark.parametrize("batch", (64, 160))  # 64: the value planes alone; 160: beside the forward's planes
def test_trainer_steps_with_and_without_the_value_planes(batch, monkeypatch):
    for knob in ("NNUE_FT_PATH", "NNUE_FUSE_L1", "NNUE_CONV_PATCHES", "NNUE_FTM_RIDE_STE"):
        monkeypatch.delenv(knob, raising=False)
    gen = torch.Generator().manual_seed(81)
    batches = [(torch.randn(batch, 3, 32, 32, generator=gen), torch.randint(0, 10, (batch,), generator=gen)) for _ in range(3)]
    results = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("NNUE_FTM_VAL_PLANES", knob)
        for form in ("eager", "graph", "many"):
            tr, first = three_steps(batch, form, batches)
            assert tr.ride_ste and (tr.val_planes is not None) == (knob == "1") and tr.fwd_planes == (batch == 160)
            if knob == "1":
                assert tr.val_planes.numel() == lib.ftm_value_planes_bytes(batch, tr.F, tr.P, tr.L1)
            if form != "eager":
                names = [c[0] for c in tr._plan_seg["front"]] + [c[0] for c in tr._plan_seg["ft_wgrad"]]
                want = ("nnue_ftm_conv_binarize_value_planes", "nnue_ftm_backward_planes")
                assert all((n in names) == (knob == "1") for n in want), names
            again, _ = three_steps(batch, form, batches)
            assert torch.equal(again.flat_params, tr.flat_params), f"knob {knob}, {form}: a second run differs"
            results[knob, form] = (tr.flat_params.clone(), first, tr.layout)
    for knob in ("0", "1"):  # the launch forms agree bit for bit
        assert torch.equal(results[knob, "graph"][0], results[knob, "eager"][0]) and torch.equal(results[knob, "many"][0], results[knob, "eager"][0])
    # first step: the same forward, so everything but the value product's consumers (threshold, conv weights) keeps its bits
    for k in SMALL:
        assert torch.equal(results["1", "eager"][1][k], results["0", "eager"][1][k]), f"step 0 grad {k} differs between the knobs"
    layout = results["0", "eager"][2]
    p0, p1 = layout.views(results["0", "eager"][0]), layout.views(results["1", "eager"][0])
    for k in orc.TRAINABLE_KEYS:  # the whole-step bar of tests/conftest.py
        assert_close_grad(p1[k], p0[k], f"three steps, {k}")
