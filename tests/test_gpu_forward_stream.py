"""The planes-fed fused forward with the table operand streamed from the plane buffer straight into the MFMA's operand registers
(ftm_forward_l1_stream_kernel behind nnue_ftm_forward_l1_planes; waves 1 x 4, the map of up to seven K tiles staged up front).
``-m gpu``.

The reference is the kernel it replaces: NNUE_FTM_FWD_STREAM=0 (read per call) launches the LDS-staged ftm_forward_l1_planes_kernel
on the same planes and map.  Per output element both contract the same fragments in the same order, so ``out`` and the layer-1
slabs must be equal bit for bit (compared as int32 words: the wide-value case holds infinities and NaNs), every element written
over a prefill of one NaN bit pattern.  The stand-alone nnue_ftm_forward_l1 under NNUE_FTM_BF_BM=32 -- the reference of
tests/test_gpu_forward_planes.py -- is held to the same bits.  NNUE_FTM_FWD_PLANES_MIN_WG=1 lets the small shapes take the path.

Shapes (B, F, L1, L2, fps, H = W, stride); P = fps * Gh * Gw, direct = min(F - 1, P), K tiles = ceil(direct / 128):
  K tiles   1 (direct 128 = P, and 100 < P: clamp sink), 2 (199), 3 (299, ends inside a 16-byte chunk), 4 (500), 5 (600), 6 (700),
            7 (799 = F - 1 < P and 896), 8 (999: past the streamed kernel, both knob values launch the LDS-staged one)
  batch     1, 31, 32, 33 (second 16-row fragment empty / partly filled / full / a second row tile of one row), 250 (ragged last row
            tile), 160 and 256.  A batch of at most 128 rows is a split-K forward for the policy; NNUE_FTM_BF_BM=32 (read per call)
            gives those the 32-row tiles, so that the kernel is reached at the batch sizes themselves.
  columns   L1 128 (two column tiles, half = 64) and 256; L2 64 and 128 (4 and 8 layer-1 column tiles: wave + 4 s)
"""

import pytest
import torch

from nnue_hip import lib
from nnue_hip.trainer import NnueTrainer
from test_gpu_forward_planes import Banded, fresh_trainer, geometry, wide

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0x7FC0A5A5  # a NaN no kernel here produces: an element still holding it was not written

KT_SHAPES = (
    (160, 129, 128, 64, 8, 4, 1),    # direct 128 = P: one full K tile
    (160, 101, 128, 64, 8, 4, 1),    # direct 100 < P 128: one K tile, clamp sink
    (160, 200, 128, 64, 8, 5, 1),    # direct 199, P 200: two
    (250, 300, 256, 128, 8, 7, 1),   # direct 299, P 392: three, ends inside a chunk; ragged last row tile; L1 256, L2 128
    (160, 501, 128, 64, 8, 8, 1),    # direct 500, P 512: four
    (160, 601, 128, 128, 8, 9, 1),   # direct 600, P 648: five
    (160, 701, 256, 64, 8, 10, 1),   # direct 700, P 800: six
    (256, 800, 128, 128, 8, 10, 1),  # direct 799 = F - 1 < P 800: seven
    (160, 897, 128, 64, 8, 11, 1),   # direct 896, P 968: seven full K tiles
    (160, 1000, 128, 64, 8, 12, 1),  # direct 999, P 1152: eight -- the LDS-staged kernel under both knob values
)
SMALL_B = tuple((b, 300, 128, 64, 8, 7, 1) for b in (1, 31, 32, 33))  # three K tiles
SHAPE_ID = lambda s: "x".join(map(str, s))  # noqa: E731
_CASES = {}


@pytest.fixture(autouse=True)
def small_shapes_take_the_path(monkeypatch):
    monkeypatch.setenv("NNUE_FTM_FWD_PLANES_MIN_WG", "1")
    for knob in ("NNUE_FTM_FWD_PLANES", "NNUE_FTM_FWD_STREAM", "NNUE_FTM_BF_BM"):
        monkeypatch.delenv(knob, raising=False)


def filled(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int32).fill_(FILL)
    return t


def words(t):
    return t.contiguous().view(torch.int32)


def case(shape, monkeypatch, table_gen=None):
    """Inputs of a shape, the map and planes of one nnue_ftm_conv_binarize_planes call and the stand-alone 32-row bf16 forward's
    results; built once per (shape, table), never modified."""
    b, f, p, l1, l2, fps, hw, stride, direct = geometry(shape)
    if b <= 128:
        monkeypatch.setenv("NNUE_FTM_BF_BM", "32")  # for the test's own calls too
    key = (shape, table_gen is not None)
    if key in _CASES:
        return _CASES[key]
    assert lib.ftm_forward_l1_planes_supported(b, f, p, l1, l2), shape
    gen = torch.Generator().manual_seed(7000 * b + f)
    c = dict(images=torch.randn(b, 3, hw, hw, generator=gen), conv_w=0.3 * torch.randn(fps, 3, 3, 3, generator=gen),
             thr=0.1 * torch.randn(fps, generator=gen), bias=torch.randn(l1, generator=gen), w1=0.1 * torch.randn(l2, l1, generator=gen),
             table=0.05 * torch.randn(f, l1, generator=gen) if table_gen is None else table_gen(gen, f, l1))
    c = {k: v.to(DEV) for k, v in c.items()}
    c["planes"] = torch.full((lib.ftm_forward_planes_bytes(b, f, p, l1),), 0xFF, dtype=torch.uint8, device=DEV)
    _, c["fm"] = lib.ftm_conv_binarize_planes(c["images"], c["conv_w"], c["thr"], stride, c["table"], l2, c["planes"])
    monkeypatch.setenv("NNUE_FTM_BF_BM", "32")  # the stand-alone fused forward on the 32-row bf16 tiles
    c["part_ref"] = filled(((l1 // 64) * b * l2,))
    c["out_ref"] = lib.ftm_forward_l1(c["table"], c["bias"], c["fm"], c["w1"], c["part_ref"], out=filled((b, l1)))
    torch.cuda.synchronize()
    if b > 128:
        monkeypatch.delenv("NNUE_FTM_BF_BM")
    _CASES[key] = c
    return c


def forward(c, knob, monkeypatch, wrap=lambda t: t):
    b, l1, l2 = c["fm"].batch, c["table"].shape[1], c["w1"].shape[0]
    monkeypatch.setenv("NNUE_FTM_FWD_STREAM", knob)
    fm = c["fm"]
    fm = lib.FeatureMatrix(wrap(fm.bits), wrap(fm.n), wrap(fm.sink), fm.scratch, fm.positions, fm.num_rows)
    out, part = wrap(filled((b, l1))), wrap(filled(((l1 // 64) * b * l2,)))
    lib.ftm_forward_l1_planes(wrap(c["table"]), wrap(c["bias"]), fm, wrap(c["planes"]), wrap(c["w1"]), part, out=out)
    torch.cuda.synchronize()
    return out, part


def assert_same_bits(got, want, what):
    for name, g, w in zip(("out", "layer-1 slabs"), got, want):
        assert not bool((words(g) == FILL).any()), f"{what}: {name} has elements that were not written"
        differ = int((words(g) != words(w)).sum())
        assert differ == 0, f"{what}: {name} differs in {differ} of {g.numel()} words"


def check(shape, monkeypatch, table_gen=None):
    c = case(shape, monkeypatch, table_gen)
    ref = (c["out_ref"], c["part_ref"])
    staged = forward(c, "0", monkeypatch)
    streamed = forward(c, "1", monkeypatch)
    assert_same_bits(staged, ref, "NNUE_FTM_FWD_STREAM=0 against the stand-alone forward")
    assert_same_bits(streamed, staged, "NNUE_FTM_FWD_STREAM=1 against =0")
    assert_same_bits(forward(c, "1", monkeypatch), streamed, "a second call")
    return c, streamed


@pytest.mark.parametrize("shape", KT_SHAPES, ids=SHAPE_ID)
def test_every_k_tile_count_is_bitwise_the_staged_kernel(shape, monkeypatch):
    check(shape, monkeypatch)


@pytest.mark.parametrize("shape", SMALL_B, ids=SHAPE_ID)
def test_batches_inside_one_row_tile(shape, monkeypatch):
    check(shape, monkeypatch)


@pytest.mark.parametrize("shape", (KT_SHAPES[7], KT_SHAPES[3]), ids=SHAPE_ID)
def test_wide_table_values(shape, monkeypatch):
    """Exponents over +-100: the planes carry denormal lo terms, the sums and the pairwise products overflow -- same bits."""
    check(shape, monkeypatch, table_gen=lambda gen, f, l1: wide(gen, f, l1))


@pytest.mark.parametrize("shape", (KT_SHAPES[7], KT_SHAPES[3], KT_SHAPES[1], SMALL_B[0]), ids=SHAPE_ID)
def test_behind_guard_bands(shape, monkeypatch):
    c, plain = check(shape, monkeypatch)
    band = Banded()
    guarded = forward(c, "1", monkeypatch, wrap=band)
    assert_same_bits(guarded, plain, "operands as interior views of NaN / 0xFF-surrounded buffers")
    assert band.untouched(), "a guard band was written"


def test_the_knob_is_read_per_call_and_absent_means_streamed(monkeypatch):
    c = case(KT_SHAPES[7], monkeypatch)
    staged = forward(c, "0", monkeypatch)
    monkeypatch.delenv("NNUE_FTM_FWD_STREAM")
    b, l1, l2 = c["fm"].batch, c["table"].shape[1], c["w1"].shape[0]
    out, part = filled((b, l1)), filled(((l1 // 64) * b * l2,))
    lib.ftm_forward_l1_planes(c["table"], c["bias"], c["fm"], c["planes"], c["w1"], part, out=out)
    torch.cuda.synchronize()
    assert_same_bits((out, part), staged, "the policy (knob unset)")


def forward_kernels(c, knob, monkeypatch):
    """Names of the fused-forward kernels one nnue_ftm_forward_l1_planes call launched, as the profiler saw them."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        if knob is None:
            monkeypatch.delenv("NNUE_FTM_FWD_STREAM", raising=False)
            b, l1, l2 = c["fm"].batch, c["table"].shape[1], c["w1"].shape[0]
            lib.ftm_forward_l1_planes(c["table"], c["bias"], c["fm"], c["planes"], c["w1"], filled(((l1 // 64) * b * l2,)), out=filled((b, l1)))
            torch.cuda.synchronize()
        else:
            forward(c, knob, monkeypatch)
    names = [e.name for e in prof.events() if "ftm_forward_l1" in e.name and "kernel" in e.name]
    return ["stream" if "ftm_forward_l1_stream_kernel" in n else "staged" if "ftm_forward_l1_planes_kernel" in n else n for n in names]


@pytest.mark.parametrize("shape, policy", ((KT_SHAPES[1], "stream"), (KT_SHAPES[8], "stream"), (KT_SHAPES[9], "staged")), ids=("1tile", "7tiles", "8tiles"))
def test_which_kernel_serves_the_call(shape, policy, monkeypatch):
    """The comparisons above hold whichever kernel runs; this one reads the launched kernel's name off the profiler: the streamed
    kernel up to seven K tiles unless the knob is 0, the LDS-staged one for eight under every knob value."""
    c = case(shape, monkeypatch)
    assert forward_kernels(c, "0", monkeypatch) == ["staged"]
    assert forward_kernels(c, "1", monkeypatch) == [policy]
    assert forward_kernels(c, None, monkeypatch) == [policy]


# ------------------------------------------------------------------ trainer
def test_trainer_is_bitwise_the_staged_forward_eager_and_as_graphs(monkeypatch):
    """Three optimizer steps at a shape the path takes (F 801, P 800: seven K tiles), eagerly and as single-step hipGraphs, with the
    knob at 0 and at 1: logits and every parameter bitwise equal.  A captured graph holds the kernel chosen at capture, so each
    knob value has trainers of its own."""
    for knob in ("NNUE_FT_PATH", "NNUE_FUSE_L1", "NNUE_CONV_PATCHES"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("NNUE_FTM_FWD_PLANES", "1")
    gen = torch.Generator().manual_seed(83)
    probe = fresh_trainer(False, 1)[1]
    batches = [(torch.randn(probe.B, 3, 32, 32, generator=gen), torch.randint(0, 10, (probe.B,), generator=gen)) for _ in range(3)]
    assert probe.fwd_planes and (min(probe.F - 1, probe.P) + 127) // 128 <= 7
    results = {}
    for knob in ("0", "1"):
        for use_graph in (False, True):
            monkeypatch.setenv("NNUE_FTM_FWD_STREAM", knob)
            _, tr = fresh_trainer(use_graph)
            assert isinstance(tr, NnueTrainer) and tr.fwd_planes
            logits = []
            for s, (images, labels) in enumerate(batches):
                tr.step(images.to(DEV), labels.to(DEV), slot=s)
                torch.cuda.synchronize()
                assert "nnue_ftm_forward_l1_planes" in [call[0] for call in tr._plan_seg["forward"]]
                logits.append(tr.logits.clone())
            results[knob, use_graph] = (torch.stack(logits), tr.flat_params.clone())
    want_logits, want_params = results["0", False]
    assert bool(torch.isfinite(want_logits).all()) and bool(torch.isfinite(want_params).all())
    for key, (got_logits, got_params) in results.items():
        assert torch.equal(words(got_logits), words(want_logits)), f"logits of (knob, graph) = {key} differ from the staged eager trainer's"
        assert torch.equal(words(got_params), words(want_params)), f"parameters of (knob, graph) = {key} differ"
