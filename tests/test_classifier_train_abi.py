"""Host-side contract of the fused classifier training step (classifier_kernels.hip): every invalid call of
nnue_classifier_train_step, nnue_classifier_train_step_bucketed and nnue_classifier_train_rider returns its NNUE_E_* code
before anything is launched, so these run without a GPU.  The pointers are host memory that a rejected call never
dereferences; no call here is valid, except the rider's, which only fills a host struct."""
import ctypes

import pytest

from nnue_hip import lib

E_ARG, E_SHAPE, E_SCRATCH = -1, -2, -4

MFMA = dict(B=64, L1=128, L2=64, L3=16, C=10)  # every first-layer product on the MFMA
SIMPLE = dict(B=5, L1=24, L2=7, L3=5, C=3)  # every first-layer product on the plain kernels
GRAD_NAMES = ("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3")
IN_NAMES = ("x", "w1", "b1", "w2", "b2", "w3", "b3", "labels", "h1", "h2", "logits", "sample_loss", "loss", "scratch")


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_uint8 * (1 << 16))()
    p = (ctypes.addressof(buf) + 15) & ~15
    yield buf, p


def _last_error():
    return lib.load().nnue_hip_last_error()


def _buckets(B, K, tiles=None, p=0, null=None):
    ptrs = {n: p for n in ("bucket", "rows", "tile_bucket", "seg")}
    if null:
        ptrs[null] = None
    t = lib.load().nnue_bucket_tile_count(B, K) if tiles is None else tiles
    return lib.NnueBuckets(K, ptrs["bucket"], ptrs["rows"], ptrs["tile_bucket"], ptrs["seg"], t)


def _caller(p):
    L = lib.load()

    def call(shape=MFMA, pairwise=1, phases=3, scratch_bytes=None, K=1, buckets=None, **ptrs):
        s = dict(shape)
        a = {n: p for n in IN_NAMES + GRAD_NAMES + ("d_x",)}
        a.update(ptrs)
        if scratch_bytes is None:
            scratch_bytes = max(L.nnue_classifier_train_scratch_bucketed(s["B"], s["L1"], s["L2"], s["L3"], s["C"], K), 1 << 30)
        args = (a["x"], pairwise, a["w1"], a["b1"], a["w2"], a["b2"], a["w3"], a["b3"], 0.0, a["labels"], 1.0,
                s["B"], s["L1"], s["L2"], s["L3"], s["C"], a["h1"], a["h2"], a["logits"], a["sample_loss"], a["loss"], a["d_x"],
                *[a[n] for n in GRAD_NAMES], a["scratch"], scratch_bytes, phases)
        if buckets is None:
            return L.nnue_classifier_train_step(*args, None)
        return L.nnue_classifier_train_step_bucketed(*args, ctypes.byref(buckets), None)

    return call


@pytest.mark.parametrize("phases", (0, 4, 8, 16, 20, 23, 28, 32, 33, 35, 49, 64, 65, -1))
def test_train_step_rejects_bad_phases(host, phases):
    """No activation or gradient bit, 4 with 16, 32 without 1 | 2 | 16, values beyond 63."""
    call = _caller(host[1])
    assert call(phases=phases) == E_ARG
    assert b"phases" in _last_error()


def test_train_step_rejects_bad_phase_combinations_for_the_shape(host):
    _, p = host
    call = _caller(p)
    B = MFMA["B"]
    # bit 8 (layer-1 slabs handed in): one layer stack, the pairwise block, L1 % 64 == 0
    assert call(phases=11, K=4, buckets=_buckets(B, 4, p=p)) == E_ARG
    assert b"one layer stack" in _last_error()
    assert call(phases=11, pairwise=0) == E_SHAPE
    assert call(phases=11, shape=dict(MFMA, L1=96)) == E_SHAPE
    assert b"L1 % 64" in _last_error()
    # bit 16 with K > 1 (grouped mode): the pairwise block and L1 % 4 == 0
    assert call(phases=17, pairwise=0, K=4, buckets=_buckets(B, 4, p=p)) == E_SHAPE
    assert call(phases=17, shape=dict(MFMA, L1=66), K=4, buckets=_buckets(B, 4, p=p)) == E_SHAPE
    assert b"L1 % 4" in _last_error()
    # bit 32 needs the MFMA d_x launch the small gradients ride in
    assert call(phases=51, shape=SIMPLE) == E_SHAPE
    assert b"bit 32" in _last_error()
    assert call(phases=51, d_x=None) == E_SHAPE


def test_train_step_rejects_bad_sizes_and_pointers(host):
    _, p = host
    call = _caller(p)
    for name in IN_NAMES:
        assert call(**{name: None}) == E_ARG, name
        assert b"null pointer" in _last_error()
    for name in GRAD_NAMES:
        assert call(**{name: None}) == E_ARG, name
        assert b"null gradient pointer" in _last_error()
    for dim in ("B", "L1", "L2", "L3", "C"):
        for v in (0, -3):
            assert call(shape=dict(MFMA, **{dim: v}), scratch_bytes=1 << 30) == E_ARG, (dim, v)
            assert b"must be positive" in _last_error()
    assert call(shape=dict(SIMPLE, L1=25)) == E_SHAPE  # pairwise needs an even L1
    assert b"even L1" in _last_error()
    # the per-sample tail keeps L2 + 2 L3 + C + 8 floats in LDS: at most 16384 of them
    base = dict(B=4, L1=64, L2=64, L3=16)
    fits = dict(base, C=16384 - (64 + 2 * 16 + 8))
    assert call(shape=dict(fits, C=fits["C"] + 1)) == E_SHAPE
    assert b"LDS" in _last_error()
    L = lib.load()
    for shape in (MFMA, SIMPLE, fits):
        need = L.nnue_classifier_train_scratch(*(shape[k] for k in ("B", "L1", "L2", "L3", "C")))
        assert need > 0 and need % 16 == 0
        assert call(shape=shape, scratch_bytes=need - 1) == E_SCRATCH, shape
        assert b"scratch" in _last_error()
    # 16-byte alignment of x, w1, scratch, d_w1, h1 and h2 (float4 loads and stores)
    for name in ("x", "w1", "scratch", "d_w1", "h1", "h2"):
        for off in (4, 8):
            assert call(**{name: p + off}) == E_ARG, (name, off)
            assert b"16-byte aligned" in _last_error()


def test_train_step_bucketed_rejects_bad_groupings(host):
    _, p = host
    call = _caller(p)
    B = MFMA["B"]
    assert call(K=65, buckets=_buckets(B, 65, tiles=(B + 15) // 16 + 65, p=p)) == E_SHAPE
    assert b"at most 64" in _last_error()
    for null in ("bucket", "rows", "tile_bucket", "seg"):
        assert call(K=4, buckets=_buckets(B, 4, p=p, null=null)) == E_ARG, null
        assert b"null bucket pointer" in _last_error()
    # a grouping made for another batch size
    assert call(K=4, buckets=_buckets(B + 16, 4, p=p)) == E_SHAPE
    assert b"another batch" in _last_error()
    # the stacked step's own scratch is larger than one stack's
    L = lib.load()
    one = L.nnue_classifier_train_scratch(*(MFMA[k] for k in ("B", "L1", "L2", "L3", "C")))
    four = L.nnue_classifier_train_scratch_bucketed(*(MFMA[k] for k in ("B", "L1", "L2", "L3", "C")), 4)
    assert four > one
    assert call(K=4, buckets=_buckets(B, 4, p=p), scratch_bytes=four - 1) == E_SCRATCH
    # the checks of the plain form hold for the stacked form as well
    assert call(K=4, buckets=_buckets(B, 4, p=p), phases=4) == E_ARG
    assert call(K=4, buckets=_buckets(B, 4, p=p), x=None) == E_ARG
    assert call(K=4, buckets=_buckets(B, 4, p=p), x=p + 4) == E_ARG


def test_train_rider_checks_its_arguments(host):
    _, p = host
    L = lib.load()
    s = MFMA
    need = L.nnue_classifier_train_scratch(s["B"], s["L1"], s["L2"], s["L3"], s["C"])
    names = ("h1", "h2", "sample_loss", "loss", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3", "scratch")

    def call(shape=s, scratch_bytes=need, buckets=None, out=True, **ptrs):
        a = {n: p for n in names}
        a.update(ptrs)
        rider = lib.NnueClsRider()
        rc = L.nnue_classifier_train_rider(1, shape["B"], shape["L1"], shape["L2"], shape["L3"], shape["C"],
                                           *[a[n] for n in names], scratch_bytes,
                                           ctypes.byref(buckets) if buckets is not None else None,
                                           ctypes.byref(rider) if out else None)
        return rc

    assert call() == 0  # host only: fills the struct, launches nothing
    for name in names:
        assert call(**{name: None}) == E_ARG, name
        assert b"null pointer" in _last_error()
    assert call(out=False) == E_ARG
    for dim in ("B", "L1", "L2", "L3", "C"):
        assert call(shape=dict(s, **{dim: 0})) == E_ARG, dim
        assert b"positive" in _last_error()
    assert call(scratch_bytes=need - 1) == E_SCRATCH
    B = s["B"]
    assert call(buckets=_buckets(B, 65, tiles=(B + 15) // 16 + 65, p=p)) == E_SHAPE
    assert call(buckets=_buckets(B, 4, p=p, null="seg")) == E_ARG
    assert call(buckets=_buckets(B - 16, 4, p=p)) == E_SHAPE
    four = L.nnue_classifier_train_scratch_bucketed(s["B"], s["L1"], s["L2"], s["L3"], s["C"], 4)
    assert call(buckets=_buckets(B, 4, p=p), scratch_bytes=four - 1) == E_SCRATCH
    assert call(buckets=_buckets(B, 4, p=p), scratch_bytes=four) == 0


def test_train_offsets_refuse_bad_sizes():
    L = lib.load()
    s = (MFMA["B"], MFMA["L1"], MFMA["L2"], MFMA["L3"], MFMA["C"])
    assert L.nnue_classifier_train_dz1_offset(*s, 1) >= 0
    for i in range(5):
        bad = list(s)
        bad[i] = 0
        assert L.nnue_classifier_train_dz1_offset(*bad, 1) == -1
        assert L.nnue_classifier_train_dz1_grouped_offset(*bad, 4) == -1
        assert L.nnue_classifier_train_x_grouped_offset(*bad, 4) == -1
    for k in (1, 65):  # grouped rows exist for 2..64 layer stacks only
        assert L.nnue_classifier_train_dz1_grouped_offset(*s, k) == -1
        assert L.nnue_classifier_train_x_grouped_offset(*s, k) == -1
    need = L.nnue_classifier_train_scratch_bucketed(*s, 4)
    dz, xg = L.nnue_classifier_train_dz1_grouped_offset(*s, 4), L.nnue_classifier_train_x_grouped_offset(*s, 4)
    rows = L.nnue_bucket_tile_count(MFMA["B"], 4) * 16
    assert dz % 16 == 0 and xg % 16 == 0
    assert dz + rows * MFMA["L2"] * 4 <= xg and xg + rows * MFMA["L1"] * 4 <= need
