"""The mode table of tests/trainer_modes.py, settled without a GPU: the trainer's own resolver (nnue_hip.step_mode.resolve,
over the library's launch-free queries) answers for every row as the table says, and the table as a whole covers every flag in
both values, every phase mask and every combination it was written for.  The data-parallel decisions, which the table's
single-rank rows do not reach, have their own table here.  tests/test_gpu_trainer_modes.py then holds the live trainer to the
same table and each row's step to the oracle."""
import os

import pytest

from nnue_hip import lib
from nnue_hip.step_mode import DpFacts
from trainer_modes import A, A_MODES, FLAGS, PHASES, ROWS, ROW_NAMES, BY_NAME, Row, build_model, differences, geometry, launches_of, \
    resolve, set_knobs, step_mode_of, LEAD


@pytest.mark.parametrize("name", ROW_NAMES)
def test_the_queries_resolve_the_row_as_the_table_says(name, monkeypatch):
    row = BY_NAME[name]
    set_knobs(monkeypatch, row)
    got = resolve(row.config)
    assert set(got) == set(A_MODES) == set(row.modes)
    wrong = differences(got, row.modes)
    assert not wrong, f"{name}: " + "; ".join(wrong)


def test_the_bf16_products_are_on_by_default(monkeypatch):
    """What the big-table rows were chosen for rests on the bf16-split tiles (nnue_ftm_uses_bf16; NNUE_FTM_BF16 is read per
    call): the split-K forward and the update in the weight gradient's epilogue at the 8192-row table, the six-plane
    stand-alone value gradient at the 16384-row one."""
    uses = lib.load().nnue_ftm_uses_bf16
    set_knobs(monkeypatch, BY_NAME["t8192_ftu"])
    small, big = BY_NAME["t8192_ftu"].config, BY_NAME["t16384_b160"].config
    s, b = geometry(small), geometry(big)
    assert (s["F"], s["P"], b["F"], b["P"]) == (8192, 8192, 16384, 16384)
    assert uses(0, small["batch"], s["F"], s["P"], small["l1"]) == 1 and uses(3, small["batch"], s["F"], s["P"], small["l1"]) == 1
    assert uses(4, big["batch"], b["F"], b["P"], big["l1"]) == 1
    monkeypatch.setenv("NNUE_FTM_BF16", "0")
    assert uses(0, small["batch"], s["F"], s["P"], small["l1"]) == 0 and uses(4, big["batch"], b["F"], b["P"], big["l1"]) == 0
    assert not resolve(small)["fuse_next_forward"]


def test_row_names_and_tuples_are_unique():
    assert len(set(ROW_NAMES)) == len(ROWS)
    seen = {}
    for row in ROWS:  # a row may share its mode with another only where shape, optimizer or knobs reach it another way
        key = (tuple(sorted(row.config.items(), key=str)), tuple(sorted(row.env.items())))
        assert key not in seen, f"{row.name} repeats {seen.get(key)}"
        seen[key] = row.name


def test_census_every_flag_takes_both_values_and_every_phase_mask_occurs():
    modes = [row.modes for row in ROWS]
    for flag in FLAGS:
        assert {m[flag] for m in modes} == {False, True}, flag
    assert {m["phases"] for m in modes} == set(PHASES)
    assert {m["ft_path"] for m in modes} == {"mfma", "bits", "list"}
    assert {m["sq"] for m in modes} == {"tiles", "gram", "none"}
    assert {m["optimizer"] for m in modes} == {"sgd", "adam"}
    assert {m["ste_launch"] for m in modes} == {None, 1, 3}
    assert any(row.config["momentum"] == 0.0 for row in ROWS) and any(row.config["clip"] for row in ROWS)


# the combinations no whole-step oracle test ran before this table: (what, predicate on (configuration, mode))
COMBINATIONS = (
    ("Adam with the layer-1 fusion and the d_w1 rider: STE launch with stages=3, no norm partials",
     lambda c, m: m["optimizer"] == "adam" and m["fuse_l1"] and m["ride_dw1"] and not m["defer_ste"] and m["ste_launch"] == 3
     and m["sq"] == "none"),
    ("phases 13 with the layer-1 fusion but no rider at L1 % 128 != 0",
     lambda c, m: m["phases"] == 13 and m["fuse_l1"] and not m["ride_dw1"] and c["l1"] % 128 != 0),
    ("phases 13 with the layer-1 fusion but no rider at L2 % 4 != 0",
     lambda c, m: m["phases"] == 13 and m["fuse_l1"] and not m["ride_dw1"] and c["l2"] % 4 != 0),
    ("phases 5 on the product path at L1 % 64 != 0", lambda c, m: m["phases"] == 5 and m["ft_path"] == "mfma" and c["l1"] % 64 != 0),
    ("fps < 8: merged backward without the STE ride, STE launch with stages=1",
     lambda c, m: c["fps"] < 8 and m["ft_path"] == "mfma" and not m["ride_ste"] and m["defer_ste"] and m["ste_launch"] == 1),
    ("fps > 8: merged backward without the STE ride, STE launch with stages=1",
     lambda c, m: c["fps"] > 8 and m["ft_path"] == "mfma" and not m["ride_ste"] and m["defer_ste"] and m["ste_launch"] == 1),
    ("fps * 28 > 4096: the second STE stage cannot ride in the norm launch",
     lambda c, m: c["fps"] * 28 > 4096 and c["optimizer"] == "sgd" and not m["defer_ste"] and m["ste_launch"] == 3),
    ("patches together with the STE ride", lambda c, m: m["use_patches"] and m["ride_ste"]),
    ("several stacks with patches", lambda c, m: m["grouped"] and m["use_patches"]),
    ("several stacks with Adam", lambda c, m: m["grouped"] and m["optimizer"] == "adam"),
    ("several stacks on the bits family (grouping from the counts)", lambda c, m: m["grouped"] and m["ft_path"] == "bits"),
    ("several stacks on the list family (grouping from the counts)", lambda c, m: m["grouped"] and m["ft_path"] == "list"),
    ("a table whose merged launch is not taken: stand-alone products, tile norm partials, no rider",
     lambda c, m: m["ft_path"] == "mfma" and not m["fuse_table_update"] and not m["ride_dw1"] and not m["ride_ste"]
     and m["sq"] == "tiles" and m["phases"] == 5 and c["l1"] % 64 == 0),
    ("the fused table update with the layer-1 fusion", lambda c, m: m["fuse_table_update"] and m["fuse_l1"]),
    ("the fused table update with the layer-1 fusion at a clamp-sink map",
     lambda c, m: m["fuse_table_update"] and m["fuse_l1"] and geometry(c)["P"] > geometry(c)["F"]),
    ("the fused table update with several stacks", lambda c, m: m["fuse_table_update"] and m["grouped"]),
    ("the fused table update with plain SGD", lambda c, m: m["fuse_table_update"] and c["optimizer"] == "sgd" and c["momentum"] == 0.0),
    ("the fused table update + next forward with Adam", lambda c, m: m["fuse_next_forward"] and m["optimizer"] == "adam"),
    ("forward and value planes", lambda c, m: m["fwd_planes"] and m["val_planes"]),
    ("value planes alone", lambda c, m: m["val_planes"] and not m["fwd_planes"]),
    ("forward planes alone", lambda c, m: m["fwd_planes"] and not m["val_planes"]),
    ("phases 59 at the shape that can take the tail into the d_x launch", lambda c, m: m["phases"] == 59 and c["l2"] == 128),
    ("SGD on the product path with the optimizer reading the table's rows for the norm",
     lambda c, m: m["ft_path"] == "mfma" and m["optimizer"] == "sgd" and m["sq"] == "none" and m["ride_ste"]),
    ("patches at overlapping taps (stride 3)", lambda c, m: m["use_patches"] and geometry(c)["stride"] == 3),
    ("the fused table update at one stack without the next forward, no layer-1 fusion",
     lambda c, m: m["fuse_table_update"] and not m["fuse_next_forward"] and not m["fuse_l1"] and not m["grouped"]),
    ("the STE launch on patches, first stage only", lambda c, m: m["use_patches"] and m["ste_launch"] == 1),
    ("the STE launch on patches, both stages", lambda c, m: m["use_patches"] and m["ste_launch"] == 3),
)


@pytest.mark.parametrize("what,holds", COMBINATIONS, ids=[c[0] for c in COMBINATIONS])
def test_census_the_combination_occurs(what, holds):
    assert any(holds(row.config, row.modes) for row in ROWS), what


def test_every_row_has_a_short_batch_and_more_than_one_tile():
    from trainer_modes import SHORT
    for row in ROWS:
        assert row.config["batch"] - SHORT >= 8, row.name


def test_the_launch_list_follows_the_mode():
    """launches_of on the two ends of the table: every default fusion on, and the gather kernels."""
    assert launches_of(BY_NAME["A"].modes) == ["nnue_ftm_conv_binarize", "nnue_ftm_forward_l1", "nnue_classifier_train_step",
                                               "nnue_ftm_backward", "nnue_sgd_step"]
    assert launches_of(BY_NAME["g5_bits_k3"].modes) == [
        "nnue_conv3x3_forward", "nnue_binarize_bits", "nnue_binarize_bits", "nnue_bucket_group", "nnue_ftb_forward",
        "nnue_classifier_train_step_bucketed", "nnue_ftb_backward_weight", "nnue_classifier_train_step_bucketed",
        "nnue_ftb_backward_values", "nnue_ste_conv_backward", "nnue_sgd_step"]
    # the sequence tests/test_gpu_update_sequence.py logged at its shape (fused table update, Adam)
    assert launches_of(BY_NAME["t8192_ftu_adam"].modes) == [
        "nnue_ftm_conv_binarize", "nnue_ftm_forward", "nnue_classifier_train_step", "nnue_ftm_gram_sqnorm_tail",
        "nnue_classifier_train_step", "nnue_ftm_backward_values_ws", "nnue_ste_conv_backward", "nnue_adam_step_ext",
        "nnue_ftm_backward_weight_update_adam"]


def test_geometry_is_the_flat_layouts():
    """geometry's restatement of the table's range of the flat buffers against FlatLayout.of on each row's model (CPU)."""
    from nnue_hip.trainer import FlatLayout
    for cfg in {tuple(sorted((k, row.config[k]) for k in ("grid", "fps", "image", "l1", "l2", "l3", "classes", "K"))) for row in ROWS}:
        cfg = {**A, **dict(cfg)}
        g, layout = geometry(cfg), FlatLayout.of(build_model(cfg))
        assert layout.names[:3] == LEAD
        lo = layout.offsets[2]
        assert (g["tbl_lo"], g["tbl_hi"]) == (lo, lo + min(g["F"] - 1, g["P"]) * cfg["l1"]), cfg
        assert layout.shapes[2] == (g["F"], cfg["l1"]) and layout.count >= g["tbl_hi"]


def test_the_phase_bits_compose_the_masks_the_library_takes():
    dx, small, beside, slabs = lib.CLS_PHASE_DX, lib.CLS_PHASE_SMALL, lib.CLS_DW1_BESIDE_DX, lib.CLS_L1_SLABS_GIVEN
    rides, small_ride, tail = lib.CLS_DW1_RIDES, lib.CLS_SMALL_RIDE, lib.CLS_TAIL_IN_DX
    assert (dx, small, beside, slabs, rides, small_ride, tail) == (1, 2, 4, 8, 16, 32, 64)
    assert dx | beside == 5 and small | beside == 6 and dx | beside | slabs == 13
    assert dx | small | rides == 19 and dx | small | rides | slabs == 27
    assert dx | small | rides | small_ride == 51 and dx | small | rides | small_ride | slabs == 59
    assert dx | small | rides | small_ride | slabs | tail == 123


# ---- data parallel: what NnueTrainer decides from DataParallel's facts (collectives, world, buckets, backend), as rows of
# (name, configuration over A, knobs, arguments of step_mode_of, what the StepMode must say)
BIG = dict(grid=32, fps=32, image=96, batch=64)  # a 32768 x 256 table: 32 MB, where the factor exchange turns itself on
NO_FX = {"NNUE_DP_FACTOR_EXCHANGE": "0"}
ALL_REDUCE = dict(factor_exchange=False, sharded_update=False, grads_materialised=True, sq="none", sq_range=None, sq_count=0)


def ranks(world=2, buckets=1, backend="nccl"):
    return DpFacts(True, world, buckets, backend)


DP_ROWS = (
    ("A: one all-reduce, complete gradients before it", {}, {}, dict(dp=ranks()),
     dict(ALL_REDUCE, defer_ste=False, ride_ste=False, fuse_table_update=False, ste_stages=3, capture_collectives=True,
          ride_dw1=True, ride_small=True, fuse_l1=True, phases=59, merged_backward_launch=True)),
    ("A on one rank with the collectives forced", {}, {}, dict(dp=ranks(world=1)),
     dict(ALL_REDUCE, defer_ste=False, ride_ste=False, fuse_table_update=False, ste_stages=3, capture_collectives=True)),
    ("big table: the factor exchange", BIG, {}, dict(dp=ranks()),
     dict(factor_exchange=True, sharded_update=False, grads_materialised=False, sq="gram", ride_dw1=False, ride_small=False,
          fuse_table_update=False, merged_backward_launch=False, defer_ste=False, ride_ste=False, ste_stages=3,
          capture_collectives=True)),
    ("big table, the exchange forced at a small one", {}, {"NNUE_DP_FACTOR_EXCHANGE": "1"}, dict(dp=ranks()),
     dict(factor_exchange=True, grads_materialised=False, sq="gram", ride_dw1=False, phases=13)),
    ("big table without the exchange, flat buffers of 64 MB: the sharded update", BIG, NO_FX, dict(dp=ranks(), count=16 << 20),
     dict(ALL_REDUCE, sharded_update=True)),
    ("big table without the exchange, flat buffers below 64 MB", BIG, NO_FX, dict(dp=ranks(), count=(16 << 20) - 4), ALL_REDUCE),
    ("small buffers, the sharded update forced", {}, {"NNUE_DP_SHARDED_UPDATE": "1"}, dict(dp=ranks()), dict(ALL_REDUCE, sharded_update=True)),
    ("big table and buffers, the sharded update refused", BIG, {**NO_FX, "NNUE_DP_SHARDED_UPDATE": "0"}, dict(dp=ranks(), count=16 << 20),
     ALL_REDUCE),
    ("two buckets: neither exchange nor shards nor capture", BIG, {}, dict(dp=ranks(buckets=2), count=16 << 20),
     dict(ALL_REDUCE, capture_collectives=False)),
    ("gloo: the collective stays eager", {}, {}, dict(dp=ranks(backend="gloo")), dict(ALL_REDUCE, capture_collectives=False)),
    ("no graphs: the collective stays eager", {}, {}, dict(dp=ranks(), use_graph=False), dict(ALL_REDUCE, capture_collectives=False)),
    ("NNUE_DP_CAPTURE=0", {}, {"NNUE_DP_CAPTURE": "0"}, dict(dp=ranks()), dict(ALL_REDUCE, capture_collectives=False)),
    ("Adam at the big table: no exchange, no shards", dict(BIG, optimizer="adam"), {}, dict(dp=ranks(), count=16 << 20), ALL_REDUCE),
)


@pytest.mark.parametrize("what,cfg,env,args,expect", DP_ROWS, ids=[r[0] for r in DP_ROWS])
def test_the_data_parallel_decisions(what, cfg, env, args, expect, monkeypatch):
    cfg = {**A, **cfg}
    set_knobs(monkeypatch, Row(what, env=env))
    sm = step_mode_of(cfg, **args)
    assert sm.ft_path == "mfma"
    wrong = differences({k: getattr(sm, k) for k in expect}, expect)
    assert not wrong, f"{what}: " + "; ".join(wrong) + f" ({sm.describe()})"
    if sm.sq == "gram":  # the norm's Gram product contracts the GLOBAL batch
        g = geometry(cfg)
        assert sm.sq_range == (g["tbl_lo"], g["tbl_hi"])
        assert sm.sq_count == int(lib.load().nnue_ftm_gram_sq_count(cfg["batch"] * args["dp"].world, cfg["l1"]))
    assert sm.phases in PHASES


def test_describe_is_the_row_of_the_record(monkeypatch):
    set_knobs(monkeypatch, BY_NAME["A"])
    assert step_mode_of(BY_NAME["A"].config).describe() == \
        "mfma | defer_ste, fuse_l1, ride_dw1, ride_ste, ride_small | sq tiles | phases 59 | STE ride, 112 chunks"
    set_knobs(monkeypatch, BY_NAME["g5_bits"])
    assert step_mode_of(BY_NAME["g5_bits"].config).describe() == "bits | defer_ste | sq none | phases 5 | STE stages=1"


# ---- the kernel family as an argument (resolve(ft_path=...), what NnueTrainer(ft_path=...) and rebuilt() pass) against the same
# family forced through the process environment
@pytest.mark.parametrize("path", ("bits", "list", "mfma", "auto"))
@pytest.mark.parametrize("name", ("A", "A_k4_clip", "g5_bits"))
def test_the_family_as_an_argument_resolves_as_the_variable_does(name, path, monkeypatch):
    row = BY_NAME[name]
    set_knobs(monkeypatch, row)
    monkeypatch.setenv("NNUE_FT_PATH", path)
    by_variable = step_mode_of(row.config)
    monkeypatch.delenv("NNUE_FT_PATH")
    before = dict(os.environ)
    by_argument = step_mode_of(row.config, ft_path=path)
    assert dict(os.environ) == before
    assert by_argument == by_variable, f"{by_argument.describe()} != {by_variable.describe()}"


@pytest.mark.parametrize("name", ("A", "A_k4_clip", "g5_bits"))
def test_the_family_argument_wins_over_the_variable(name, monkeypatch):
    row = BY_NAME[name]
    set_knobs(monkeypatch, row)
    monkeypatch.setenv("NNUE_FT_PATH", "bits")
    want = step_mode_of(row.config)
    monkeypatch.setenv("NNUE_FT_PATH", "list")
    before = dict(os.environ)
    assert step_mode_of(row.config, ft_path="bits") == want
    assert dict(os.environ) == before
    assert step_mode_of(row.config).ft_path == "list"  # (and without the argument the variable still decides)
