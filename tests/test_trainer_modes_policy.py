"""The mode table of tests/trainer_modes.py, settled without a GPU: the library's launch-free queries (lib.ft_path,
nnue_ftm_forward_l1_supported, ..._l1_planes_supported, ..._backward_cw_supported, ..._backward_ste_chunks,
..._value_planes_supported, ..._update_forward_supported, nnue_classifier_train_fused_tail_supported,
nnue_ftm_backward_sq_count) answer for every row as the table says, and the table as a whole covers every flag in both
values, every phase mask and every combination it was written for.  tests/test_gpu_trainer_modes.py then holds the live
trainer to the same table and each row's step to the oracle."""
import pytest

from trainer_modes import A_MODES, FLAGS, PHASES, ROWS, ROW_NAMES, BY_NAME, differences, geometry, launches_of, resolve, set_knobs


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
    from nnue_hip import lib
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
