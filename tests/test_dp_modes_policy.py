"""The data-parallel table of tests/dp_modes.py, settled without a GPU: every row resolves to the mode it states through the
trainer's own launch-free resolver, the rank slices of its three steps are what the table says (which ranks come up short or
empty), the oracle's per-rank pieces add up to the global step the ranks are held to, and the bars the driver applies pass a
float32 rounding of the oracle but see one sample lost from the rank-summed small gradients.  tests/test_gpu_dp_modes.py then
runs every row on every rank."""
import pytest
import torch

import nnue_oracle as orc
from dp_modes import BY_NAME, GROUPS, ROW_NAMES, ROWS, oracle_of, rows_of
from trainer_modes import KNOBS, SHORT, build_model, compare_held, differences, geometry, hyper, set_knobs, step_mode_of


@pytest.mark.parametrize("name", ROW_NAMES)
def test_the_queries_resolve_the_row_as_the_table_says(name, monkeypatch):
    row = BY_NAME[name]
    set_knobs(monkeypatch, row)
    sm = step_mode_of(row.config, dp=row.facts())
    wrong = differences({k: getattr(sm, k) for k in row.expect}, row.expect)
    assert not wrong, f"{name}: " + "; ".join(wrong) + f" ({sm.describe()})"
    # without graphs the same mode but for the capture
    eager = step_mode_of(row.config, dp=row.facts(), use_graph=False)
    assert not eager.capture_collectives
    assert differences({k: getattr(eager, k) for k in row.expect}, dict(row.expect, capture_collectives=False)) == []
    if sm.factor_exchange:  # the norm's Gram product contracts the GLOBAL batch
        from nnue_hip import lib
        g = geometry(row.config)
        assert sm.sq_range == (g["tbl_lo"], g["tbl_hi"])
        assert sm.sq_count == int(lib.load().nnue_ftm_gram_sq_count(row.config["batch"] * row.world, row.config["l1"]))


def test_rows_are_unique_and_their_knobs_are_the_data_parallel_ones():
    assert len(set(ROW_NAMES)) == len(ROWS)
    seen = {}
    for row in ROWS:
        assert all(k in KNOBS and k.startswith("NNUE_DP_") for k in row.env), row.name
        assert (row.backend, row.env.get("NNUE_DP_FORCE_COLLECTIVES")) in (("gloo", None), ("nccl", "1")), row.name
        key = (tuple(sorted(row.config.items(), key=str)), tuple(sorted(row.env.items())), row.group)
        assert key not in seen, f"{row.name} repeats {seen.get(key)}"
        seen[key] = row.name
    assert GROUPS == [(1, "nccl"), (2, "gloo"), (4, "gloo")]  # three spawns, at most 1 + 4 processes on the GPU


def test_census_what_no_process_group_ran_before_occurs():
    def some(holds):
        return any(holds(r, r.config, r.expect) for r in ROWS)
    multi = lambda r: r.world > 1  # noqa: E731
    assert some(lambda r, c, m: multi(r) and c["optimizer"] == "adam" and c["K"] == 1)
    assert some(lambda r, c, m: multi(r) and c["optimizer"] == "adam" and c["K"] > 1)
    assert some(lambda r, c, m: multi(r) and c["optimizer"] == "adam" and r.env.get("NNUE_DP_FACTOR_EXCHANGE") == "1"
                and r.env.get("NNUE_DP_SHARDED_UPDATE") == "1" and not m["factor_exchange"] and not m["sharded_update"])
    assert some(lambda r, c, m: r.world == 4 and m["sharded_update"] and c["momentum"] == 0.0)
    for how in ("factor_exchange", "sharded_update"):
        assert some(lambda r, c, m: multi(r) and m[how] and c["K"] > 1), how
    for path in ("bits", "list"):
        assert some(lambda r, c, m: multi(r) and m["ft_path"] == path), path
    assert some(lambda r, c, m: multi(r) and m["sharded_update"] and m["ft_path"] == "bits")
    assert some(lambda r, c, m: multi(r) and m["factor_exchange"] and geometry(c)["P"] == geometry(c)["F"] == 256)
    assert some(lambda r, c, m: multi(r) and m["factor_exchange"] and geometry(c)["P"] > geometry(c)["F"])
    assert some(lambda r, c, m: multi(r) and m["factor_exchange"] and c["l1"] == 72)
    assert some(lambda r, c, m: r.world == 4 and m["factor_exchange"])
    assert some(lambda r, c, m: multi(r) and m["factor_exchange"] and m["fuse_next_forward"])
    assert some(lambda r, c, m: multi(r) and r.buckets == 2)
    for how in ("factor_exchange", "sharded_update", "fuse_next_forward"):
        assert some(lambda r, c, m: r.backend == "nccl" and m["capture_collectives"] and m[how]), how
    assert some(lambda r, c, m: r.backend == "nccl" and m["capture_collectives"] and c["optimizer"] == "adam")


# real samples per rank of the short third step, by (rows per rank, world)
SHORT_STEP = {(12, 2): [11, 0], (11, 2): [9, 0], (16, 2): [16, 3], (8, 4): [8, 8, 3, 0], (24, 1): [11], (32, 1): [19]}


def test_the_rank_slices_are_what_the_table_says():
    assert {(r.config["batch"], r.world) for r in ROWS} == set(SHORT_STEP)
    assert {r.config["batch"] * r.world for r in ROWS} == {22, 24, 32}  # ragged against the 16- and 32-row tiles or one short of them
    for row in ROWS:
        b, w = row.config["batch"], row.world
        assert row.counts(0) == row.counts(1) == [b] * w, row.name
        assert row.counts(2) == SHORT_STEP[(b, w)] and sum(row.counts(2)) == b * w - SHORT, row.name
        if w > 1:  # the last rank is short or empty, and it is not the only rank with rows
            assert row.counts(2)[-1] < b and row.counts(2)[0] > 0, row.name
    assert any(r.counts(2)[-1] == 0 for r in ROWS) and any(0 < r.counts(2)[-1] < r.config["batch"] for r in ROWS if r.world > 1)
    # 4-byte and 16-byte unpack of the bit map: P = 968 is no multiple of 16, P = 256 and 8192 are
    fx = [geometry(r.config)["P"] for r in ROWS if r.expect["factor_exchange"]]
    assert {p % 16 == 0 for p in fx} == {False, True} and {968, 256, 8192} <= set(fx)


def cheapest(group):
    """The group's row with the smallest table and batch."""
    return min(rows_of(group), key=lambda r: (geometry(r.config)["F"] * r.config["l1"], r.config["batch"], r.config["K"]))


@pytest.fixture(scope="module")
def oracles():
    return {}


@pytest.mark.parametrize("group", GROUPS, ids=[f"{b}{w}" for w, b in GROUPS])
def test_the_oracles_rank_slices_add_up(group, oracles):
    """What the driver holds each rank to is one global oracle step cut by rows: the ranks' own steps on their slices, taken in
    float64 from the same parameters, give back its logits, its loss as the mean of the rank-local losses the trainer returns
    (sum over the rank's rows / B, times B * world / n), and its gradients as the sum the collective forms; the flat layout's
    shards restore the packed gradients."""
    from nnue_hip.trainer import FlatLayout
    row = cheapest(group)
    cfg, world, b = row.global_config, row.world, row.config["batch"]
    stride = geometry(cfg)["stride"]
    refs = oracles.setdefault(row.name, oracle_of(row))
    layout = FlatLayout.of(build_model(cfg), pad_to=4 * world)
    assert layout.count % (4 * world) == 0
    for ref in refs:
        n = ref["images"].shape[0]
        assert [min((r + 1) * b, n) - min(r * b, n) for r in range(world)] == row.counts(ref["step"])
        logits, losses, total = [], [], {k: torch.zeros_like(v) for k, v in ref["grads"].items()}
        for r in range(world):
            rows = slice(min(r * b, n), min((r + 1) * b, n))
            n_r = rows.stop - rows.start
            if n_r == 0:
                losses.append(0.0)
                continue
            images, labels = ref["images"][rows].double(), ref["labels"][rows]
            lg, loss, grads, _ = orc.loss_and_grads_explicit(ref["before"], images, labels, stride, cfg["clip"])
            logits.append(lg)
            losses.append(float(loss) * n_r / b * (b * world / n))
            for k in total:
                total[k] += grads[k] * n_r / n
        assert float((torch.cat(logits) - ref["logits"]).abs().max()) <= 1e-12 * max(1.0, float(ref["logits"].abs().max()))
        assert abs(sum(losses) / world - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
        for k, g in ref["grads"].items():
            assert float((total[k] - g).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1e-300), k
        flat = layout.pack({k: v.float() for k, v in ref["grads"].items()})
        per = layout.count // world
        shards = [flat[r * per:(r + 1) * per].clone() for r in range(world)]
        for k, v in layout.views(torch.cat(shards)).items():
            assert torch.equal(v, ref["grads"][k].float()), k


def _held(ref, grads, after, state, cfg):
    f32 = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    g = geometry(cfg)
    held = dict(optimizer="sgd", sink=g["F"] - 1 if g["P"] > g["F"] else None, logits=ref["logits"].float(),
                loss=torch.tensor(ref["loss"]).float(), norm=torch.tensor(ref["norm"]).float(), grads=f32(grads),
                params=f32(after), was=f32(ref["before"]), momentum=f32(state))
    return held


def test_the_bars_see_a_sample_lost_from_the_summed_small_gradients(oracles):
    """compare_held on the first oracle step of the two-rank base row: the oracle rounded to float32 is inside every bar;
    the same step with the last sample's term missing from the summed visual_threshold and conv.weight gradients -- what a
    dropped row of one rank's chunk would give -- is outside the gradient and the update bars."""
    row = BY_NAME["ar"]
    cfg = row.global_config
    ref = oracles.setdefault(row.name, oracle_of(row))[0]
    n, hp = ref["images"].shape[0], hyper(cfg)
    clean = {}
    assert compare_held(_held(ref, ref["grads"], ref["after"], ref["state"], cfg), ref, n, n, None, "rounded", clean) == []
    print("rounded to float32:", {k: round(v, 4) for k, v in clean.items()})
    assert clean and all(v <= 1.0 for v in clean.values())
    assert {"logits", "loss", "norm", "grad", "parameters", "update", "momentum"} <= set(clean)

    _, _, last, _ = orc.loss_and_grads_explicit(ref["before"], ref["images"][n - 1:].double(), ref["labels"][n - 1:],
                                                geometry(cfg)["stride"], cfg["clip"])
    grads = {k: v.clone() for k, v in ref["grads"].items()}
    for k in ("visual_threshold", "conv.weight"):
        grads[k] -= last[k] / n
    after, state = {k: v.clone() for k, v in ref["before"].items()}, {}
    orc.sgd_step(after, grads, state, hp["lr"], hp["momentum"], hp["weight_decay"], ref["max_grad_norm"])
    lost = {}
    fails = compare_held(_held(ref, grads, after, state, cfg), ref, n, n, None, "one sample lost", lost)
    print("one sample lost:", {k: round(v, 4) for k, v in lost.items()})
    assert lost["grad"] > 1.0 and lost["update"] > 1.0
    assert any("visual_threshold" in f for f in fails) and any("conv.weight" in f for f in fails)
