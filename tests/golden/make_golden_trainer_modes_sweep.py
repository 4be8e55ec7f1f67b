"""Generates tests/golden/trainer_modes_sweep.json: the mode tests/trainer_modes.py::resolve gives every row's configuration (and
three big tables) under no knob at all and under the row's own environment, and under each of the two with every single knob of
the step-mode policy set to each of its non-default values on top -- recorded at the commit BEFORE the policy moved out of
NnueTrainer.__init__ into nnue_hip/step_mode.py, when ``resolve`` was a hand-written restatement of it.
tests/test_step_mode_golden.py asks the resolver the trainer now uses the same questions and wants the same answers: the table's
rows name 44 points, the sweep holds the policy still at the points between them.

Run it only to record a deliberate policy change (it needs nothing but the built library, no GPU):
    python tests/golden/make_golden_trainer_modes_sweep.py
The fixture holds data only: `keys` (the mode's keys, the order of every record's values), `configs` (one per row, then BIG_TABLES)
and `records` [config index, environment, values].
"""
import json
import os
import sys
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent
PATH = GOLDEN / "trainer_modes_sweep.json"

# knob -> its non-default values.  First the knobs the Python policy reads itself (lib.ft_path's NNUE_FT_PATH among them), then
# the per-call knobs the library reads behind the launch-free queries.  NNUE_FTM_SPLIT_BACKWARD is read by the policy per call
# and by the library once per process; with it set every answer of the library that depends on it is masked by the policy's own
# reading, so its entries do not depend on what the process started with.  NNUE_FTM_RIDE_STE_V64 is the library's alone and
# once per process: not swept.
SWEEP = (
    ("NNUE_FT_PATH", ("bits", "list")),  # ("mfma" is what the default takes wherever the shape allows it)
    ("NNUE_CONV_PATCHES", ("0", "1")),
    ("NNUE_DEFER_STE", ("0",)),
    ("NNUE_FUSE_L1", ("0",)),
    ("NNUE_FTM_FWD_PLANES", ("0",)),
    ("NNUE_FTM_SPLIT_BACKWARD", ("1",)),
    ("NNUE_FTM_RIDE_DW1", ("0",)),
    ("NNUE_FUSE_TABLE_UPDATE", ("0", "1")),
    ("NNUE_NORM_PARTIALS", ("0",)),
    ("NNUE_FTM_RIDE_STE", ("0",)),
    ("NNUE_FUSE_NEXT_FORWARD", ("0",)),
    ("NNUE_CLS_RIDE_SMALL", ("0",)),
    ("NNUE_CLS_FUSE_TAIL_DX", ("0",)),
    ("NNUE_FTM_VAL_PLANES", ("0",)),
    ("NNUE_FTM_VAL_PLANES_MIN_TILES", ("1",)),
    ("NNUE_FTM_FWD_PLANES_MIN_WG", ("1",)),
    ("NNUE_FTM_BF16", ("0",)),
)


# beside the rows: a 32768 x 256 table (32 MB, where NNUE_FUSE_TABLE_UPDATE=auto turns the fused table update on; no row's
# table is that big, the resolution launches nothing), over base A
BIG_TABLES = (dict(grid=32, fps=32, image=96, batch=64), dict(grid=32, fps=32, image=96, batch=64, optimizer="adam"),
              dict(grid=32, fps=32, image=96, batch=200, K=4))


def environments(own):
    """The environments a configuration is resolved under: none and its row's own, and each of the two with every single knob
    setting on top (a knob such as NNUE_FTM_FWD_PLANES only acts at these shapes beside the row's NNUE_FTM_FWD_PLANES_MIN_WG)."""
    envs = []
    for base in ({}, dict(own)):
        for env in [base] + [{**base, k: v} for k, values in SWEEP for v in values]:
            if env not in envs:
                envs.append(env)
    return envs


def resolve_under(tm, cfg, env):
    """tm.resolve(cfg) with exactly `env` of tm.KNOBS set; the environment is left as it was found."""
    saved = {k: os.environ.pop(k, None) for k in tm.KNOBS}
    try:
        os.environ.update(env)
        return tm.resolve(cfg)
    finally:
        for k in tm.KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def record(tm):
    keys = sorted(tm.A_MODES)
    points = [(row.config, row.env) for row in tm.ROWS] + [({**tm.A, **cfg}, {}) for cfg in BIG_TABLES]
    records = []
    for i, (cfg, own) in enumerate(points):
        for env in environments(own):
            mode = resolve_under(tm, cfg, env)
            assert sorted(mode) == keys
            records.append([i, env, [mode[k] for k in keys]])
    return dict(keys=keys, configs=[cfg for cfg, _ in points], records=records)


def main():
    sys.path[:0] = [str(GOLDEN.parent), str(GOLDEN.parent.parent / "nnue-vision_amd")]
    import trainer_modes as tm
    assert all(k in tm.KNOBS for k, _ in SWEEP)
    table = record(tm)
    at = {(i, json.dumps(env, sort_keys=True)): v for i, env, v in table["records"]}
    for knob, values in SWEEP:
        for value in values:
            under = [(i, env, v) for i, env, v in table["records"] if env.get(knob) == value]
            moved = sum(v != at.get((i, json.dumps({k: x for k, x in env.items() if k != knob}, sort_keys=True)), v) for i, env, v in under)
            print(f"{knob}={value} moves {moved} of {len(under)} records")
            assert moved, (knob, value)
    PATH.write_text(json.dumps(table, separators=(",", ":")) + "\n")
    print("wrote", PATH, len(table["records"]), "records,", PATH.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
