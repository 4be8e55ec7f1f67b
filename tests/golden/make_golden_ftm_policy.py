"""Generates tests/golden/ftm_policy.npz: what every launch-free shape query of csrc/ftm_kernels.hip answers over a grid of
shapes and per-call knob settings, recorded from the library as built at the commit BEFORE the policy was moved into one
resolver.  tests/test_ftm_policy_golden.py asks the current library the same questions and wants the same answers.

Run it only to record a deliberate policy change (it needs nothing but the built library, no GPU):
    python tests/golden/make_golden_ftm_policy.py
The fixture holds data only: `rows` int32 [2028, 7] (B, F, P, L1, H, W, stride; H = W = stride = 0 where the row has no
image), `knobs` the JSON list of the environment of each setting, and per query q an array `q` [len(KNOBS), 2028] (int64;
`uses_bf16` is [len(KNOBS), 2028, 6], one column per `which`).
"""
import json
import os
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent
PATH = GOLDEN / "ftm_policy.npz"

BATCHES = (1, 32, 37, 64, 128, 130, 193, 200, 256, 257, 512, 1024, 2048)
SHAPES = (  # F, P, H, W, stride
    (800, 968, 32, 32, 3),
    (968, 968, 31, 31, 3),
    (864, 864, 17, 23, 2),
    (2000, 4048, 0, 0, 0),
    (5000, 4048, 0, 0, 0),
    (1501, 4048, 0, 0, 0),
    (2000, 3240, 0, 0, 0),
    (300, 1152, 34, 34, 3),
    (65536, 65536, 224, 224, 7),
    (1, 968, 32, 32, 3),
    (800, 968, 32, 32, 2),
    (801, 970, 0, 0, 0),
)
WIDTHS = (64, 104, 136, 184, 200, 256, 312, 316, 440, 444, 512, 1020, 1024)
L2 = 72
KNOBS = (  # all read per call
    {},
    {"NNUE_FTM_BF_WM": "32"},
    {"NNUE_FTM_BF16": "0"},
    {"NNUE_FTM_VAL_PLANES": "0"},
    {"NNUE_FTM_VAL_PLANES_MIN_TILES": "1", "NNUE_FTM_FWD_PLANES_MIN_WG": "1"},
    {"NNUE_FTM_BF_BM": "32"},
)
PER_CALL = ("NNUE_FTM_BF16", "NNUE_FTM_BF_BM", "NNUE_FTM_BF_WM", "NNUE_FTM_VAL_PLANES", "NNUE_FTM_VAL_PLANES_MIN_TILES",
            "NNUE_FTM_FWD_PLANES_MIN_WG")
QUERIES = ("supported", "scratch", "forward_l1_supported", "forward_l1_planes_supported", "backward_cw_supported", "backward_sq_count",
           "backward_ste_chunks", "value_planes_supported", "update_forward_supported", "gram_scratch", "uses_bf16")


def rows():
    return np.array([(b, f, p, l1, h, w, s) for b in BATCHES for (f, p, h, w, s) in SHAPES for l1 in WIDTHS], dtype=np.int32)


def ask(L, row):
    b, f, p, l1, h, w, s = (int(v) for v in row)
    return {
        "supported": L.nnue_ftm_supported(f, p, l1),
        "scratch": L.nnue_ftm_scratch(b, f, p, l1),
        "forward_l1_supported": L.nnue_ftm_forward_l1_supported(b, f, p, l1, L2),
        "forward_l1_planes_supported": L.nnue_ftm_forward_l1_planes_supported(b, f, p, l1, L2),
        "backward_cw_supported": L.nnue_ftm_backward_cw_supported(b, f, p, l1, L2),
        "backward_sq_count": L.nnue_ftm_backward_sq_count(b, f, p, l1),
        "backward_ste_chunks": L.nnue_ftm_backward_ste_chunks(b, f, p, l1, h, w, s),
        "value_planes_supported": L.nnue_ftm_value_planes_supported(b, f, p, l1, h, w, s),
        "update_forward_supported": L.nnue_ftm_update_forward_supported(b, min(b, 128), f, p, l1),
        "gram_scratch": L.nnue_ftm_gram_scratch(b, f, p),
        "uses_bf16": [L.nnue_ftm_uses_bf16(which, b, f, p, l1) for which in range(6)],
    }


def record(L):
    """{query: int64 array [len(KNOBS), rows(, 6)]} from the loaded library `L`; the environment is left as it was found."""
    grid = rows()
    saved = {k: os.environ.pop(k, None) for k in PER_CALL}
    try:
        out = {q: [] for q in QUERIES}
        for env in KNOBS:
            os.environ.update(env)
            answers = [ask(L, row) for row in grid]
            for q in QUERIES:
                out[q].append([a[q] for a in answers])
            for k in env:
                del os.environ[k]
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return {q: np.asarray(v, dtype=np.int64) for q, v in out.items()}


def branch_counts(table):
    """Rows of the default knob setting that take each branch of the policy."""
    d = {q: table[q][0] for q in QUERIES}
    return {
        "ste_ride": int((d["backward_ste_chunks"] > 0).sum()),
        "value_planes": int((d["value_planes_supported"] != 0).sum()),
        "rider": int((d["backward_cw_supported"] != 0).sum()),
        "update_forward": int((d["update_forward_supported"] != 0).sum()),
        "six_plane_values": int((d["uses_bf16"][:, 5] != 0).sum()),
        "planes_forward": int((d["forward_l1_planes_supported"] != 0).sum()),
        "split_k_forward": int((d["scratch"] > 0).sum()),
    }


def main():
    sys.path.insert(0, str(GOLDEN.parent.parent / "nnue-vision_amd"))
    from nnue_hip import lib
    table = record(lib.load())
    counts = branch_counts(table)
    assert all(counts.values()), counts
    for k in range(1, len(KNOBS)):
        changed = np.zeros(len(rows()), dtype=bool)
        for q in QUERIES:
            diff = table[q][k] != table[q][0]
            changed |= diff.reshape(len(changed), -1).any(axis=1)
        print(KNOBS[k], "changes", int(changed.sum()), "rows")
        assert changed.any(), KNOBS[k]
    np.savez_compressed(PATH, rows=rows(), knobs=np.array(json.dumps(KNOBS)), **table)
    print(counts)
    print("wrote", PATH, PATH.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
