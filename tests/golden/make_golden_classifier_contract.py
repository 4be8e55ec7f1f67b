"""Generates tests/golden/classifier_contract.npz: the host contract of the classifier block in csrc/classifier_kernels.hip,
recorded from the library as built at the commit BEFORE its dispatch was moved into one plan (train_step_plan) and one
launcher per product.  tests/test_classifier_contract_golden.py replays the same calls against the current library and wants the
same codes, the same full text of nnue_hip_last_error() and the same answers.

Run it only to record a deliberate change of the contract (it needs nothing but the built library, no GPU):
    python tests/golden/make_golden_classifier_contract.py

Every recorded nnue_classifier_train_step(_bucketed) call is one the library REFUSES (NNUE_E_ARG, NNUE_E_SHAPE or
NNUE_E_SCRATCH): an accepted call would launch, so record() stops at the first row with any other code and nothing is written.
The pointers are host memory that a refused call never dereferences.

The fixture holds data only:
  `messages`  the JSON list of the distinct error texts, each stored once
  `calls`     int32 [N, 11]: section (0 = early checks, scratch_bytes = 0; 1 = late checks, ample scratch), B, L1, L2, L3, C,
              pairwise, K, phases, d_x given, index into POINTERS of the pointer moved 4 bytes off alignment (-1: none)
  `code`      int8 [N], `message` int16 [N] (index into `messages`)
  `queries`   int32 [M, 6]: B, L1, L2, L3, C, K of the launch-free queries, and per query q an int64 array `q` [M] or [M, 2]
              (one column per `pairwise`); `rider` uint8 [M, 2, 256]: what nnue_classifier_train_rider writes into a zeroed
              nnue_cls_rider for the fixed fake pointers below.
"""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent
PATH = GOLDEN / "classifier_contract.npz"

REFUSALS = (-1, -2, -4)  # NNUE_E_ARG, NNUE_E_SHAPE, NNUE_E_SCRATCH
SHAPES = {  # B, L1, L2, L3, C: C1, C2, B37, cls257 and simple of tests/test_gpu_classifier_train.py and one MFMA shape off 128
    "C1": (32, 64, 32, 8, 10),
    "C2": (512, 1024, 128, 32, 10),
    "B37": (37, 256, 48, 16, 7),
    "cls257": (40, 320, 160, 40, 257),
    "simple": (33, 24, 7, 5, 3),
    "L1_96": (64, 96, 64, 16, 10),
}
STACKS = (1, 4)
POINTERS = ("x", "w1", "scratch", "d_w1", "h1", "h2", "w2", "w3")  # the ones an alignment check reads
QUERY_BATCHES = (1, 37, 512, 1024)
QUERY_STACKS = (1, 3, 8)
QUERIES = ("scratch", "train_scratch", "dz1_offset", "dz1_grouped_offset", "x_grouped_offset", "fused_tail_supported", "tile_count")
FUSED_STEP = 123
SMALL_RIDE = 32
AMPLE = 1 << 40  # bytes of scratch no shape here needs

IN_NAMES = ("x", "w1", "b1", "w2", "b2", "w3", "b3", "labels", "h1", "h2", "logits", "sample_loss", "loss", "scratch")
GRAD_NAMES = ("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3")
RIDER_NAMES = ("h1", "h2", "sample_loss", "loss", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3", "scratch")
FAKE = {n: 0x10000 * (i + 1) for i, n in enumerate(RIDER_NAMES + ("bucket", "rows", "tile_bucket", "seg"))}  # never dereferenced


def call_rows(L):
    """The refused calls: int32 [N, 11] (module docstring)."""
    rows = []
    for shape in SHAPES.values():  # (a) early checks: nothing later than the scratch check is reached
        for pairwise in (0, 1):
            for K in STACKS:
                for dx in (1, 0):
                    rows += [(0, *shape, pairwise, K, ph, dx, -1) for ph in range(128)]
    for shape in SHAPES.values():  # (b) late checks
        for pairwise in (0, 1):
            for K in STACKS:
                rows += [(1, *shape, pairwise, K, ph, 0, -1) for ph in range(128) if ph & SMALL_RIDE]
            if not L.nnue_classifier_train_fused_tail_supported(*shape, 1, pairwise):
                rows.append((1, *shape, pairwise, 1, FUSED_STEP, 1, -1))
    c2 = SHAPES["C2"]
    rows += [(1, *c2, 1, 1, FUSED_STEP, 1, POINTERS.index(n)) for n in ("w2", "w3")]
    rows += [(1, *c2, 1, 1, 3, 1, POINTERS.index(n)) for n in ("x", "w1", "scratch", "d_w1", "h1", "h2")]
    return np.array(rows, dtype=np.int32)


def query_rows():
    return np.array([(b, *s[1:], k) for b in QUERY_BATCHES for s in SHAPES.values() for k in QUERY_STACKS], dtype=np.int32)


def _buckets(lib, L, B, K, ptrs):
    return lib.NnueBuckets(K, ptrs["bucket"], ptrs["rows"], ptrs["tile_bucket"], ptrs["seg"], L.nnue_bucket_tile_count(B, K))


def record(lib):
    """(codes int8 [N], texts [N], {query: array}) from the loaded module `lib`.  Raises at the first train-step call that is
    not refused: that call has launched, and no later one is made."""
    L = lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    codes, texts = [], []
    for sec, B, L1, L2, L3, C, pairwise, K, phases, dx, mis in call_rows(L).tolist():
        a = {n: p for n in IN_NAMES + GRAD_NAMES}
        if mis >= 0:
            a[POINTERS[mis]] = p + 4
        args = (a["x"], pairwise, a["w1"], a["b1"], a["w2"], a["b2"], a["w3"], a["b3"], 0.0, a["labels"], 1.0, B, L1, L2, L3, C,
                a["h1"], a["h2"], a["logits"], a["sample_loss"], a["loss"], p if dx else None, *[a[n] for n in GRAD_NAMES],
                a["scratch"], AMPLE if sec else 0, phases)
        if K == 1:
            rc = L.nnue_classifier_train_step(*args, None)
        else:
            bk = _buckets(lib, L, B, K, {n: p for n in ("bucket", "rows", "tile_bucket", "seg")})
            rc = L.nnue_classifier_train_step_bucketed(*args, ctypes.byref(bk), None)
        if rc not in REFUSALS:
            raise AssertionError(f"nnue_classifier_train_step returned {rc} (not a refusal) for section {sec} B={B} L1={L1} L2={L2} "
                                 f"L3={L3} C={C} pairwise={pairwise} K={K} phases={phases} d_x={dx} misaligned={mis}")
        codes.append(rc)
        texts.append(L.nnue_hip_last_error().decode())
    q = {name: [] for name in QUERIES + ("rider",)}
    for B, L1, L2, L3, C, K in query_rows().tolist():
        q["scratch"].append(L.nnue_classifier_scratch_bucketed(B, L1, L2, L3, K))
        need = L.nnue_classifier_train_scratch_bucketed(B, L1, L2, L3, C, K)
        q["train_scratch"].append(need)
        q["dz1_offset"].append([L.nnue_classifier_train_dz1_offset(B, L1, L2, L3, C, pw) for pw in (0, 1)])
        q["dz1_grouped_offset"].append(L.nnue_classifier_train_dz1_grouped_offset(B, L1, L2, L3, C, K))
        q["x_grouped_offset"].append(L.nnue_classifier_train_x_grouped_offset(B, L1, L2, L3, C, K))
        q["fused_tail_supported"].append([L.nnue_classifier_train_fused_tail_supported(B, L1, L2, L3, C, K, pw) for pw in (0, 1)])
        q["tile_count"].append(L.nnue_bucket_tile_count(B, K))
        riders = []
        for pw in (0, 1):
            out = lib.NnueClsRider()
            bk = _buckets(lib, L, B, K, FAKE)
            rc = L.nnue_classifier_train_rider(pw, B, L1, L2, L3, C, *[FAKE[n] for n in RIDER_NAMES], need,
                                               ctypes.byref(bk) if K > 1 else None, ctypes.byref(out))
            assert rc == 0, (rc, L.nnue_hip_last_error())
            riders.append(bytes(out.opaque))
        q["rider"].append([np.frombuffer(r, dtype=np.uint8) for r in riders])
    table = {name: np.asarray(v, dtype=np.uint8 if name == "rider" else np.int64) for name, v in q.items()}
    return np.asarray(codes, dtype=np.int8), texts, table


def main():
    sys.path.insert(0, str(GOLDEN.parent.parent / "nnue-vision_amd"))
    from nnue_hip import lib
    codes, texts, table = record(lib)
    assert set(codes.tolist()) == set(REFUSALS), set(codes.tolist())
    messages = sorted(set(texts))
    index = {m: i for i, m in enumerate(messages)}
    np.savez_compressed(PATH, messages=np.array(json.dumps(messages)), calls=call_rows(lib.load()), code=codes,
                        message=np.array([index[t] for t in texts], dtype=np.int16), queries=query_rows(), **table)
    print(len(codes), "refused calls,", len(messages), "distinct messages,", len(query_rows()), "query rows")
    print("wrote", PATH, PATH.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
