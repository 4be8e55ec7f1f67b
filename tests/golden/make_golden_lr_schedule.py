"""Generates tests/golden/lr_schedule_cases.json from the REAL reference: the float64 values of its ``get_lr``
(training_utils.py:283-336) at chosen iterations of six configurations.  tests/test_lr_schedule.py wants
``nnue_hip.lr_schedule.LrSchedule.lr`` to return the same doubles with ``==``.

Run it where the reference tree is (it is never read by a test); its ``training_utils.py`` needs only the standard library
and torch:
    python tests/golden/make_golden_lr_schedule.py <path to the reference tree>
The fixture holds data only: per case the configuration's fields, the iterations and the values as ``float.hex`` strings
(exact) beside their decimal repr (readable).
"""
import json
import sys
from pathlib import Path
from types import SimpleNamespace

PATH = Path(__file__).resolve().parent / "lr_schedule_cases.json"

BASE = dict(learning_rate=0.01, min_lr=0.0, warmup_iters=0, lr_decay_iters=100, decay_lr=True, use_cyclical_lr=False,
            cyclical_lr_period=1000, cyclical_lr_amplitude=0.1)
ITS = list(range(8)) + [50, 99, 100, 101]
CASES = {
    "plain_cosine_100": (dict(BASE), ITS),
    "warmup_5": (dict(BASE, warmup_iters=5), ITS),
    "no_decay": (dict(BASE, decay_lr=False), ITS),
    "cyclical_period_8_clamped": (dict(BASE, min_lr=1e-4, use_cyclical_lr=True, cyclical_lr_period=8, cyclical_lr_amplitude=0.5), ITS),
    "warmup_0_min_lr": (dict(BASE, min_lr=1e-3, learning_rate=0.05), ITS),
    "long_29400": (dict(BASE, lr_decay_iters=29400, warmup_iters=100), ITS + [14700, 29398, 29399, 29400]),
}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from training_utils import get_lr
    out = {}
    for name, (fields, its) in CASES.items():
        cfg = SimpleNamespace(**fields)
        values = [get_lr(it, cfg=cfg) for it in its]
        out[name] = {"config": fields, "iterations": its, "hex": [float(v).hex() for v in values], "repr": [repr(float(v)) for v in values]}
    # the reference's own failure, recorded as a fact: a division by zero at it == warmup_iters == lr_decay_iters
    try:
        get_lr(5, cfg=SimpleNamespace(**dict(BASE, warmup_iters=5, lr_decay_iters=5)))
        raised = None
    except ZeroDivisionError:
        raised = "ZeroDivisionError"
    out["_reference_at_warmup_eq_decay_iters"] = raised
    PATH.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", PATH, PATH.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
