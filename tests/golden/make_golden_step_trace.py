"""Generates tests/golden/step_trace.json: the run form of every scripted call of tests/step_trace.py (entry points, graph
replays, collectives, the graph cache and the counters after each call), recorded on one MI355X at the commit BEFORE
``NnueTrainer.step`` and ``step_many`` got one driver.  tests/test_gpu_step_trace.py runs the same script on the current trainer
and wants the same trace.

Run it only to record a deliberate change of a run form (it needs the built library and a GPU; default knobs):
    python tests/golden/make_golden_step_trace.py [OUTPUT]
The fixture holds data only: per scenario the list of records ``{trainer, call, events, state}``.
"""
import json
import sys
import tempfile
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent
ROOT = GOLDEN.parent.parent
for p in (str(ROOT / "nnue-vision_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> None:
    import step_trace
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN / "step_trace.json"
    out = {}
    for name in step_trace.SCENARIOS:
        why = step_trace.off_form(name)
        if why:
            raise SystemExit(f"{name}: {why}; record with default knobs")
        with tempfile.TemporaryDirectory() as tmp:
            out[name] = step_trace.run_scenario(name, tmp)
        print(f"{name}: {len(out[name])} calls", flush=True)
    lines = [f"{json.dumps(name)}: [\n" + ",\n".join("  " + json.dumps(r) for r in recs) + "\n]" for name, recs in out.items()]
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
