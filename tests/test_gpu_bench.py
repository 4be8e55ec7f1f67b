"""bench.py as the comparisons call it: a plain run reports the timed steps only and, with --dump-outputs, writes what the
last timed step computed; --full adds the per-kernel pass and the roofline.  Tiny workload (c1).  ``-m gpu``."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def run_bench(*flags):
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--workload", "c1", *flags],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    rec = run_bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(32 * 7 / rec["timed_s"], rel=1e-2)  # batch 32 per step (timed_s is rounded to 1 us)
    assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    for key in ("roofline", "kernels", "gather_path", "cpu_baseline"):
        assert key not in rec, key
    files = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    for name in ("loss", "logits", "visual_threshold", "conv.weight", "input.weight", "input.bias"):
        assert name in files, sorted(files)
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    for name, a in files.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert files["logits"].shape == (32, 10)
    assert float(files["loss"][0]) == pytest.approx(rec["config"]["loss_after"], abs=1e-4)


def test_full_run_adds_the_instrumented_pass():
    rec = run_bench("--steps", "5", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-gather-compare")
    assert rec["steps"] == 5 and rec["roofline"]["kernel"] in rec["kernels"]
    assert rec["config"]["eager_ms_per_step_instrumented"] > 0
