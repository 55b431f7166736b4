"""-m gpu: bench.py's plain run (set-up, warm-up, timed steps, the JSON line; the diagnostic legs only with --full) and
--dump-outputs, at a small size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    out = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--arch", "resnet50", "--crop", "193", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads(r.stdout.splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "images/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 4 / (d["ms_per_step"] / 1e3)) <= 1e-3 * d["value"]
    for k in ("roofline", "phase_ms", "ms_step_lr0.01", "ms_per_step_direct", "cpu_baseline", "config5"):
        assert k not in d, k                      # --full only
    files = sorted(os.listdir(out))
    assert files == ["losses.npy", "student_momentum.npy", "student_weights.npy", "teacher_weights.npy"], files
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 << 20
    arr = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arr.values())
    # the dumped meters are the ones the last timed step returned (the line rounds them to 5 digits)
    assert np.allclose(arr["losses"], d["losses_last_step"], rtol=0, atol=1e-5)
    assert arr["student_weights"].shape == arr["teacher_weights"].shape == arr["student_momentum"].shape
    assert np.abs(arr["student_momentum"]).max() > 0
