"""bench.py end to end at a small size (a child process: the bench owns its process): a plain
run prints its line without the --full extras and --dump-outputs writes the last timed step's
loss, carried state and updated parameters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "2", "--seq", "300", "--segments", "2", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "bf16"
    assert line["unit"] == "audio-frames/s" and line["higher_is_better"] is True
    # value and ms_per_step describe the same timed steps: frames per step / ms_per_step
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * 300 / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert line["cpu_baseline"] is None   # the CPU baselines are --full's
    files = sorted(os.listdir(out))
    arrays = {f: np.load(out / f) for f in files}
    assert arrays["loss.npy"].dtype == np.float64
    assert float(arrays["loss.npy"][0]) == pytest.approx(line["loss_last"], abs=1e-4)
    params = [f for f in files if f.startswith("param.")]
    state = [f for f in files if f.startswith("state.")]
    assert "param.encoder.output_proj.weight.npy" in params and state
    assert all(arrays[f].dtype == np.float32 and np.isfinite(arrays[f]).all() for f in params + state)
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
