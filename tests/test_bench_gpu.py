"""-m gpu: the plain bench command (`bench.py --gpus 1 --steps K --warmup W`) prints the headline line alone -- what moved behind
`--full` is absent -- and `--dump-outputs DIR` writes the last timed step's loss, flat parameters and flat gradients as float32 .npy"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_hbm", "sustained", "comm", "configs", "reference_loop", "cpu_baseline", "rel_l2_vs_oracle",
             "torch_gpu_baseline", "variants")


def test_plain_bench_line_and_output_dump(tmp_path):
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["dtype"] == "f32"
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - 8 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(out)) == ["grads.npy", "loss.npy", "params.npy"]
    arrays = {k: np.load(os.path.join(out, k + ".npy")) for k in ("loss", "params", "grads")}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["loss"].shape == (1,) and float(arrays["loss"][0]) == line["config"]["final_loss"]
    assert arrays["params"].shape == arrays["grads"].shape and arrays["params"].size >= line["config"]["params"]
    assert float(np.abs(arrays["grads"]).max()) > 0
