"""bench.py --dump-outputs on the GPU: two runs with the same arguments write the same outputs (up to the rounding of the
kernels' fp32 atomics), so that two builds of the project can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "16", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env={k: v for k, v in os.environ.items() if k != "VSX_BENCH_FULL"})
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["whole_path"]["loss_finite"] and line["full"] is False
    assert line["dumped_outputs"] == {"loss": [1], "params": [4194304], "grads": [4194304]}
    out = {n: np.load(os.path.join(out_dir, f"{n}.npy")) for n in ("loss", "params", "grads")}
    # the dump is the last timed step: its loss is the one the result line reports
    assert round(float(out["loss"][0]), 5) == line["whole_path"]["final_loss"]
    return out


@pytest.mark.gpu
def test_bench_dump_outputs_are_reproducible(tmp_path):
    a, b = _bench_dump(tmp_path / "a"), _bench_dump(tmp_path / "b")
    assert all(v.dtype == np.float32 for v in list(a.values()) + list(b.values()))
    # the parameters after the last step: the seeded ones in both runs, bit for bit (the steps do not drift apart)
    assert np.array_equal(a["params"], b["params"])
    # loss and gradients of the last step: equal up to the order in which fp32 atomics accumulated (measured: 3e-6 relative
    # on the loss, 3.5e-4 relative L2 on the gradients at this batch; a learning rate > 0 made the runs differ by percents)
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= 1e-4 * abs(float(a["loss"][0]))
    ga, gb = a["grads"].astype(np.float64), b["grads"].astype(np.float64)
    assert np.linalg.norm(ga - gb) <= 1e-2 * np.linalg.norm(ga)
    assert np.abs(ga - gb).max() <= 1e-2 * np.abs(ga).max()
