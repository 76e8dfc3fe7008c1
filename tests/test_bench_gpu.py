"""bench.py on the device: a plain line times exactly --steps steps and carries the headline only; --dump-outputs holds what the last
timed step returned."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_line_and_dumped_outputs(tmp_path):
    """the same model, driven as bench.py drives it (one evaluation that sets the device up, W warm-up and K timed training steps), ends on
    the loss and gradients that the plain run wrote"""
    steps, warmup, n = 3, 2, 1024
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--n", str(n), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["steps"] == steps and r["warmup"] == warmup and r["ms_per_step"] > 0 and r["unit"] == "evals/s" and r["dtype"] == "f64"
    assert not {"configs", "cpu_baseline", "sustained", "stages_ms_per_eval", "gram_hbm"} & set(r), sorted(r)

    sys.path.insert(0, ROOT)
    import bench
    m, run_step, _ = bench.build_model("cfg2", 0, n)
    losses = []
    step = bench.training_step(m, lambda: losses.append(float(m.loss())), "exact")
    run_step()
    for _ in range(warmup + steps):
        step()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    files = sorted(glob.glob(str(tmp_path / "grad_*.npy")))
    assert len(files) == len(grads) and len(grads) > 0, files
    loss = np.load(str(tmp_path / "loss.npy"))
    assert loss.dtype == np.float64 and abs(float(loss) - losses[-1]) <= 1e-11 * abs(losses[-1]), (float(loss), losses[-1])
    for f, g in zip(files, grads):
        d = np.load(f)
        assert d.dtype == np.float64 and d.shape == g.shape, f
        assert np.max(np.abs(d - g)) <= 1e-9 * max(1e-300, np.max(np.abs(g))), f
