"""bench.py's command line: a plain run times the headline only, `--full` keeps every secondary leg, and
`--dump-outputs DIR` writes what the timed path left after its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_secondary_legs(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (20, 3, False, None)
    assert a.no_cpu_baseline and a.no_accuracy and a.no_secondary and a.no_cold
    assert a.config4_steps == 0 and a.stream_frames == 0


def test_full_run_keeps_every_leg(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    assert not (a.no_cpu_baseline or a.no_accuracy or a.no_secondary or a.no_cold)
    assert a.config4_steps == 3 and a.stream_frames == 300
    # the thinning options still hold under --full
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--stream-frames", "0")
    assert a.no_cpu_baseline and a.stream_frames == 0 and not a.no_accuracy


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gpu_available, tmp_path):
    """A plain run on config 2 (50 keyframes): --steps sets the timed iterations exactly, the line carries the headline
    fields and none of the --full ones, and the dumped state is the problem's (pose 0 is held fixed by the solver, so it
    is the seed-0 input bit for bit)."""
    import synthetic
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--config", "config2", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["unit"] == "BA it/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 7 and d["config"]["iterations_timed"] == 7
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert d["full"] is False
    for k in ("roofline", "kernel_ms", "accuracy", "fp64_linear", "dropin_call", "config4", "config5", "cpu_baseline"):
        assert k not in d, k
    p = synthetic.make_problem("config2", seed=0)
    ptz, rays, cost = (np.load(out / f"{n}.npy") for n in ("ptz", "rays", "cost"))
    assert ptz.dtype == rays.dtype == cost.dtype == np.float64
    assert ptz.shape == (p.n_pose, 3) and rays.shape == (p.n_landmark, 2) and cost.shape == (2,)
    assert np.isfinite(ptz).all() and np.isfinite(rays).all()
    np.testing.assert_array_equal(ptz[0], p.init_ptz[0])
    assert 0 < cost[0] < cost[1]  # the last solve lowered the cost it started from
    assert d["dumped_outputs"]["arrays"] == {"ptz": list(ptz.shape), "rays": list(rays.shape), "cost": [2]}
