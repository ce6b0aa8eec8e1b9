"""`python bench.py --gpus 2` started from a bare shell on a ONE-GPU box: bench.py launches its two ranks itself (torch.distributed.run,
127.0.0.1), the ranks share the GPU over gloo, rank 0 prints the JSON line with the N > 1 fields (sharded tracking, the exchanged mapping
step, both small-message forms).  The launch path the driver's scaling run takes; not a scaling figure."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_2_from_a_bare_shell():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SPLAT_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "5", "--workload", "A",
                        "--full", "--no-roofline", "--sustain-s", "0.2"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "weak"
    for k in ("allreduce_ms", "allreduce_small_ms", "allreduce_small_folded_ms", "tracking_replicated_iters_per_s",
              "mapping_with_exchange_iters_per_s"):
        assert d[k] is not None and d[k] > 0, k
    assert "gloo" in d["collectives"]


def _plain_run(out, steps):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5", "--workload",
                        "A", "--dump-outputs", str(out)], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run measures the headline only (no --full figures in its line) and --dump-outputs writes the timed path's last step: the
    map and the poses (float32, the workload's shapes) and a finite loss.  A second run with the same arguments writes the same outputs
    to rounding (the last timed step starts from the seeded scene; the composites' float atomics sum in a run-dependent order)."""
    import numpy as np
    out = tmp_path / "outputs"
    r = _plain_run(out, 30)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 30 and d["warmup"] == 5 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "iters/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"]
    for k in ("sustained", "tracking_iters_per_s", "dropin_iters_per_s", "roofline", "b_loop", "slam_loop", "cpu_baseline"):
        assert k not in d, k
    n = d["config"]["gaussians"]
    shapes = {"means3D": (n, 3), "rgb_colors": (n, 3), "unnorm_rotations": (n, 4), "logit_opacities": (n, 1), "log_scales": (n, 1),
              "loss": (1,)}
    for name, shape in shapes.items():
        a = np.load(out / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), (name, a.dtype, a.shape)
    assert np.load(out / "cam_trans.npy").shape[:2] == (1, 3) and np.load(out / "cam_unnorm_rots.npy").shape[:2] == (1, 4)
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
    again = tmp_path / "again"
    _plain_run(again, 30)
    for f in out.iterdir():
        a, b = np.load(f), np.load(again / f.name)
        assert a.shape == b.shape and float(np.abs(a.astype(np.float64) - b).max()) <= 1e-5 * max(1.0, float(np.abs(a).max())), f.name
