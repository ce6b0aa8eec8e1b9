"""The frame loop with tracking / densification at resolutions of their own, measured: the synthetic 1200 x 680 sequence of
``bench.py``'s ``slam_loop`` (13 frames, two runs, the second reported) through ``rgbd_slam(engine="fused")`` under

  full        ``replica_config()``: every step at full resolution
  splatam_s   ``splatam_s_config()``: 10 tracking / 15 mapping iterations, densification at 600 x 340
  phone       phone-like: ``replica_config()`` with tracking at 600 x 340 and densification at 300 x 170, full-size mapping

One JSON line per configuration: frames/s (the first frame excluded, as ``slam_loop`` does), rows at the end, ``phase_ms`` per phase
and frame (``prepare_frames`` among them), tracking ATE RMSE against the synthetic trajectory.  The reduced frames are derived from
the full frames by the frame-preparation kernel (``config['data']`` carries the sizes).

    python scripts/multires_run.py [--configs full,splatam_s,phone] [--frames 13] [--runs 2] [--out profiles/multires.md]
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python scripts/multires_run.py --configs phone --runs 1
    python scripts/multires_run.py --kernel-stats DIR/.../trace_kernel_stats.csv          (prints the frame-preparation kernel's row)
"""
import argparse
import csv
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, FX, FY, CX, CY = 1200, 680, 300_000, 600.0, 600.0, 599.5, 339.5          # bench.py WORKLOADS["B"]


def configs():
    from splatam_amd import pipeline
    phone = pipeline.replica_config()
    phone['data'] = dict(desired_image_height=H, desired_image_width=W, tracking_image_height=H // 2, tracking_image_width=W // 2,
                         densification_image_height=H // 4, densification_image_width=W // 4)
    return {"full": pipeline.replica_config(), "splatam_s": pipeline.splatam_s_config(W, H), "phone": phone}


def run_config(name, cfg, ds, runs):
    import numpy as np
    import torch
    from splatam_amd import evaluation, pipeline
    dev = torch.device("cuda")
    frames = len(ds)
    for _ in range(runs):
        torch.manual_seed(0)
        np.random.seed(0)
        torch.cuda.synchronize(dev)
        params, _, st = pipeline.rgbd_slam(ds, cfg, engine="fused")
        torch.cuda.synchronize(dev)
    counted = st['frame_s'][1:]
    phases = {}
    for fr in st['phase_ms'][1:]:
        for k, v in fr.items():
            phases[k] = phases.get(k, 0.0) + v
    n = max(len(counted), 1)
    poses = torch.stack([ds[t][3] for t in range(frames)])
    first_w2c = torch.linalg.inv(poses[0]).float().contiguous()
    data = cfg.get('data', {})
    return {"config": name, "frames": frames, "runs": runs,
            "tracking_size": [data.get('tracking_image_width', W), data.get('tracking_image_height', H)],
            "densification_size": [data.get('densification_image_width', W), data.get('densification_image_height', H)],
            "tracking_iters": cfg['tracking']['num_iters'], "mapping_iters": cfg['mapping']['num_iters'],
            "frames_per_s": round(n / max(sum(counted), 1e-9), 3), "ms_per_frame": round(1e3 * sum(counted) / n, 2),
            "rows_first_last": [st['num_gaussians'][0], st['num_gaussians'][-1]], "redone_iterations": st['redone_iterations'],
            "phase_ms_per_frame": {k: round(v / n, 3) for k, v in sorted(phases.items())},
            "ate_rmse_m": round(float(evaluation.trajectory_error(params, first_w2c, poses, frames)), 6)}


def kernel_row(path):
    """The frame-preparation kernel's row of a rocprofv3 ``*_kernel_stats.csv``."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "frame_prepare" in r.get("Name", "")]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="full,splatam_s,phone")
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the lines to this markdown file (box and commit first)")
    ap.add_argument("--kernel-stats", default=None, help="print the frame-preparation kernel's rows of a rocprofv3 kernel stats CSV and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        for r in kernel_row(args.kernel_stats):
            print(json.dumps(r))
        return
    import torch
    from splatam_amd import pipeline
    ds = pipeline.SyntheticRGBDSequence(N, W, H, FX, FY, CX, CY, num_frames=args.frames, seed=3, device=torch.device("cuda")).preload()
    all_cfg = configs()
    lines = [json.dumps(run_config(name, all_cfg[name], ds, args.runs)) for name in args.configs.split(",")]
    for line in lines:
        print(line, flush=True)
    if args.out:
        try:
            head = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            head = "unknown"
        with open(args.out, "a") as f:
            f.write(f"\n`scripts/multires_run.py --frames {args.frames} --runs {args.runs}` on {socket.gethostname()} "
                    f"({torch.cuda.get_device_name(0)}), commit {head} + working tree:\n\n```\n" + "\n".join(lines) + "\n```\n")


if __name__ == "__main__":
    main()
