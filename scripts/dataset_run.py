"""The frame loop fed from disk against the same loop fed from memory, measured: the synthetic 1200 x 680 sequence of ``bench.py``'s
``slam_loop`` is written to a temporary directory in Replica layout (``results/frame*.jpg`` as JPEG, ``results/depth*.png`` =
round(z * 6553.5) as 16-bit PNG, ``traj.txt``), read back through ``datasets.get_dataset`` and run through
``rgbd_slam(engine="fused")`` at

  splatam     ``replica_config()``: 40 tracking / 60 mapping iterations at full resolution
  splatam_s   ``splatam_s_config()``: 10 / 15 iterations, densification at 600 x 340 (from disk: ``dataset.at_size(340, 600)``)

and, for comparison, from an in-memory sequence that holds the very frames the loader hands over (the decoded JPEG bytes as float32,
float32(float64(raw) / 6553.5) depth), where the loop derives the reduced frames itself.  One JSON line per run: frames/s (the first
frame excluded, as ``slam_loop`` does), the ``prepare_frames`` phase per frame, host time inside ``dataset[i]`` per call and per frame (of
which: waiting for the decoded frame, the upload calls) and the share of frames the read-ahead had already begun, all over the counted
frames; then one line per setting with the disk / memory ratio of every run pair.

    python scripts/dataset_run.py [--settings splatam,splatam_s] [--frames 13] [--runs 2] [--prefetch 4] [--out profiles/datasets.md]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, FX, FY, CX, CY, SCALE = 1200, 680, 300_000, 600.0, 600.0, 599.5, 339.5, 6553.5          # bench.py WORKLOADS["B"]


def write_sequence(root, frames):
    """The synthetic sequence in Replica layout under ``root``/room0; returns the data config dict."""
    import numpy as np
    import torch
    from PIL import Image
    from splatam_amd import pipeline
    ds = pipeline.SyntheticRGBDSequence(N, W, H, FX, FY, CX, CY, num_frames=frames, seed=3, device=torch.device("cuda"))
    base = os.path.join(root, "room0", "results")
    os.makedirs(base)
    with open(os.path.join(root, "room0", "traj.txt"), "w") as traj:
        for t in range(frames):
            color, depth, _, pose = ds[t]
            rgb = np.rint(color.cpu().numpy()).clip(0, 255).astype(np.uint8)
            raw = np.rint(depth.cpu().numpy()[..., 0].astype(np.float64) * SCALE).clip(0, 65535).astype(np.uint16)
            Image.fromarray(rgb).save(os.path.join(base, f"frame{t:06d}.jpg"), quality=95)
            Image.fromarray(raw).save(os.path.join(base, f"depth{t:06d}.png"))
            traj.write(" ".join(repr(float(x)) for x in pose.cpu().numpy().reshape(-1)) + "\n")
    return dict(dataset_name="replica", camera_params=dict(image_height=H, image_width=W, fx=FX, fy=FY, cx=CX, cy=CY, png_depth_scale=SCALE))


class MemorySequence:
    """The items of a dataset, read once and kept on the device."""

    def __init__(self, dataset):
        self.items = [dataset[t] for t in range(len(dataset))]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, t):
        return self.items[t]


class Metered:
    """A dataset whose every ``[t]`` notes what it added to the loader's counters, so that frame 0 (decoded on the spot, and excluded
    from frames/s) can be left out of the per-frame figures."""

    def __init__(self, dataset, calls):
        self.dataset, self.calls = dataset, calls

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, t):
        before = dict(self.dataset.stats)
        item = self.dataset[t]
        self.calls.append((t, {k: v - before[k] for k, v in self.dataset.stats.items()}))
        return item


def settings():
    from splatam_amd import pipeline
    return {"splatam": pipeline.replica_config(), "splatam_s": pipeline.splatam_s_config(W, H)}


def one_run(name, cfg, source, root, data_cfg, memory, prefetch):
    import numpy as np
    import torch
    from splatam_amd import datasets, evaluation, pipeline
    torch.manual_seed(0)
    np.random.seed(0)
    extra, ds = {}, memory
    if source == "disk":
        loader = datasets.get_dataset(data_cfg, root, "room0", desired_height=H, desired_width=W, device="cuda", prefetch=prefetch)
        calls = []
        ds = Metered(loader, calls)
        data = cfg.get('data', {})
        size = (data.get('densification_image_height', H), data.get('densification_image_width', W))
        if size != (H, W):
            extra['densify_dataset'] = Metered(loader.at_size(*size), calls)
    torch.cuda.synchronize()
    try:
        params, _, st = pipeline.rgbd_slam(ds, cfg, engine="fused", **extra)
        torch.cuda.synchronize()
        stats = None
        if source == "disk":
            later = [d for t, d in calls if t > 0]
            stats = {k: sum(d[k] for d in later) for k in loader.stats}
            poses = loader.transformed_poses
        else:
            poses = torch.stack([ds[t][3] for t in range(len(ds))])
    finally:
        if source == "disk":
            loader.close()
    counted = st['frame_s'][1:]
    n = max(len(counted), 1)
    prepare = sum(fr.get('prepare_frames', 0.0) for fr in st['phase_ms'][1:]) / n
    out = {"setting": name, "source": source, "frames": len(ds), "frames_per_s": round(n / max(sum(counted), 1e-9), 3),
           "ms_per_frame": round(1e3 * sum(counted) / n, 3), "prepare_frames_ms_per_frame": round(prepare, 3),
           "rows_last": st['num_gaussians'][-1],
           "ate_rmse_m": round(float(evaluation.trajectory_error(params, torch.linalg.inv(poses[0]).float().contiguous(), poses, len(ds))), 6)}
    if stats is not None:
        out.update(dataset_item_ms_per_call=round(1e3 * stats['item_s'] / max(stats['items'], 1), 3),
                   dataset_ms_per_frame=round(1e3 * stats['item_s'] / n, 3),
                   dataset_fetch_ms_per_frame=round(1e3 * stats['fetch_s'] / max(stats['fetches'], 1), 3),
                   decode_wait_ms_per_frame=round(1e3 * stats['wait_s'] / max(stats['fetches'], 1), 3),
                   upload_calls_ms_per_frame=round(1e3 * stats['upload_s'] / max(stats['fetches'], 1), 3),
                   prefetch=prefetch, prefetch_hit_rate=round(stats['prefetch_hits'] / max(stats['fetches'], 1), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="splatam,splatam_s")
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--prefetch", type=int, default=4)
    ap.add_argument("--out", default=None, help="append the lines to this markdown file")
    args = ap.parse_args()
    import torch
    from splatam_amd import datasets
    root = tempfile.mkdtemp(prefix="dataset_run_")
    lines = []
    try:
        data_cfg = write_sequence(root, args.frames)
        loader = datasets.get_dataset(data_cfg, root, "room0", desired_height=H, desired_width=W, device="cuda", prefetch=0)
        memory = MemorySequence(loader)
        all_cfg = settings()
        for name in args.settings.split(","):
            rates = {"disk": [], "memory": []}
            # one run of each source first (lists sized, allocator warm, files in the page cache), then the measured pairs, interleaved
            for source in ("memory", "disk"):
                one_run(name, all_cfg[name], source, root, data_cfg, memory, args.prefetch)
            for r in range(args.runs):
                for source in ("memory", "disk"):
                    res = dict(one_run(name, all_cfg[name], source, root, data_cfg, memory, args.prefetch), run=r)
                    rates[source].append(res["frames_per_s"])
                    lines.append(json.dumps(res))
                    print(lines[-1], flush=True)
            lines.append(json.dumps({"setting": name, "disk_over_memory": [round(d / m, 4) for d, m in zip(rates["disk"], rates["memory"])],
                                     "disk_frames_per_s": rates["disk"], "memory_frames_per_s": rates["memory"]}))
            print(lines[-1], flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if args.out:
        try:
            head = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            head = "unknown"
        with open(args.out, "a") as f:
            f.write(f"\n`scripts/dataset_run.py --frames {args.frames} --runs {args.runs} --prefetch {args.prefetch}` on "
                    f"{torch.cuda.get_device_name(0)}, commit {head} + working tree:\n\n```\n" + "\n".join(lines) + "\n```\n")


if __name__ == "__main__":
    main()
