"""Frames pushed one at a time through ``session.SlamSession.add_raw_frame``, as a sensor would deliver them: host arrays of RGB
bytes and raw depth, resized on the device to the loop's resolutions, tracked, mapped and made keyframes before the next is read.

The sequence is a NeRFCapture directory (``--capture DIR``: its PNGs decoded ahead of the clock, uint16 depth with 6553.5 units per
metre) or, by default, the synthetic sequence of ``bench.py``'s ``slam_loop`` turned into bytes and float32 depth:

  splatam_s     1200 x 680 bytes and depth, ``pipeline.splatam_s_config()`` (10 + 15 iterations, densification at 600 x 340)
  online_demo   the values of the reference's configs/iphone/online_demo.py: 1920 x 1440 bytes over a 256 x 192 float32 depth image, the
                loop at 960 x 720, densification at 480 x 360, 60 + 60 iterations, the depth-loss retry, a window of 32

Every setting is replayed twice: unpaced (frames/s; the latency of every frame from the call to its pose being complete on the
device: p50, p95, max) and paced at ``--rate`` Hz (frame t is due at t / rate: how many frames were due before their predecessor had
finished, and the latencies again).  The first frame (set-up, allocations) is excluded from every figure.  One JSON line per setting
and pacing.

    python scripts/live_run.py [--settings splatam_s,online_demo] [--frames 13] [--rate 30] [--capture DIR] [--out profiles/live.md]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def settings(frames):
    from splatam_amd import pipeline, slam
    demo = pipeline.replica_config(tracking_iters=60, mapping_iters=60, mapping_window_size=32,
                                   keyframe_every=max(int(frames // 5), 1) if frames < 25 else 5)
    demo['tracking'].update(use_depth_loss_thres=True, depth_loss_thres=20000,
                            lrs=dict(slam.REPLICA_TRACKING['lrs'], cam_unnorm_rots=0.001, cam_trans=0.004))
    demo['data'] = dict(desired_image_height=720, desired_image_width=960, densification_image_height=360, densification_image_width=480)
    # (raw colour w, h), (raw depth w, h), Gaussians of the synthetic scene, focal length at the raw size
    return {"splatam_s": (pipeline.splatam_s_config(1200, 680), (1200, 680), (1200, 680), 300_000, 600.0),
            "online_demo": (demo, (1920, 1440), (256, 192), 1_000_000, 960.0)}


def synthetic_frames(color_size, depth_size, n_gaussians, focal, frames):
    """[(rgb uint8 [H, W, 3], depth float32 [H', W'])] on the host, the intrinsics of the colour image, the true world-to-camera poses."""
    import torch
    from splatam_amd import pipeline, slam
    (W, H), (zw, zh) = color_size, depth_size
    ds = pipeline.SyntheticRGBDSequence(n_gaussians, W, H, focal, focal, W / 2 - 0.5, H / 2 - 0.5, num_frames=frames, seed=3, device=torch.device("cuda"))
    ys, xs = slam._nearest_index(zh, H, "cuda"), slam._nearest_index(zw, W, "cuda")
    out, gt = [], []
    for t in range(frames):
        color, depth, k, _ = ds[t]
        out.append((torch.round(color).clamp(0, 255).to(torch.uint8).cpu().numpy(), depth[..., 0][ys][:, xs].contiguous().cpu().numpy()))
        gt.append(ds.gt_w2c(t).cpu())
    return out, ds.k[:3, :3].cpu().numpy(), None, gt


def capture_frames(path, frames):
    import numpy as np
    from splatam_amd import datasets
    ds = datasets.NeRFCaptureDataset(basedir=os.path.dirname(os.path.abspath(path)), sequence=os.path.basename(os.path.abspath(path)),
                                     device="cpu", prefetch=0)
    n = min(frames, len(ds))
    out = [(np.array(datasets._decode_color(ds.color_paths[t])), np.array(datasets._decode_depth(ds.depth_paths[t]))) for t in range(n)]
    k = np.array([[ds.fx, 0, ds.cx], [0, ds.fy, ds.cy], [0, 0, 1]], dtype=np.float32)
    ds.close()
    return out, k, ds.png_depth_scale, None


def replay(name, cfg, frames, k, depth_scale, gt, rate):
    """One pass over ``frames``; ``rate``: None (as fast as the loop takes them) or frames per second."""
    import numpy as np
    import torch
    from splatam_amd import session
    dev = torch.device("cuda")
    torch.manual_seed(0)
    np.random.seed(0)
    latency, late, poses = [], 0, []
    with session.SlamSession(cfg, len(frames), engine="fused", device=dev) as s:
        s.add_raw_frame(frames[0][0], frames[0][1], k, depth_scale=depth_scale)         # set-up and allocations: not counted
        torch.cuda.synchronize(dev)
        start = time.perf_counter()
        for t in range(1, len(frames)):
            if rate is not None:
                due = start + (t - 1) / rate
                wait = due - time.perf_counter()
                if wait > 0:
                    time.sleep(wait)
                else:
                    late += t > 1                           # (due before its predecessor had finished)
            t0 = time.perf_counter()
            r = s.add_raw_frame(frames[t][0], frames[t][1], k, depth_scale=depth_scale)
            torch.cuda.synchronize(dev)                     # the pose is complete on the device
            latency.append(1e3 * (time.perf_counter() - t0))
            poses.append(r['w2c'])
        total = time.perf_counter() - start
        _, _, st = s.finish()
    n = len(latency)
    phases = {}
    for fr in st['phase_ms'][1:]:
        for key, v in fr.items():
            phases[key] = phases.get(key, 0.0) + v
    out = {"setting": name, "pacing_hz": rate, "frames_counted": n, "raw_colour": list(frames[0][0].shape[1::-1]), "raw_depth": list(frames[0][1].shape[1::-1]),
           "depth_dtype": str(frames[0][1].dtype), "tracking_iters": cfg['tracking']['num_iters'], "mapping_iters": cfg['mapping']['num_iters'],
           "frames_per_s": round(n / total, 3),
           "latency_ms": {"p50": round(float(np.percentile(latency, 50)), 2), "p95": round(float(np.percentile(latency, 95)), 2),
                          "max": round(max(latency), 2)},
           "tracking_iters_run": [d['tracking_iters'] for d in st['decisions'][1:]],
           "phase_ms_per_frame": {key: round(v / n, 3) for key, v in sorted(phases.items())},
           "rows_first_last": [st['num_gaussians'][0], st['num_gaussians'][-1]], "redone_iterations": st['redone_iterations']}
    if rate is not None:
        out["frames_due_before_predecessor_finished"] = int(late)
    if gt is not None:
        out["max_translation_error_m"] = round(max(float((p[:3, 3].cpu() - g[:3, 3]).norm()) for p, g in zip(poses, gt[1:])), 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="splatam_s,online_demo")
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--rate", type=float, default=30.0)
    ap.add_argument("--capture", default=None, help="a NeRFCapture directory (transforms.json, rgb/, depth/) instead of the synthetic sequence")
    ap.add_argument("--out", default=None, help="append the lines to this markdown file (box and commit first)")
    args = ap.parse_args()
    import torch
    lines = []
    every = settings(args.frames)
    for name in args.settings.split(","):
        cfg, color_size, depth_size, n_gaussians, focal = every[name]
        if args.capture:
            frames, k, depth_scale, gt = capture_frames(args.capture, args.frames)
        else:
            frames, k, depth_scale, gt = synthetic_frames(color_size, depth_size, n_gaussians, focal, args.frames)
        replay(name, cfg, frames[:3], k, depth_scale, None, None)                   # warm-up: clocks, the allocator, the lists' sizes
        for rate in (None, args.rate):
            lines.append(json.dumps(replay(name, cfg, frames, k, depth_scale, gt, rate)))
            print(lines[-1], flush=True)
    if args.out:
        try:
            head = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            head = "unknown"
        with open(args.out, "a") as f:
            f.write(f"\n`scripts/live_run.py --settings {args.settings} --frames {args.frames} --rate {args.rate}` on {socket.gethostname()} "
                    f"({torch.cuda.get_device_name(0)}), commit {head} + working tree:\n\n```\n" + "\n".join(lines) + "\n```\n")


if __name__ == "__main__":
    main()
