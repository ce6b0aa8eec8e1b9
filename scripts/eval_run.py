#!/usr/bin/env python3
"""Runs the synthetic RGB-D sequence through ``pipeline.rgbd_slam(evaluate=...)`` and prints ONE JSON line: the averages of the
evaluation (PSNR, depth L1, MS-SSIM, ATE) and ``eval_ms_per_frame``.

``--compare-torch``: additionally times the metric kernels (``fused.evaluate_metrics``) against the torch form of the same metrics
(``slam.eval_frame_metrics`` with ``slam.ms_ssim``, everything on the device) on the SAME device planes -- one rendered frame of the
final map and its RGB-D frame --, alternating between the two in this process, after a warm-up of each, ``--compare-frames`` frames
per side in total, every timed block ended by a device synchronise.  The torch form is the only other implementation of these
metrics that runs on the device; there is no earlier version of the kernels to compare with."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def compare_torch(ds, params, frames_per_side, rounds=4, warmup=10):
    from splatam_amd import fused, slam
    from splatam_amd.fused import FusedEngine
    color, depth, intr, pose = ds[0]
    color, depth = (color.permute(2, 0, 1) / 255).contiguous(), depth.permute(2, 0, 1).contiguous()
    w2c = torch.linalg.inv(pose).float().contiguous()
    cam = slam.setup_camera(color.shape[2], color.shape[1], intr[:3, :3].cpu().numpy(), w2c.cpu().numpy(), device=color.device)
    curr = {'cam': cam, 'im': color, 'depth': depth, 'id': 0, 'w2c': w2c}
    eng = FusedEngine({k: v.detach().float().contiguous() for k, v in params.items()}, cam)
    eng.relearn_lists(curr, 0)
    im, d, sil, _ = (t.clone() for t in eng.render(curr, 0))
    depth_sil = torch.cat([d, sil[None]]).contiguous()
    per = max(1, frames_per_side // rounds)
    table = torch.zeros(per, 8, dtype=torch.float64, device=color.device)

    def kernels(n):
        for i in range(n):
            fused.evaluate_metrics(im, d, sil, curr, table[i % per], 0.5, sil_mask=False, ms_ssim=True)

    def torch_form(n):
        out = None
        with torch.no_grad():
            for _ in range(n):
                out = slam.eval_frame_metrics(im, depth_sil, curr, 0.5, False)
        return out
    kernels(warmup)
    last = torch_form(warmup)
    torch.cuda.synchronize()
    t_k = t_t = 0.0
    for _ in range(rounds):
        t0 = time.perf_counter()
        kernels(per)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        last = torch_form(per)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_k, t_t = t_k + (t1 - t0), t_t + (t2 - t1)
    n = per * rounds
    row = table[0].cpu().numpy()
    return {'frames_per_side': n, 'size': [int(color.shape[2]), int(color.shape[1])], 'kernels_ms_per_frame': 1e3 * t_k / n,
            'torch_ms_per_frame': 1e3 * t_t / n, 'torch_over_kernels': t_t / t_k,
            'kernels': {'psnr': float(row[0]), 'depth_l1': float(row[2]), 'ms_ssim': float(row[3])},
            'torch': {'psnr': float(last['psnr']), 'depth_l1': float(last['depth_l1']), 'ms_ssim': float(last['ms_ssim'])}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--gaussians", type=int, default=400000, help="splats of the synthetic scene the frames are rendered from")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--tracking-iters", type=int, default=10)
    ap.add_argument("--mapping-iters", type=int, default=15)
    ap.add_argument("--engine", default="fused", choices=["fused", "dropin"])
    ap.add_argument("--eval-every", type=int, default=1)
    ap.add_argument("--eval-dir", default=None)
    ap.add_argument("--no-ms-ssim", action="store_true")
    ap.add_argument("--compare-torch", action="store_true")
    ap.add_argument("--compare-frames", type=int, default=200, help="frames per side of --compare-torch")
    a = ap.parse_args()
    from splatam_amd import pipeline
    W, H = a.width, a.height
    f = 0.5 * W
    ds = pipeline.SyntheticRGBDSequence(a.gaussians, W, H, f, f, W / 2 - 0.5, H / 2 - 0.5, num_frames=a.frames, seed=2, step_m=0.012,
                                        step_deg=0.4).preload()
    cfg = pipeline.replica_config(tracking_iters=a.tracking_iters, mapping_iters=a.mapping_iters, keyframe_every=2)
    torch.manual_seed(0)
    np.random.seed(0)
    t0 = time.perf_counter()
    params, _, stats = pipeline.rgbd_slam(ds, cfg, engine=a.engine, evaluate=dict(eval_every=a.eval_every, eval_dir=a.eval_dir,
                                                                                  ms_ssim=not a.no_ms_ssim))
    torch.cuda.synchronize()
    ev = stats['eval']
    out = {'size': [W, H], 'frames': a.frames, 'engine': a.engine, 'gaussians_final': stats['num_gaussians'][-1], 'run_s': time.perf_counter() - t0,
           'evaluated_frames': ev['frames'], 'avg_psnr': ev['avg_psnr'], 'avg_depth_rmse': ev['avg_depth_rmse'], 'avg_depth_l1': ev['avg_depth_l1'],
           'avg_ms_ssim': ev['avg_ms_ssim'], 'ate_rmse': ev['ate_rmse'], 'lpips': ev['lpips'], 'eval_ms_per_frame': ev['eval_ms_per_frame'],
           'repeated': ev['repeated']}
    if a.compare_torch:
        out['compare_torch'] = compare_torch(ds, params, a.compare_frames)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
