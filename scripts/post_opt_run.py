#!/usr/bin/env python3
"""The refinement of a finished map (splatam_amd/post_opt.py) on a synthetic map of bench.py's workload B, on the device:

  1. the DRIVER: the map is written as the ``params.npz`` of a finished run, its keyframe views become the mapping dataset, and
     ``post_splatam_opt(engine="fused")`` refines it with the reference's configuration (configs/replica/post_splatam_opt.py: loss
     weights, rates, densification thresholds) on a schedule scaled to ``--iters``.  Printed: iterations/s of an untimed run, and from a
     second, bracketed run (a device synchronisation around every call) the phase split of an iteration while densification
     accumulates -- loss + backward, the colour pass' means2D gradient (the extra 3-channel backward composite of
     splat_iter_means2d_accumulate), densify, Adam -- with the SHARE of the means2D pass: the number a follow-up that forms that
     gradient inside the mapping backward composite would be judged on;
  2. gs against what the parent could express: two sequences on the same seeded map, alternating ``--alternations`` times in one
     process -- (a) ``loss_backward(gs)`` (b) ``loss_backward(mapping)``, each followed by ``accumulate_mean2d_gradient``, ``densify`` (one
     scheduled densification in the middle of the block) and ``adam_map``.  Warm-up as bench.py describes it: the schedule runs for
     >= 0.15 s before the first block (clocks), every block restores the seeded map and runs untimed warm-up iterations (which also
     learn the list statistics) before its timed ones.  (a) must not be slower than (b) by more than (b)'s own run-to-run spread.

Prints one JSON line at the end (and writes it to ``--out``)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

LRS = dict(means3D=0.00032, rgb_colors=0.0025, unnorm_rotations=0.001, logit_opacities=0.05, log_scales=0.005, cam_unnorm_rots=0.0, cam_trans=0.0)
WEIGHTS = dict(im=0.5, depth=1.0)


class _Views:
    """The keyframe views of a bench scene as a dataset: (colour 0..255 [H,W,3], depth [H,W,1], intrinsics [4,4], camera-to-world)."""

    def __init__(self, frames, k4, dev):
        self.items = [((f['im'].permute(1, 2, 0) * 255.0).contiguous(), f['depth'].permute(1, 2, 0).contiguous(), k4, torch.eye(4, device=dev))
                      for f in frames]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, t):
        return self.items[t]


def densify_dict(iters):
    """configs/replica/post_splatam_opt.py's thresholds on a schedule scaled from 15 000 iterations to ``iters``."""
    s = iters / 15000.0
    return dict(start_after=max(int(500 * s), 1), remove_big_after=max(int(3000 * s), 1), stop_after=iters, densify_every=max(int(100 * s * 5), 2),
                grad_thresh=0.0002, num_to_split_into=2, removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005,
                reset_opacities=True, reset_opacities_every=max(int(3000 * s), 2))


def driver_runs(workload, views, iters, dev):
    import bench
    from splatam_amd import post_opt
    N, W, H, fx, fy, cx, cy = bench.WORKLOADS[workload]
    params, variables, frames, _ = bench.build_scene(workload, dev, views)
    order = sorted(frames)[1:]                                        # the keyframe views (frame 1 is bench.py's tracking frame)
    k4 = torch.tensor([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32, device=dev)
    ds = _Views([frames[t] for t in order], k4, dev)
    tmp = tempfile.mkdtemp(prefix="post_opt_run_")
    ckpt = {k: v.detach().cpu().numpy() for k, v in params.items()}
    for k in ('cam_unnorm_rots', 'cam_trans'):                        # the poses of the views, in the dataset's order
        ckpt[k] = ckpt[k][..., order]
    n = ckpt['means3D'].shape[0]
    ckpt.update(timestep=np.zeros(n, dtype=np.float32), intrinsics=k4[:3, :3].cpu().numpy(), w2c=np.eye(4, dtype=np.float32), org_width=W,
                org_height=H, gt_w2c_all_frames=np.stack([np.eye(4, dtype=np.float32)] * len(order)), keyframe_time_indices=np.arange(len(order)))
    path = os.path.join(tmp, "params.npz")
    np.savez(path, **ckpt)
    config = dict(workdir=tmp, run_name="refined", seed=0, primary_device=str(dev), report_iter_progress=False, use_wandb=False,
                  data=dict(desired_image_height=H, desired_image_width=W, num_frames=len(order), eval_num_frames=len(order), param_ckpt_path=path),
                  train=dict(num_iters_mapping=iters, sil_thres=0.5, loss_weights=WEIGHTS, lrs_mapping=dict(LRS), lrs_mapping_means3D_final=0.0000032,
                             lr_delay_mult=0.01, use_gaussian_splatting_densification=True, densify_dict=densify_dict(iters)))
    out = {}
    for name, timed in (("untimed", False), ("bracketed", True)):
        import random
        random.seed(0)
        torch.manual_seed(0)
        _, _, stats, _ = post_opt.post_splatam_opt(json.loads(json.dumps(config)), engine="fused", dataset=ds, evaluate=False, timed=timed)
        rows = [r[2] for r in stats['rows']]
        out[name] = dict(iterations=iters, loop_s=round(stats['loop_s'], 4), iterations_per_s=round(iters / stats['loop_s'], 1),
                         densifications=len(stats['rows']), rows_start=n, rows_end=rows[-1] if rows else n, redone_iterations=stats['redone_iterations'])
        if timed:
            ph = {k: round(v, 4) for k, v in stats['phase_s'].items()}
            core = sum(ph.get(k, 0.0) for k in ("loss_backward", "means2d_accumulate", "densify", "adam", "relearn_lists"))
            out[name]['phase_s'] = ph
            out[name]['phase_share'] = {k: round(ph.get(k, 0.0) / core, 4) for k in ("loss_backward", "means2d_accumulate", "densify", "adam", "relearn_lists")}
        print(f"[driver/{name}] {json.dumps(out[name])}", flush=True)
        stats.pop('engine', None)
        torch.cuda.empty_cache()
    return out


def alternation(workload, views, alternations, steps, warmup, dev):
    """(a) the gs iteration against (b) the sequence the parent could express, on the same seeded map, alternating."""
    import bench
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frames, (N, W, H) = bench.build_scene(workload, dev, views)
    order = sorted(frames)[1:]
    seed = {k: v.detach().clone() for k, v in params.items()}
    scene_radius = float(torch.max(frames[order[0]]['depth']) / 2.0)
    eng = FusedEngine(params, frames[order[0]]['cam'], gaussian_capacity=int(1.5 * N) + 65536, variables=variables)
    eng.keep_map_grads = False
    modes = {"gs": dict(loss='gs', loss_weights=WEIGHTS, lrs=LRS), "mapping": dict(slam.REPLICA_MAPPING, loss_weights=WEIGHTS, lrs=LRS)}
    # one scheduled densification in the middle of a block's timed iterations, accumulation in every iteration
    dd = dict(densify_dict(15000), start_after=warmup + steps // 2, densify_every=warmup + steps // 2, stop_after=10 ** 9, remove_big_after=10 ** 9,
              reset_opacities_every=10 ** 9)

    def iterate(cfg, first, count):
        for it in range(first, first + count):
            t = order[it % len(order)]
            eng.loss_backward(frames[t], t, cfg, tracking=False)
            eng.accumulate_mean2d_gradient()
            scheduled = slam.edit_schedule(it, dd, 'densify_every').edits
            edited = eng.densify(it, dd, scene_radius, accumulate=False)
            if edited and not eng.lists_known():
                eng.relearn_lists(frames[t], t)
            if not scheduled:
                eng.adam_map(cfg['lrs'])

    def block(cfg):
        eng.replace_map(seed)
        eng.reset_map_optimizer()
        iterate(cfg, 0, warmup - 3)
        torch.cuda.synchronize(dev)
        if eng.check_overflow():
            raise SystemExit("instance lists overflowed during warm-up")
        iterate(cfg, warmup - 3, 3)
        torch.cuda.synchronize(dev)
        if eng.check_overflow():
            raise SystemExit("instance lists overflowed during warm-up")
        rows0 = eng.P
        t0 = time.perf_counter()
        iterate(cfg, warmup, steps)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if eng.check_overflow():
            raise SystemExit("instance lists overflowed in a timed block")
        return steps / dt, rows0, eng.P

    t0 = time.perf_counter()                                          # clock pre-warm: the schedule itself, both modes, >= 0.15 s
    while time.perf_counter() - t0 < 0.15:
        for cfg in modes.values():
            block(cfg)
    series = {k: [] for k in modes}
    rows = {}
    for i in range(alternations):
        for name in (("gs", "mapping") if i % 2 == 0 else ("mapping", "gs")):
            rate, r0, r1 = block(modes[name])
            series[name].append(round(rate, 1))
            rows[name] = (r0, r1)
    a, b = np.array(series["gs"]), np.array(series["mapping"])
    spread = float(b.max() - b.min())
    out = dict(workload=workload, rows=N, steps=steps, warmup=warmup, alternations=alternations, gs_iterations_per_s=series["gs"],
               mapping_iterations_per_s=series["mapping"], rows_in_block=rows, gs_median=float(np.median(a)), mapping_median=float(np.median(b)),
               mapping_spread=round(spread, 1), gs_minus_mapping=round(float(np.median(a) - np.median(b)), 1),
               gs_not_slower=bool(np.median(a) >= np.median(b) - spread))
    print(f"[alternation] {json.dumps(out)}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", default="B")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--iters", type=int, default=600, help="iterations of the driver runs (the reference's schedule scaled from 15 000)")
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100, help="timed iterations per block of the alternation")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-driver", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("post_opt_run.py needs a GPU")
    dev = torch.device("cuda:0")
    result = {}
    result['alternation'] = alternation(args.workload, args.views, args.alternations, args.steps, args.warmup, dev)
    if not args.skip_driver:
        result['driver'] = driver_runs(args.workload, args.views, args.iters, dev)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if result['alternation']['gs_not_slower'] else 1


if __name__ == "__main__":
    sys.exit(main())
