"""What a checkpoint costs (splatam_amd/checkpoint.py, ``SlamSession.save_checkpoint`` / ``restore``), on the synthetic loop of
``bench.py``'s ``slam_loop``: 13 frames at 1200 x 680, ``replica_config()``, the map the loop builds (one Gaussian per valid first-frame
pixel, then densification).

    python scripts/checkpoint_run.py [--frames 13] [--dir DIR]          the costs: one JSON line
    python scripts/checkpoint_run.py --loop [--tree PATH] [--name NAME]  the loop with the keys off: ``bench.slam_loop_figure("B")`` of the
                                                                         tree at PATH (default: this one), one JSON line

The costs: the session is fed with ``add_frame`` as ``rgbd_slam`` feeds it; after frame 4 it checkpoints WITHOUT keyframe planes, after
frame 8 WITH them.  Reported per checkpoint: the milliseconds ``save_checkpoint`` held the caller (the device was idle when it was
called: the time is the copies to the host, their one synchronisation and the JSON), the time of the FOLLOWING frame (the writer thread
runs beside it) against the median of the run's other frames, how long the thread then still had to be waited for, and the bytes of
every file.  Then ``restore`` from each checkpoint in a fresh session -- keyframe planes from the dataset for the first, from
``keyframes8.npz`` for the second -- timed to the device being idle again, and the rest of the frames fed to the second.

The loop with the keys off is measured per TREE in a process of its own, so that a checkout of the parent commit can be run through the
same function (profiles/live.md section 1 does the same)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_figure(name):
    import torch
    import bench
    fig = bench.slam_loop_figure("B", torch.device("cuda"))
    runs = fig.pop("runs")
    return {"tree": name, "slam_loop": fig, "runs_frames_per_s": [r["frames_per_s"] for r in runs],
            "phase_ms_per_frame": runs[-1]["phase_ms_per_frame"], "gaussians_first_last": runs[-1]["gaussians_first_last"]}


def costs(frames, directory):
    import numpy as np
    import torch
    import bench
    from splatam_amd import pipeline
    from splatam_amd.session import SlamSession
    dev = torch.device("cuda")
    N, W, H, fx, fy, cx, cy = bench.WORKLOADS["B"]
    ds = pipeline.SyntheticRGBDSequence(N, W, H, fx, fy, cx, cy, num_frames=frames, seed=3, device=dev).preload()
    cfg = pipeline.replica_config()
    plan = {4: False, 8: True}                      # frame -> with keyframe planes

    def session():
        return SlamSession(cfg, frames, engine="fused", return_pose=False, reference_division=True)

    def run(checkpoints):
        torch.manual_seed(0)
        np.random.seed(0)
        saves, pending = {}, None
        with session() as s:
            for t in range(frames):
                s._begin_frame()
                s.add_frame(*ds[t])
                torch.cuda.synchronize(dev)
                if pending is not None:                 # the frame that ran beside the writer thread is done: how long is the thread still busy?
                    t0 = time.perf_counter()
                    written = s.join_checkpoint()
                    saves[pending].update(join_wait_ms=round(1e3 * (time.perf_counter() - t0), 2), bytes=written, next_frame=t)
                    pending = None
                if checkpoints and t in plan:
                    t0 = time.perf_counter()
                    s.save_checkpoint(directory, keyframes=plan[t])
                    saves[t] = dict(keyframes=plan[t], save_call_ms=round(1e3 * (time.perf_counter() - t0), 2), rows=s.stats['num_gaussians'][-1],
                                    keyframes_held=len(s.keyframe_list))
                    pending = t
            _, _, stats = s.finish()
        return stats, saves
    run(False)                                          # warm-up: clocks, the allocator, the lists' sizes
    plain, _ = run(False)
    stats, saves = run(True)
    frame_ms = [1e3 * x for x in stats['frame_s']]
    beside = {v['next_frame'] for v in saves.values()}
    others = [frame_ms[t] for t in range(1, frames) if t not in beside]
    for v in saves.values():
        v['next_frame_ms'] = round(frame_ms[v.pop('next_frame')], 2)
    out = {"frames": frames, "image": f"{W}x{H}", "rows_first_last": [stats['num_gaussians'][0], stats['num_gaussians'][-1]],
           "frame_ms_median_of_frames_without_a_writer": round(statistics.median(others), 2),
           "frame_ms_min_max_of_those": [round(min(others), 2), round(max(others), 2)],
           "frame_ms_median_of_a_run_without_checkpoints": round(statistics.median(1e3 * x for x in plain['frame_s'][1:]), 2),
           "checkpoints": {str(t): v for t, v in saves.items()}, "restores": {}}
    for t, with_planes in plan.items():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        s = SlamSession.restore(cfg, directory, t, dataset=None if with_planes else ds, engine="fused", return_pose=False)
        torch.cuda.synchronize(dev)
        out["restores"][str(t)] = dict(planes_from="keyframes file" if with_planes else "dataset", seconds=round(time.perf_counter() - t0, 3),
                                       keyframes=len(s.keyframe_list), rows=int(s.params['means3D'].shape[0]))
        if with_planes:
            with s:
                for u in range(t + 1, frames):
                    s.add_frame(*ds[u])
                _, _, st = s.finish()
            torch.cuda.synchronize(dev)
            out["restores"][str(t)].update(continued_to_rows=st['num_gaussians'][-1], straight_run_rows=stats['num_gaussians'][-1],
                                           redone_iterations=st['redone_iterations'],
                                           views_equal_the_straight_runs=[d['views'] for d in st['decisions']] == [d['views'] for d in stats['decisions']])
        else:
            s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", action="store_true", help="measure the loop with the checkpoint keys off instead of the costs")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose bench.py and package are measured")
    ap.add_argument("--name", default="this")
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--dir", default=None, help="where the checkpoints go (default: a temporary directory, removed afterwards)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if args.loop:
        print(json.dumps(loop_figure(args.name)), flush=True)
        return
    if args.dir is not None:
        print(json.dumps(costs(args.frames, args.dir)), flush=True)
        return
    with tempfile.TemporaryDirectory(prefix="splatam_checkpoint_run") as directory:
        print(json.dumps(costs(args.frames, directory)), flush=True)


if __name__ == "__main__":
    main()
