"""The view overlay (csrc/viewoverlay.hip) measured on bench.py's workload B map -- 300 000 Gaussians, 1200 x 680 -- with a synthetic run
of 2 000 frames (17 999 segments: 1 999 of trajectory, 16 000 of frusta), seen from a camera a metre and a half behind the first pose.
One JSON line:

  kernels_us      microseconds per launch of each kernel alone, hipEvents around ``--launches`` back-to-back launches, ``--repeats``
                  times (all repeats are listed: their spread is the noise): run_segments (2 000 frames), clear, points (300 000
                  rows, size 1), segments_all (17 999), segments_current (the trajectory and one frustum: 2 007), finish
  render_view_us  the whole ``FusedEngine.render_view`` call the same way, the configurations ALTERNATING inside every repeat so that
                  none has the warmer machine: plain (``mode="color"``, no overlay: code the parent commit has), centers,
                  color_all (``frusta="all"``), color_current (``frusta="current"``)
  ratio           each configuration's median over plain's median
  drawn           pixels of the key plane that hold a point / a segment in the configurations (the pictures show something)

    python scripts/view_overlay_run.py [--frames 2000] [--launches 20] [--repeats 5] [--warmup 3] [--line-width 1] [--point-size 1]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from mesh_run import CX, CY, FX, FY, H, N, W, timed  # noqa: E402


def scene(frames):
    """Workload B's map with a run of ``frames`` poses on a slow arc through the room (a few metres in all, like a Replica sequence)."""
    import numpy as np
    import torch
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables = slam.synthetic_params(N, W, H, FX, FY, CX, CY, num_frames=frames, seed=0, device="cuda")
    t = torch.arange(frames, dtype=torch.float32, device="cuda")
    ang = 0.6 * torch.sin(t * (2 * math.pi / frames))
    with torch.no_grad():
        params['cam_unnorm_rots'][0, 0], params['cam_unnorm_rots'][0, 2] = torch.cos(ang / 2), torch.sin(ang / 2)
        params['cam_unnorm_rots'][0, 1] = params['cam_unnorm_rots'][0, 3] = 0.0
        params['cam_trans'][0, 0] = 0.8 * torch.sin(t * (4 * math.pi / frames))
        params['cam_trans'][0, 1] = 0.2 * torch.sin(t * (6 * math.pi / frames))
        params['cam_trans'][0, 2] = -0.6 * (1 - torch.cos(t * (2 * math.pi / frames)))
        cam = slam.setup_camera(W, H, [[FX, 0, CX], [0, FY, CY], [0, 0, 1]], np.eye(4, dtype=np.float32), device="cuda")
        eng = FusedEngine(params, cam, variables=variables)
        view = eng.view_camera(W, H)
    return eng, view


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--line-width", type=int, default=1)
    ap.add_argument("--point-size", type=int, default=1)
    args = ap.parse_args()
    import torch
    from splatam_amd import _capi
    from splatam_amd.view import RunOverlay
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    eng, view = scene(args.frames)
    k = (FX, FY, CX, CY)
    w2c = torch.eye(4, device="cuda")
    w2c[2, 3] = 1.5                                            # a metre and a half behind the first pose: the run lies in the picture
    with torch.no_grad():
        overlay = RunOverlay(eng, args.frames, intrinsics=k, size=(W, H))
        configs = {
            "plain": dict(mode="color"),
            "centers": dict(mode="centers", point_size=args.point_size),
            "color_all": dict(mode="color", overlay=overlay, frusta="all", line_width=args.line_width),
            "color_current": dict(mode="color", overlay=overlay, frusta="current", line_width=args.line_width),
        }
        for _ in range(3):                                     # the view's lists sized and learnt, as a viewer's are after its first frames
            eng.render_view(view, w2c=w2c, intrinsics=k)
            if not view.check_overflow():
                break
        drawn = {}
        for name, kw in configs.items():
            for _ in range(args.warmup):
                image = eng.render_view(view, w2c=w2c, intrinsics=k, overlay_planes=name != "plain", **kw)
            if name != "plain":
                key = image.key
                drawn[name] = {"points": int(((key >= 0) & (key.bitwise_and(1 << 31) == 0)).sum()), "segments": int(((key >= 0) & (key.bitwise_and(1 << 31) != 0)).sum())}
        assert int(image.truncated) == 0
        # the kernels alone
        L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
        ov = view.overlay_args()
        n = args.frames
        f = _capi.SplatViewOverlayFinish()
        f.depth, f.occlude, f.fill = view.camera.buf['out6'][3].data_ptr(), 1, 0
        f.rgb_colors, f.num_rows = eng.params['rgb_colors'].data_ptr(), eng.P
        f.segment_colors, f.num_segments, f.rgb8 = overlay.colors.data_ptr(), overlay.num_segments, view.rgb8.data_ptr()
        seg, means = overlay.segments.data_ptr(), eng.params['means3D'].data_ptr()

        def current():
            L.splat_view_segments(C.byref(ov), seg, 0, n - 1, args.line_width, stream)
            L.splat_view_segments(C.byref(ov), seg, n - 1 + 8 * (n - 1), 8, args.line_width, stream)
        kernels = {
            "run_segments": lambda: overlay.refresh(),
            "clear": lambda: L.splat_view_overlay_clear(C.byref(ov), stream),
            "points": lambda: L.splat_view_points(C.byref(ov), means, eng.P, args.point_size, stream),
            "segments_all": lambda: L.splat_view_segments(C.byref(ov), seg, 0, 9 * n - 1, args.line_width, stream),
            "segments_current": current,
            "finish": lambda: L.splat_view_overlay_finish(C.byref(ov), C.byref(f), stream),
        }
        out = {"frames": n, "segments": overlay.num_segments, "gaussians": eng.P, "size": [W, H], "launches": args.launches, "repeats": args.repeats,
               "line_width": args.line_width, "point_size": args.point_size, "drawn": drawn, "kernels_us": {}, "render_view_us": {}, "ratio": {}}
        for name, fn in kernels.items():
            for _ in range(args.warmup):
                fn()
            out["kernels_us"][name] = [round(timed(fn, args.launches), 1) for _ in range(args.repeats)]
        times = {name: [] for name in configs}
        for _ in range(args.repeats):
            for name, kw in configs.items():
                times[name].append(round(timed(lambda: eng.render_view(view, w2c=w2c, intrinsics=k, **kw), args.launches), 1))
        out["render_view_us"] = times
        plain = statistics.median(times["plain"])
        out["ratio"] = {name: round(statistics.median(v) / plain, 3) for name, v in times.items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
