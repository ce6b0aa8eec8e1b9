"""What looking at the map costs (csrc/view.hip; ``FusedEngine.render_view``, ``SlamSession.render_view``).  One JSON line per part:

  finish   splat_view_finish alone at 1200 x 680 -- bytes only (colour and depth mode) and bytes plus cloud -- with hipEvents around
           ``--launches`` back-to-back launches after a warm-up, the forms alternating, ``--repeats`` times; microseconds per CALL at that
           cadence (no kernel trace is taken) and the GB/s of the ALGORITHMIC bytes (each plane read once, each output written once).
           ``splat_frame_ingest_planes`` at the same size is timed in the same process, for scale.
  call     a whole ``render_view`` (camera kernel + composite + finish kernel) plus the copy of ``rgb8`` into a pinned slot, on a map of
           300 000 Gaussians at 1200 x 680 (the size of ``bench.py``'s slam_loop scene) from a pose beside the map's: hipEvents around
           ``--calls`` calls, per call, and the host time the calls take to enqueue.
  live     ``scripts/live_run.py``'s SplaTAM-S setting paced at ``--rate`` Hz, without and with ``render_view(follow=True,
           to_host=True)`` after every frame: latency p50 / p95 from the call to the pose being complete on the device (without a
           view: a device synchronisation) or to the picture's event (with a view: what a consumer waits for; the copy is behind
           the pose on the loop's stream), how many frames were due before their predecessor had finished, and how many
           pictures came back truncated.

    python scripts/view_run.py [--parts finish,call,live] [--launches 2000] [--repeats 5] [--calls 200] [--frames 13] [--rate 30]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

W, H = 1200, 680


def timed(fn, launches):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches          # microseconds per call


def part_finish(args):
    import numpy as np
    import torch
    from splatam_amd import fused
    from splatam_amd.view import jet_lut
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    out6 = torch.from_numpy(rng.uniform(-0.1, 1.1, size=(6, H, W)).astype(np.float32)).to(dev)
    out6[3] = out6[3] * 5
    lut = torch.from_numpy(jet_lut()).to(dev)
    w2c = torch.eye(4, device=dev)
    k = (600.0, 600.0, W / 2 - 0.5, H / 2 - 0.5)
    rgb8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    pts, col = torch.empty(H * W, 3, device=dev), torch.empty(H * W, 3, device=dev)
    raw_rgb = torch.from_numpy(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
    raw_z = torch.from_numpy((0.5 + 4 * rng.random((H, W))).astype(np.float32)).to(dev)
    planes = (torch.empty(3, H, W, device=dev), torch.empty(1, H, W, device=dev))
    px = W * H
    forms = {"bytes_colour": (lambda: fused.view_finish(out6, "color", background=(1.0, 1.0, 1.0), rgb8=rgb8), px * (16 + 3)),
             "bytes_depth": (lambda: fused.view_finish(out6, "depth", lut=lut, rgb8=rgb8), px * (4 + 3)),
             "bytes_colour+cloud": (lambda: fused.view_finish(out6, "color", background=(1.0, 1.0, 1.0), rgb8=rgb8, points=pts, colors=col,
                                                              intrinsics=k, w2c=w2c), px * (20 + 3 + 24)),
             "ingest_planes_f32": (lambda: fused.ingest_planes(raw_rgb, raw_z, None, (H, W), out=planes), px * (3 + 4 + 16))}
    for fn, _ in forms.values():
        timed(fn, args.launches)
    us = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, (fn, _) in forms.items():
            us[name].append(timed(fn, args.launches))
    return {"part": "finish", "size": [W, H], "launches": args.launches, "forms": {
        name: {"us_per_call": [round(v, 2) for v in vals], "median_us": round(float(np.median(vals)), 2), "algorithmic_bytes": forms[name][1],
               "GB_per_s": round(forms[name][1] / (float(np.median(vals)) * 1e-6) / 1e9, 1)} for name, vals in us.items()}}


def part_call(args):
    import numpy as np
    import torch
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    dev = torch.device("cuda")
    f, cx, cy = 600.0, W / 2 - 0.5, H / 2 - 0.5
    params, variables = slam.synthetic_params(300_000, W, H, f, f, cx, cy, num_frames=2, seed=0, device="cuda")
    k = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    cam = slam.setup_camera(W, H, k, np.eye(4, dtype=np.float32), device="cuda")
    th = np.deg2rad(4.0)
    w2c = torch.tensor([[np.cos(th), 0, np.sin(th), 0.05], [0, 1, 0, -0.02], [-np.sin(th), 0, np.cos(th), 0.3], [0, 0, 0, 1]], dtype=torch.float32, device=dev)
    slot = torch.empty(H, W, 3, dtype=torch.uint8, pin_memory=True)
    out = {"part": "call", "size": [W, H], "gaussians": 300_000, "calls": args.calls}
    with torch.no_grad():
        eng = FusedEngine(params, cam, variables=variables)
        view = eng.view_camera(W, H)
        for _ in range(3):                          # the view camera learns its lists as any camera does
            eng.render_view(view, w2c=w2c, intrinsics=k, background=(1.0, 1.0, 1.0))
            if not view.check_overflow():
                break
        out["lists"] = {"tile_stride": view.camera.tile_stride, "longest_list": view.camera.max_list_hint}

        def call():
            image = eng.render_view(view, w2c=w2c, intrinsics=k, background=(1.0, 1.0, 1.0))
            slot.copy_(image.rgb8, non_blocking=True)
        timed(call, args.calls)
        vals, host = [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals.append(timed(call, args.calls))
            host.append(1e6 * (time.perf_counter() - t0) / args.calls)
        out["us_per_call"] = [round(v, 1) for v in vals]
        out["median_us"] = round(float(np.median(vals)), 1)
        out["truncated"] = int(view.truncated)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        out["host_enqueue_us_per_call"] = round(1e6 * (time.perf_counter() - t0) / args.calls, 1)
        torch.cuda.synchronize()
    return out


def part_live(args):
    import numpy as np
    import torch
    import live_run
    from splatam_amd import session
    cfg, color_size, depth_size, n_gaussians, focal = live_run.settings(args.frames)["splatam_s"]
    frames, k, depth_scale, _ = live_run.synthetic_frames(color_size, depth_size, n_gaussians, focal, args.frames)
    dev = torch.device("cuda")
    lines = []
    for with_view in (False, True, False, True):
        torch.manual_seed(0)
        np.random.seed(0)
        latency, late = [], 0
        with session.SlamSession(cfg, len(frames), engine="fused", device=dev) as s:
            s.add_raw_frame(frames[0][0], frames[0][1], k, depth_scale=depth_scale)
            if with_view:                           # the first picture, then the digest that sizes the view's lists (as a consumer would)
                for _ in range(3):
                    s.render_view(follow=True, to_host=True, background=(1.0, 1.0, 1.0)).event.synchronize()
                    if not s.view_check_overflow():
                        break
            truncated = 0
            torch.cuda.synchronize(dev)
            start = time.perf_counter()
            for t in range(1, len(frames)):
                due = start + (t - 1) / args.rate
                wait = due - time.perf_counter()
                if wait > 0:
                    time.sleep(wait)
                else:
                    late += t > 1
                t0 = time.perf_counter()
                s.add_raw_frame(frames[t][0], frames[t][1], k, depth_scale=depth_scale)
                if with_view:                       # the consumer's wait: the event behind the picture's copy (which is behind the pose)
                    picture = s.render_view(follow=True, to_host=True, background=(1.0, 1.0, 1.0))
                    picture.event.synchronize()
                    truncated += int(picture.truncated[0] != 0)
                else:
                    torch.cuda.synchronize(dev)     # the pose is complete on the device
                latency.append(1e3 * (time.perf_counter() - t0))
            s.finish()
        lines.append({"part": "live", "setting": "splatam_s", "pacing_hz": args.rate, "view_per_frame": with_view, "frames_counted": len(latency),
                      "latency_ms": {"p50": round(float(np.percentile(latency, 50)), 2), "p95": round(float(np.percentile(latency, 95)), 2),
                                     "max": round(max(latency), 2)}, "frames_due_before_predecessor_finished": int(late),
                      "truncated_pictures": int(truncated) if with_view else None})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="finish,call,live")
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--rate", type=float, default=30.0)
    args = ap.parse_args()
    for part in args.parts.split(","):
        out = {"finish": part_finish, "call": part_call, "live": part_live}[part](args)
        for line in (out if isinstance(out, list) else [out]):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
