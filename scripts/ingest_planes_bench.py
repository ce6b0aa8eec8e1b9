"""``fused.ingest_planes`` (one launch: csrc/frameprep.hip P3) against ``fused.ingest_frame`` + ``fused.prepare_frame`` (P2 then P1, the
0..255 frame written and read again in between) on a phone's frame: 1920 x 1440 RGB bytes over a 256 x 192 float32 depth image (uint16
for the pair, which takes no float depth) to 960 x 720 and to 480 x 360.  hipEvents around ``--launches`` back-to-back launches after a
warm-up, the three forms alternating, ``--repeats`` times in one process; microseconds per CALL at that launch cadence (not the kernel's own duration: no kernel trace is taken) and, from it, the GB/s of the
ALGORITHMIC bytes (the colour image once, the depth pixels an output reads, the planes written once; for the pair also the frame
in between, written and read).  One JSON line per destination size.

    python scripts/ingest_planes_bench.py [--launches 2000] [--repeats 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CW, CH, ZW, ZH = 1920, 1440, 256, 192


def timed(fn, launches):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from splatam_amd import fused
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    rgb = torch.from_numpy(rng.integers(0, 256, size=(CH, CW, 3), dtype=np.uint8)).to(dev)
    z32 = torch.from_numpy((0.5 + 4 * rng.random((ZH, ZW))).astype(np.float32)).to(dev)
    z16 = torch.from_numpy(rng.integers(0, 65536, size=(ZH, ZW)).astype(np.uint16)).to(dev)
    for h, w in ((720, 960), (360, 480)):
        planes = (torch.empty(3, h, w, device=dev), torch.empty(1, h, w, device=dev))
        frame = (torch.empty(h, w, 3, device=dev), torch.empty(h, w, 1, device=dev))
        forms = {"ingest_planes_f32": lambda: fused.ingest_planes(rgb, z32, None, (h, w), out=planes),
                 "ingest_planes_u16": lambda: fused.ingest_planes(rgb, z16, 6553.5, (h, w), out=planes),
                 "ingest_frame+prepare_frame_u16": lambda: fused.prepare_frame(*fused.ingest_frame(rgb, z16, 6553.5, (h, w), out=frame), out=planes)}
        depth_read = min(ZW * ZH, w * h)
        out_bytes = 16 * h * w
        algorithmic = {"ingest_planes_f32": CW * CH * 3 + 4 * depth_read + out_bytes, "ingest_planes_u16": CW * CH * 3 + 2 * depth_read + out_bytes,
                       "ingest_frame+prepare_frame_u16": CW * CH * 3 + 2 * depth_read + 3 * out_bytes}
        for fn in forms.values():                                   # warm-up: clocks, code objects
            timed(fn, args.launches)
        us = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name, fn in forms.items():
                us[name].append(timed(fn, args.launches))
        torch.cuda.synchronize(dev)
        print(json.dumps({"colour": [CW, CH], "depth": [ZW, ZH], "destination": [w, h], "launches": args.launches, "forms": {
            name: {"us_per_call": [round(v, 2) for v in vals], "median_us": round(float(np.median(vals)), 2),
                   "spread": round((max(vals) - min(vals)) / min(vals), 4), "algorithmic_bytes": algorithmic[name],
                   "GB_per_s": round(algorithmic[name] / (float(np.median(vals)) * 1e-6) / 1e9, 1)} for name, vals in us.items()}}), flush=True)


if __name__ == "__main__":
    main()
