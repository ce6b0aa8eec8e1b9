"""The three frame entries (csrc/frameprep.hip) of TWO builds of the library, timed in one process: this tree's libsplat_hip.so against
``--other`` (for instance the parent commit's, built into a directory of its own).  The C entries are called directly, so only the
kernels and their launchers differ.  hipEvents around ``--launches`` back-to-back launches after a warm-up, as
scripts/ingest_planes_bench.py does it, the two libraries alternating, ``--repeats`` times: microseconds per CALL at that launch
cadence.  Cases: P1, P2 and P3 (uint16 depth) at 1200 x 680 -> 1200 x 680, and P3 from 1920 x 1440 bytes over a 256 x 192 float32
depth to 960 x 720.  One JSON line per case: both series, their medians, each library's run-to-run spread (max - min over min).

    python scripts/frame_path_ab.py --other /path/to/other/libsplat_hip.so [--launches 2000] [--repeats 7]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load(path):
    i, p, d = C.c_int32, C.c_void_p, C.c_double
    L = C.CDLL(path)
    L.splat_frame_prepare.argtypes = [i, i, p, p, i, i, p, p, p]
    L.splat_frame_ingest.argtypes = [i, i, p, i, i, p, d, i, i, p, p, p]
    L.splat_frame_ingest_planes.argtypes = [i, i, p, i, i, p, i, d, i, i, p, p, p]
    return L


def timed(fn, launches):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        assert fn() == 0
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    from splatam_amd import _capi
    libs = {"other": load(args.other), "this": load(_capi.LIB_PATH)}
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    up = lambda a: torch.from_numpy(a).to(dev)         # noqa: E731
    W, H = 1200, 680
    color, depth = up((rng.random((H, W, 3)) * 255).astype(np.float32)), up((0.5 + 4 * rng.random((H, W))).astype(np.float32))
    rgb, z16 = up(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)), up(rng.integers(0, 65536, size=(H, W)).astype(np.uint16))
    big, z32 = up(rng.integers(0, 256, size=(1440, 1920, 3), dtype=np.uint8)), up((0.5 + 4 * rng.random((192, 256))).astype(np.float32))
    a, b = torch.empty(3 * 1440 * 1920, device=dev), torch.empty(1440 * 1920, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pa, pb = a.data_ptr(), b.data_ptr()
    cases = {
        "P1 1200x680": lambda L: L.splat_frame_prepare(W, H, color.data_ptr(), depth.data_ptr(), W, H, pa, pb, s),
        "P2 1200x680": lambda L: L.splat_frame_ingest(W, H, rgb.data_ptr(), W, H, z16.data_ptr(), 6553.5, W, H, pa, pb, s),
        "P3 u16 1200x680": lambda L: L.splat_frame_ingest_planes(W, H, rgb.data_ptr(), W, H, z16.data_ptr(), _capi.SPLAT_DEPTH_U16, 6553.5, W, H, pa, pb, s),
        "P3 f32 1920x1440+256x192->960x720": lambda L: L.splat_frame_ingest_planes(1920, 1440, big.data_ptr(), 256, 192, z32.data_ptr(), _capi.SPLAT_DEPTH_F32,
                                                                                   1.0, 960, 720, pa, pb, s),
    }
    for name, call in cases.items():
        for L in libs.values():                                     # warm-up: clocks, code objects
            timed(lambda: call(L), args.launches)
        us = {k: [] for k in libs}
        for _ in range(args.repeats):
            for k, L in libs.items():
                us[k].append(timed(lambda: call(L), args.launches))
        print(json.dumps({"case": name, "launches": args.launches, **{k: {
            "us_per_call": [round(v, 3) for v in vals], "median_us": round(float(np.median(vals)), 3), "min_us": round(min(vals), 3),
            "max_us": round(max(vals), 3), "spread": round((max(vals) - min(vals)) / min(vals), 4)} for k, vals in us.items()}}), flush=True)


if __name__ == "__main__":
    main()
