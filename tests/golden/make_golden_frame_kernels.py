"""Generates tests/golden/frame_kernels_reference.npz: the outputs of the three frame entry points (``prepare_frame``, ``ingest_frame``,
``ingest_planes``: csrc/frameprep.hip) AS THE LIBRARY OF ONE COMMIT COMPUTES THEM ON THE DEVICE, bit for bit, so that a later change
of the kernels can be held to them (tests/test_gpu_frame_golden.py).  The kernels have no atomics and IEEE divisions: one differing
bit means that the order of operations changed.

Cases (tests/frame_ref.py ``golden_frame_kernel_runs``): ``frame_ref.SIZES`` for prepare_frame (a seeded depth and the special-float
depth), ``frame_ref.RAW_CASES`` for ingest_frame and ingest_planes (uint16 depth at scale 6553.5; for the planes the special-float
depth too).  Every case runs with its outputs on a 16-byte boundary (lead 64) and off it (lead 61); the generator REQUIRES the two to
agree in every bit and records the one result, which the test then demands of both leads.  The inputs are regenerated from the seeds
(stored as ``seed_rule``), only outputs are recorded, as their uint32 views.

Run on a machine with the device, at the commit to record:  python tests/golden/make_golden_frame_kernels.py [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import frame_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "frame_kernels_reference.npz"))
    ap.add_argument("--commit", default=None, help="the commit whose library runs (default: git rev-parse HEAD)")
    args = ap.parse_args()
    from splatam_amd import fused
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True, check=True).stdout.strip()
    out = {}
    for (key, a, b), (key61, a61, b61) in zip(frame_ref.golden_frame_kernel_runs(fused, 64), frame_ref.golden_frame_kernel_runs(fused, 61)):
        assert key == key61
        a, b, a61, b61 = (x.view(np.uint32) for x in (a, b, a61, b61))
        assert np.array_equal(a, a61) and np.array_equal(b, b61), f"{key}: the 16-byte and the scalar stores disagree"
        out[key + "/colour"], out[key + "/depth"] = a.copy(), b.copy()
    out["commit"] = np.array(commit)
    out["scale"] = np.array(frame_ref.GOLDEN_SCALE)
    out["seed_rule"] = np.array("frame/raw: 100 * source width + destination width; special floats: 10 * depth width + destination width")
    out["sizes"] = np.array(frame_ref.SIZES, dtype=np.int32)
    out["raw_cases"] = np.array(frame_ref.RAW_CASES, dtype=np.int32)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(out) - 5} arrays of {commit[:12]}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
