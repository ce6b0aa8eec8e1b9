"""What aligning a reconstruction costs (csrc/icp.hip; ``splatam_amd.mesh_score.align_icp``).  One JSON line per measurement, on
two-surface synthetic clouds: ``--sizes`` source points sampled (seed 2) on the two-box mesh of tests/icp_ref.py moved by G^-1 (3 degrees,
2.7 cm), against as many targets sampled with seed 1.

  steps      one iteration split into its launches, each with hipEvents over ``--launches`` back-to-back calls, ``--repeats`` times (the
             median and the spread): I1 transform, the cell keys + ``torch.sort`` of the queries, the grid's query with the order given,
             I2 accumulate, I3 solve.  Measured at the start pose, where the query walks furthest.
  whole      ``align_icp`` end to end (grid built inside, wall clock around a synchronise), evaluations, status, host reads, and the
             same with the grid built before.
  resort     ``align_icp`` with the queries re-sorted by cell every iteration, every 5th, every 10th and once; the results must be the
             same bits.
  reads      host reads of the state per run at ``check_every`` 1, 5 and 31.

    python scripts/icp_run.py [--parts steps,whole,resort,reads] [--sizes 200000,1000000,4000000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, launches):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches          # microseconds per call


def spread(fn, launches, repeats):
    import numpy as np
    t = [timed(fn, launches) for _ in range(repeats)]
    return {"us": round(float(np.median(t)), 2), "min": round(min(t), 2), "max": round(max(t), 2)}


def clouds(n):
    """(source, target) float32 [n, 3] on the device, sampled there."""
    import numpy as np
    import torch
    import icp_ref as I
    from splatam_amd import mesh_score as S
    v, f = I.two_box_mesh()
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    target = S.sample_surface(dv, df, n, 1)[0]
    inv = np.linalg.inv(I.G)
    state = torch.from_numpy(np.concatenate((inv.reshape(-1), np.zeros(8)))).cuda()
    source = S.apply_state(S.sample_surface(dv, df, n, 2)[0], state)
    return source, target


def wall(fn, repeats):
    import numpy as np
    import torch
    out, t = None, []
    for _ in range(repeats + 1):                              # (the first is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    t = t[1:]
    return out, {"ms": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def part_steps(args, n, source, target):
    import numpy as np
    import torch
    from splatam_amd import _capi
    from splatam_amd import mesh_score as S
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    grid = S.NearestGrid(target)
    state = torch.from_numpy(np.concatenate((np.eye(4).reshape(-1), np.zeros(8)))).cuda()
    moved = S.apply_state(source, state)
    order = grid.cell_order(moved)
    dist2, index = grid.query(moved, order=order)
    partials = torch.zeros(_capi.SPLAT_ICP_ROWS, _capi.SPLAT_ICP_SUMS, dtype=torch.float64, device="cuda")
    origin = [grid.lo[k] + 0.5 * grid.cell * grid.dims[k] for k in range(3)]
    c = (C.c_double * 3)(*origin)
    history = torch.zeros(31, 4, dtype=torch.float64, device="cuda")
    saved = state.clone()

    def solve():
        state.copy_(saved)                                    # (status 0 again: the solve runs every time; the 192-byte copy is in the figure)
        _capi.check(L.splat_icp_solve(partials.data_ptr(), n, 30, 1e-6, 1e-6, c, state.data_ptr(), history.data_ptr(), stream), "splat_icp_solve")
    out = {"part": "steps", "n": n, "grid": list(grid.dims), "cell": grid.cell, "launches": args.launches, "repeats": args.repeats}
    out["transform"] = spread(lambda: S.apply_state(source, state, out=moved), args.launches, args.repeats)
    out["keys_sort"] = spread(lambda: grid.cell_order(moved), args.launches, args.repeats)
    out["query_sorted"] = spread(lambda: grid.query(moved, order=order), args.launches, args.repeats)
    out["query_unsorted"] = spread(lambda: grid.query(moved, sort=False), max(1, args.launches // 4), args.repeats)
    S.accumulate_moments(source, target, dist2, index, 0.1, origin, state, partials)
    out["accumulate"] = spread(lambda: S.accumulate_moments(source, target, dist2, index, 0.1, origin, state, partials), args.launches, args.repeats)
    out["solve"] = spread(solve, args.launches, args.repeats)
    out["state_copy"] = spread(lambda: state.copy_(saved), args.launches, args.repeats)
    # the bytes I2 has to move: 12 source + 4 dist2 + 4 index + a 12-byte gather per correspondence
    out["accumulate_bytes"] = 32 * n
    out["accumulate_GBps"] = round(32 * n / (out["accumulate"]["us"] * 1e-6) / 1e9, 1)
    print(json.dumps(out), flush=True)


def part_whole(args, n, source, target):
    from splatam_amd import mesh_score as S
    found, t = wall(lambda: S.align_icp(source, target), args.runs)
    grid = S.NearestGrid(target)
    _, t_grid = wall(lambda: S.align_icp(source, target, grid=grid), args.runs)
    evaluations = len(found["history"])
    print(json.dumps({"part": "whole", "n": n, "align_icp": t, "with_grid_given": t_grid, "evaluations": evaluations, "status": found["status"],
                      "fitness": found["fitness"], "inlier_rmse": found["inlier_rmse"], "host_reads": -(-evaluations // 5),
                      "ms_per_evaluation_enqueued": round(t_grid["ms"] / (5 * -(-evaluations // 5)), 3),
                      "translation_cm_rotation_deg": S.motion_of(found["transformation"])}), flush=True)


def part_resort(args, n, source, target):
    from splatam_amd import mesh_score as S
    grid = S.NearestGrid(target)
    keep, base, out = S.ICP_RESORT_EVERY, None, {"part": "resort", "n": n}
    try:
        for every in (1, 5, 10, 10 ** 9):
            S.ICP_RESORT_EVERY = every
            found, t = wall(lambda: S.align_icp(source, target, grid=grid), args.runs)
            if base is None:
                base = found
            same = found["transformation"].tobytes() == base["transformation"].tobytes() and found["history"].tobytes() == base["history"].tobytes()
            out["once" if every > 1000 else f"every_{every}"] = dict(t, same_bits=same)
    finally:
        S.ICP_RESORT_EVERY = keep
    print(json.dumps(out), flush=True)


def part_reads(args, n, source, target):
    import torch
    from splatam_amd import mesh_score as S
    grid = S.NearestGrid(target)
    out = {"part": "reads", "n": n}
    real = torch.Tensor.cpu
    for every in (1, 5, 31):
        count = [0]

        def counting(self, *a, **k):
            count[0] += 1
            return real(self, *a, **k)
        torch.Tensor.cpu = counting
        try:
            found, t = wall(lambda: S.align_icp(source, target, grid=grid, check_every=every), args.runs)
        finally:
            torch.Tensor.cpu = real
        out[f"check_every_{every}"] = dict(t, host_reads_per_run=count[0] / (args.runs + 1), evaluations=len(found["history"]))
    print(json.dumps(out), flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--parts", default="steps,whole,resort,reads")
    parser.add_argument("--sizes", default="200000,1000000,4000000")
    parser.add_argument("--launches", type=int, default=20)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--runs", type=int, default=3)
    args = parser.parse_args()
    import torch
    assert torch.cuda.is_available(), "icp_run.py measures on the GPU"
    parts = {"steps": part_steps, "whole": part_whole, "resort": part_resort, "reads": part_reads}
    for n in (int(s) for s in args.sizes.split(",")):
        source, target = clouds(n)
        for name in args.parts.split(","):
            parts[name](args, n, source, target)
        del source, target
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
