"""What scoring a mesh costs (csrc/meshscore.hip; ``splatam_amd.mesh_score``).  One JSON line per part, at the protocol's size (200 000
samples against 200 000) on a mesh of ``bench.py``'s workload-B map (300 000 Gaussians, 1200 x 680; ``extract_mesh`` at ``--voxel``
metres) against a copy shifted rigidly by ``--shift`` metres:

  kernels    M0 .. M5 and the two ``torch.sort`` calls, each with hipEvents over ``--launches`` back-to-back calls, ``--repeats`` times.
             M4's account: candidates evaluated and shells walked per query (the kernel's own counters, a separate launch), its
             ALGORITHMIC bytes (16 per candidate, 12 + 8 per query) and their share of the HBM peak (6.29 TB/s measured with a float4
             copy) -- most candidate reads are served by the caches, since sorted neighbours read the same records.  The same M4
             with the queries left unsorted alongside.
  cells      building the grid and querying it (sort included) at cell sizes aimed at 1, 2, 4, 8 and 16 points per non-empty cell.
  baselines  chunked ``torch.cdist`` + ``min`` on the device over the same points; ``scipy.spatial.cKDTree`` on the host when scipy
             can be imported.
  whole      ``score_mesh`` end to end, wall clock.

    python scripts/mesh_score_run.py [--parts kernels,cells,baselines,whole] [--samples 200000] [--voxel 0.02] [--shift 0.01]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_MEASURED = 6.29e12


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


def meshes(args):
    import torch
    import mesh_run
    from splatam_amd import mesh
    eng, view = mesh_run.scene(4)
    with torch.no_grad():
        m = mesh.extract_mesh(eng, [0, 1, 2, 3], (mesh_run.W, mesh_run.H), (mesh_run.FX, mesh_run.FY, mesh_run.CX, mesh_run.CY),
                              voxel_size=args.voxel, view=view, sil_thres=0.5)
    shift = torch.tensor([args.shift, -args.shift / 2, args.shift / 3], device="cuda")
    return m, mesh.Mesh(m.vertices + shift, m.faces, m.colors)


def part_kernels(args, rec, gt):
    import numpy as np
    import torch
    from splatam_amd import _capi
    from splatam_amd import mesh_score as S
    n, L, stream = args.samples, _capi.lib(), torch.cuda.current_stream().cuda_stream
    rep = lambda fn, k=args.launches: [round(timed(fn, k), 1) for _ in range(args.repeats)]      # noqa: E731
    out = {"part": "kernels", "samples": n, "faces": int(rec.faces.shape[0]), "vertices": int(rec.vertices.shape[0])}
    out["M0_areas_us"] = rep(lambda: S.surface_prefix(rec.vertices, rec.faces)[0])
    area, prefix = S.surface_prefix(rec.vertices, rec.faces)
    out["cumsum_us"] = rep(lambda: torch.cumsum(area, 0))
    out["M1_sample_us"] = rep(lambda: S.sample_surface(rec.vertices, rec.faces, n, 0, prefix=prefix))
    queries = S.sample_surface(rec.vertices, rec.faces, n, 0, prefix=prefix)[0]
    targets = S.sample_surface(gt.vertices, gt.faces, n, 0)[0]
    grid = S.NearestGrid(targets)
    out["grid"] = {"cell": grid.cell, "dims": list(grid.dims), "cells": grid.cells,
                   "non_empty_cells": int((grid.start[1:] > grid.start[:-1]).sum().item())}
    key = torch.empty(n, dtype=torch.int32, device="cuda")
    out["M2_cell_keys_us"] = rep(lambda: L.splat_nn_cell_keys(C.byref(grid.struct), targets.data_ptr(), n, key.data_ptr(), stream))
    out["sort_us"] = rep(lambda: torch.sort(key, stable=True))
    skey, order = torch.sort(key, stable=True)
    order = order.to(torch.int32)
    records, start = torch.empty_like(grid.records), torch.empty_like(grid.start)
    out["M3_cell_starts_us"] = rep(lambda: L.splat_nn_cell_starts(C.byref(grid.struct), skey.data_ptr(), order.data_ptr(), targets.data_ptr(),
                                                                  records.data_ptr(), start.data_ptr(), stream))
    qorder = grid._sorted_keys(queries)[1]
    dist2, index = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    query = lambda o: L.splat_nn_query(C.byref(grid.struct), queries.data_ptr(), o, n, dist2.data_ptr(), index.data_ptr(), None, stream)      # noqa: E731
    out["M4_nearest_us"] = rep(lambda: query(qorder.data_ptr()))
    out["M4_nearest_unsorted_queries_us"] = rep(lambda: query(None))
    acc = grid.query(queries, account=True)[2].double()
    cand = float(acc[:, 0].mean().item())
    nbytes = n * (16 * cand + 20)
    med = float(np.median(out["M4_nearest_us"]))
    out["M4_account"] = {"candidates_per_query": round(cand, 1), "candidates_max": int(acc[:, 0].max().item()),
                         "shells_per_query": round(float(acc[:, 1].mean().item()), 2), "shells_max": int(acc[:, 1].max().item()),
                         "algorithmic_bytes": int(nbytes), "GB_per_s": round(nbytes / (med * 1e-6) / 1e9, 1),
                         "share_of_measured_peak": round(nbytes / (med * 1e-6) / HBM_MEASURED, 4),
                         "record_bytes": 16 * n, "candidate_evaluations_per_us": round(n * cand / med, 1)}
    row = torch.zeros(4, dtype=torch.float64, device="cuda")
    partials = torch.empty(3 * _capi.SPLAT_NN_REDUCE_ROWS, dtype=torch.float64, device="cuda")
    out["M5_reduce_us"] = rep(lambda: S.reduce_distances(dist2, 0.05, row, partials))
    import mesh_run
    out["sha256_reduce_row"] = mesh_run.digest([row])                   # two builds of the library reduce alike when these lines agree
    return out


def part_cells(args, rec, gt):
    import torch
    from splatam_amd import mesh_score as S
    n = args.samples
    queries, targets = S.sample_surface(rec.vertices, rec.faces, n, 0)[0], S.sample_surface(gt.vertices, gt.faces, n, 0)[0]
    box = torch.stack((targets.min(dim=0).values, targets.max(dim=0).values)).double().cpu().numpy()
    out = {"part": "cells", "samples": n, "rows": []}
    for per_cell in (1.0, 2.0, 4.0, 8.0, 16.0):
        lo, cell, dims = S.plan_grid(box[0], box[1], n, per_cell=per_cell)
        grid = S.NearestGrid(targets, cell=cell, bounds=(box[0], box[1]))
        acc = grid.query(queries, account=True)[2].double()
        filled = int((grid.start[1:] > grid.start[:-1]).sum().item())
        out["rows"].append({"aimed_points_per_cell": per_cell, "cell": cell, "cells": grid.cells, "non_empty_cells": filled,
                            "points_per_non_empty_cell": round(n / max(filled, 1), 2),
                            "candidates_per_query": round(float(acc[:, 0].mean().item()), 1), "shells_per_query": round(float(acc[:, 1].mean().item()), 2),
                            "build_us": [round(timed(lambda: S.NearestGrid(targets, cell=cell, bounds=(box[0], box[1])), 3), 1) for _ in range(args.repeats)],
                            "query_with_sort_us": [round(timed(lambda: grid.query(queries), 5), 1) for _ in range(args.repeats)]})
    return out


def part_baselines(args, rec, gt):
    import numpy as np
    import torch
    from splatam_amd import mesh_score as S
    n = args.samples
    queries, targets = S.sample_surface(rec.vertices, rec.faces, n, 0)[0], S.sample_surface(gt.vertices, gt.faces, n, 0)[0]
    grid = S.NearestGrid(targets)
    ours = grid.query(queries)[0]

    def cdist(chunk=4096):
        best = torch.empty(n, device="cuda")
        for s in range(0, n, chunk):
            best[s:s + chunk] = torch.cdist(queries[s:s + chunk], targets).min(dim=1).values
        return best
    out = {"part": "baselines", "samples": n}
    out["grid_build_and_query_us"] = [round(timed(lambda: S.NearestGrid(targets).query(queries), 3), 1) for _ in range(args.repeats)]
    out["cdist_min_us"] = [round(timed(cdist, 1), 1) for _ in range(args.repeats)]
    diff = (cdist() - ours.sqrt()).abs().max().item()
    out["cdist_largest_difference_m"] = diff
    try:
        from scipy.spatial import cKDTree
        q, t = queries.cpu().numpy(), targets.cpu().numpy()
        vals = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            d = cKDTree(t).query(q, workers=-1)[0]
            vals.append(round(1e6 * (time.perf_counter() - t0), 1))
        out["ckdtree_host_us"] = vals
        out["ckdtree_largest_difference_m"] = float(np.abs(d - np.sqrt(ours.cpu().numpy().astype(np.float64))).max())
    except ImportError:
        out["ckdtree_host_us"] = None
    return out


def part_whole(args, rec, gt):
    import torch
    from splatam_amd import mesh_score as S
    vals = []
    for _ in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score = S.score_mesh(rec, gt, samples=args.samples)
        vals.append(round(1e3 * (time.perf_counter() - t0), 2))
    return {"part": "whole", "samples": args.samples, "score_mesh_wall_ms": vals, "score": score}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernels,cells,baselines,whole")
    ap.add_argument("--samples", type=int, default=200_000)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--shift", type=float, default=0.01)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    rec, gt = meshes(args)
    for part in args.parts.split(","):
        print(json.dumps({"kernels": part_kernels, "cells": part_cells, "baselines": part_baselines, "whole": part_whole}[part](args, rec, gt)),
              flush=True)


if __name__ == "__main__":
    main()
