"""What cleaning a mesh costs on the device (csrc/meshclean.hip; ``splatam_amd.mesh_clean``) and what it removes, on ``scripts/mesh_run.py``'s
map (workload B: 300 000 Gaussians, 1200 x 680) meshed from a sparse volume at each of ``--voxels``.  One JSON line per voxel size:

  mesh      vertices, faces, components with a face, and at ``clean_mesh``'s defaults the components kept and the share of faces and of
            area removed.
  kernels   microseconds per call, hipEvents around ``--launches`` back-to-back calls, the best of ``--repeats``: C1
            (``splat_mesh_components``: init, link, flatten), C2 (``splat_mesh_component_stats``: init, vertices, faces), the filter and
            the compaction (torch, with its one host read: wall clock), and ``clean_mesh`` end to end (wall clock).  C1's achieved bytes/s
            against its algorithmic bytes (12 F + 4 V read, 4 V written).  The split of C1 into link and flatten comes from the kernel
            trace of a profiler run of this script (``--no-host --launches 5`` under ``rocprofv3 --kernel-trace --stats``).
  host      the route this replaces, on the same mesh: download, ``scipy.sparse.csgraph.connected_components``, a numpy filter and
            compaction, upload; wall clock of each step.  The two cleaned meshes are compared.

    python scripts/mesh_clean_run.py [--voxels 0.01,0.005] [--sil-thres 0.5] [--views 4] [--launches 20] [--repeats 3] [--no-host]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from mesh_run import FX, FY, CX, CY, H, W, scene, timed  # noqa: E402

INTR = (FX, FY, CX, CY)


def wall(fn, repeats):
    import torch
    best, out = float("inf"), None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return 1e3 * best, out


def host_route(mesh, min_vertices):
    """download, scipy components, numpy filter and compaction, upload: (milliseconds per step, the cleaned Mesh on the device)."""
    import numpy as np
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from splatam_amd.mesh import Mesh
    ms = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, f, c = (t.cpu().numpy() for t in mesh)
    ms["download"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    V = len(v)
    rows, cols = np.concatenate((f[:, 0], f[:, 1])), np.concatenate((f[:, 1], f[:, 2]))
    _, comp = connected_components(coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(V, V)), directed=False)
    ms["components"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    keep_f = (np.bincount(comp) >= min_vertices)[comp[f[:, 0]]]
    kept = f[keep_f]
    used = np.zeros(V, dtype=bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    out = (v[used], renumber[kept].astype(np.int32), c[used])
    ms["filter"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    up = Mesh(*(torch.from_numpy(np.ascontiguousarray(a)).to(mesh.vertices.device) for a in out))
    torch.cuda.synchronize()
    ms["upload"] = 1e3 * (time.perf_counter() - t0)
    ms["total"] = sum(ms.values())
    return ms, up


def measure(args, eng, view, voxel):
    import torch
    from splatam_amd import mesh as M
    from splatam_amd import mesh_clean as MC
    from splatam_amd.mesh_render import _keep_faces
    with torch.no_grad():
        mesh = M.extract_mesh(eng, list(range(args.views)), (W, H), INTR, voxel_size=voxel, view=view, sil_thres=args.sil_thres, sparse=True)
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    cleaned, report = MC.clean_mesh(mesh, report=True)
    out = {"voxel": voxel, "vertices": V, "faces": F, "components": report["components"], "components_kept": report["components_kept"],
           "faces_removed_share": report["faces_removed"] / max(F, 1), "area_m2": report["area_m2"],
           "area_removed_share": report["area_removed_m2"] / report["area_m2"] if report["area_m2"] > 0 else 0.0,
           "vertices_after": int(cleaned.vertices.shape[0]), "faces_after": int(cleaned.faces.shape[0])}
    labels = MC.label_components(V, mesh.faces)
    sizes = torch.bincount(labels.long(), minlength=V)
    out["largest_component_vertices"] = int(sizes.max())
    c1 = min(timed(lambda: MC.label_components(V, mesh.faces), args.launches) for _ in range(args.repeats))
    c2 = min(timed(lambda: MC.component_stats(mesh, labels), args.launches) for _ in range(args.repeats))
    stats = MC.component_stats(mesh, labels)

    def compaction():
        survive = MC.surviving_components(stats)
        idx = mesh.faces.long()
        return _keep_faces(mesh, idx, survive[labels[idx[:, 0]].long()])
    comp_ms, _ = wall(compaction, args.repeats)
    whole_ms, _ = wall(lambda: MC.clean_mesh(mesh), args.repeats)
    nbytes = 12 * F + 4 * V + 4 * V
    out.update({"c1_components_us": c1, "c2_stats_us": c2, "filter_and_compaction_wall_ms": comp_ms, "clean_mesh_wall_ms": whole_ms,
                "c1_algorithmic_bytes": nbytes, "c1_bytes_per_s": nbytes / (c1 * 1e-6)})
    if not args.no_host:
        best = None
        for _ in range(args.repeats):
            ms, host = host_route(mesh, 200)
            best = ms if best is None or ms["total"] < best["total"] else best
        out["host_route_ms"] = best
        out["host_equals_device"] = all(torch.equal(a, b) for a, b in zip(host, cleaned))
        out["device_over_host"] = whole_ms / best["total"]
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--voxels", default="0.01,0.005")
    parser.add_argument("--sil-thres", type=float, default=0.5)
    parser.add_argument("--views", type=int, default=4)
    parser.add_argument("--launches", type=int, default=20)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--no-host", action="store_true", help="skip the host route (scipy)")
    args = parser.parse_args()
    eng, view = scene(args.views)
    for voxel in (float(x) for x in args.voxels.split(",")):
        print(json.dumps(measure(args, eng, view, voxel)), flush=True)


if __name__ == "__main__":
    main()
