"""What simplifying a mesh costs on the device (csrc/meshsimplify.hip; ``splatam_amd.mesh_simplify``) and what it gives, on
``scripts/mesh_run.py``'s map (workload B: 300 000 Gaussians, 1200 x 680) meshed from a sparse volume at ``--voxel``, at a cell of each of
``--cells`` voxels.  First a line that names the box, then one JSON line per cell size and placement:

  mesh      vertices and faces before and after, the shares kept, occupied cells, cells by rank, fallbacks, ``rms_plane_distance_m``.
  steps     microseconds per call, hipEvents around ``--launches`` back-to-back calls after a warm-up call, the best of ``--repeats``: S0
            keys, the cluster ids (torch: a stable sort, a flag, a prefix sum, a scatter), S1 vertex sums, S2 quadrics, S3 placement, S4
            faces, the removal of repeated triples (torch: two stable sorts), each into buffers made beforehand; the compaction with its
            one host read and ``simplify_mesh`` end to end (wall clock around a synchronise).  S2's achieved bytes/s against its
            algorithmic bytes (12 F of faces, 12 V of vertices and 4 V of cluster ids read once, 80 bytes of sums per occupied cell).
  score     ``score_mesh(simplified, original)``: how far the simplified surface is from the one it replaces.
  host      the route this replaces, on the same mesh: download, the numpy restatement (tests/meshsimplify_ref.py), upload; wall clock
            of each step.  The two meshes are compared (faces exactly, vertices to 1e-6 cell: another eigensolver).

    python scripts/mesh_simplify_run.py [--voxel 0.01] [--cells 2,3,4] [--sil-thres 0.5] [--views 4] [--launches 20] [--repeats 3] [--no-host]
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mesh_run import FX, FY, CX, CY, H, W, scene, timed  # noqa: E402

INTR = (FX, FY, CX, CY)


def best(fn, launches, repeats):
    fn()                                                                # warm: code objects, the allocator's blocks
    return min(timed(fn, launches) for _ in range(repeats))


def wall(fn, repeats):
    import torch
    fn()
    least, out = float("inf"), None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        least = min(least, time.perf_counter() - t0)
    return 1e3 * least, out


def host_route(mesh, cell, placement):
    """download, the numpy restatement, upload: (milliseconds per step, the simplified Mesh on the device)."""
    import numpy as np
    import torch
    import meshsimplify_ref as Q
    from splatam_amd.mesh import Mesh
    ms = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, f, c = (t.cpu().numpy() for t in mesh)
    ms["download"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    out = Q.simplify(v, f, c, cell, placement)[:3]
    ms["numpy"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    up = Mesh(*(torch.from_numpy(np.ascontiguousarray(a)).to(mesh.vertices.device) for a in out))
    torch.cuda.synchronize()
    ms["upload"] = 1e3 * (time.perf_counter() - t0)
    ms["total"] = sum(ms.values())
    return ms, up


def measure(args, mesh, cell, placement):
    import torch
    from splatam_amd import _capi
    from splatam_amd import mesh_simplify as MS
    from splatam_amd.mesh import Mesh
    from splatam_amd.mesh_render import _keep_faces
    from splatam_amd.mesh_score import score_mesh
    v, f, c = mesh
    V, F, dev = int(v.shape[0]), int(f.shape[0]), v.device
    out_mesh, report = MS.simplify_mesh(mesh, cell, placement=placement, report=True)
    out = {"cell": cell, "cell_voxels": round(cell / args.voxel, 3), "placement": placement, **report,
           "vertices_kept_share": report["vertices_kept"] / max(V, 1), "faces_kept_share": report["faces_kept"] / max(F, 1)}
    L, s = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    check = _capi.check
    keys = MS.cell_keys(v, cell)
    cluster = MS.cluster_ids(keys)
    acc = MS.cluster_sums(mesh, cell, cluster, quadrics=placement == "quadric")
    placed = MS.place_clusters(acc, cell, placement, colors=True)
    triples = MS.cluster_faces(f, cluster)
    keep = triples[:, 0] >= 0
    count, sums, refused = torch.zeros_like(acc["count"]), torch.zeros_like(acc["sums"]), torch.zeros_like(acc["refused"])
    p = lambda t: t.data_ptr()          # noqa: E731
    steps = {
        "s0_keys_us": lambda: check(L.splat_mesh_simplify_keys(p(v), V, cell, p(keys), s), "keys"),
        "cluster_ids_us": lambda: MS.cluster_ids(keys),
        "s1_vertices_us": lambda: check(L.splat_mesh_simplify_vertices(p(v), p(c), V, p(cluster), cell, p(count), p(sums), s), "vertices"),
        "s3_place_us": lambda: check(L.splat_mesh_simplify_place(p(acc["count"]), p(acc["sums"]), p(acc["cell_keys"]), V, cell,
                                                                 MS.PLACEMENTS[placement], p(placed["positions"]), p(placed["colors"]), p(placed["rank"]),
                                                                 p(placed["fallback"]), p(placed["value"]), s), "place"),
        "s4_faces_us": lambda: check(L.splat_mesh_simplify_faces(p(f), F, V, p(cluster), p(triples), s), "faces"),
        "dedupe_us": lambda: MS.first_of_each_triple(triples, keep),
    }
    if placement == "quadric":
        steps["s2_quadrics_us"] = lambda: check(L.splat_mesh_simplify_quadrics(p(v), V, p(f), F, p(cluster), cell, p(sums), p(refused), s), "quadrics")
    for name, fn in steps.items():
        out[name] = best(fn, args.launches, args.repeats)
    if placement == "quadric":
        nbytes = 12 * F + 16 * V + 80 * report["cells"]
        out.update({"s2_algorithmic_bytes": nbytes, "s2_bytes_per_s": nbytes / (out["s2_quadrics_us"] * 1e-6)})
    kept = MS.first_of_each_triple(triples, keep)
    faces_of = Mesh(placed["positions"], triples, placed["colors"])
    out["compaction_wall_ms"], _ = wall(lambda: _keep_faces(faces_of, MS._face_indices(triples, V), kept), args.repeats)
    out["simplify_mesh_wall_ms"], _ = wall(lambda: MS.simplify_mesh(mesh, cell, placement=placement), args.repeats)
    score = score_mesh(out_mesh, mesh, samples=args.samples, device=dev)
    out["score_against_original"] = {k: score[k] for k in ("accuracy_cm", "completion_cm", "completion_ratio") if k in score}
    if not args.no_host:
        ms, host = host_route(mesh, cell, placement)
        out["host_route_ms"] = ms
        same_faces = host.faces.shape == out_mesh.faces.shape and bool(torch.equal(host.faces, out_mesh.faces))
        out["host_faces_equal_device"] = same_faces
        if host.vertices.shape == out_mesh.vertices.shape:
            out["host_vertices_max_difference_cells"] = float((host.vertices.double() - out_mesh.vertices.double()).abs().max()) / cell
        out["device_over_host"] = out["simplify_mesh_wall_ms"] / ms["total"]
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--voxel", type=float, default=0.01)
    parser.add_argument("--cells", default="2,3,4", help="cell sizes, in voxels")
    parser.add_argument("--sil-thres", type=float, default=0.5)
    parser.add_argument("--views", type=int, default=4)
    parser.add_argument("--launches", type=int, default=20)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--samples", type=int, default=200_000)
    parser.add_argument("--no-host", action="store_true", help="skip the host route (numpy)")
    args = parser.parse_args()
    import torch
    from splatam_amd import mesh as M
    eng, view = scene(args.views)
    with torch.no_grad():
        mesh = M.extract_mesh(eng, list(range(args.views)), (W, H), INTR, voxel_size=args.voxel, view=view, sil_thres=args.sil_thres, sparse=True)
    print(json.dumps({"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "voxel": args.voxel,
                      "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0])}), flush=True)
    for cells in (float(x) for x in args.cells.split(",")):
        for placement in ("quadric", "mean"):
            print(json.dumps(measure(args, mesh, cells * args.voxel, placement)), flush=True)


if __name__ == "__main__":
    main()
