"""Marching cubes beside marching tetrahedra (``extract(method="cubes")``; csrc/tsdf.hip, csrc/tsdf_sparse.hip), in one process, on
``scripts/mesh_run.py``'s map (workload B: 300 000 Gaussians, 1200 x 680), views and launch-repeat scheme: the dense volume at
``--voxel`` and the sparse one at ``--fine-voxel``, the two volumes of profiles/mesh.md and profiles/mesh_sparse.md.  One JSON line per
volume; in each, the two methods ALTERNATE inside every repeat, so the tetrahedra figures are the baseline of the same run:

  triangles, vertices      of either mesh
  pass_us                  microseconds per launch of the extraction pass (T2 / S3 against their cubes forms), hipEvents around
                           ``--launches`` back-to-back launches, ``--repeats`` times
  weld_us                  ``torch.unique`` over the keys plus the three stable sorts of the faces, the same way
  extract_ms               ``extract()`` as a whole, wall clock per call around ``--launches`` back-to-back calls
  clean_ms, score_ms       ``clean_mesh`` of the mesh and ``score_mesh`` of the mesh against itself, the same way

    python scripts/mesh_cubes_run.py [--parts dense,sparse] [--voxel 0.01] [--fine-voxel 0.005] [--sil-thres 0.5] [--views 4] [--launches 5] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from mesh_run import scene, timed  # noqa: E402
from mesh_sparse_run import fuse_dense, fuse_sparse, views_of  # noqa: E402

METHODS = ("tetrahedra", "cubes")


def wall_ms(fn, calls):
    """Milliseconds per call, wall clock around ``calls`` back-to-back calls with a synchronisation on either side."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return round(1e3 * (time.perf_counter() - t0) / calls, 3)


def weld(keys):
    """What ``_Surface.extract`` does between the pass and the vertices."""
    import torch
    uniq, inverse = torch.unique(keys.reshape(-1), return_inverse=True)
    faces = inverse.view(-1, 3)
    for col in (2, 1, 0):
        faces = faces[torch.sort(faces[:, col], stable=True).indices]
    return uniq, faces


def measure(args, volume, name):
    import torch
    from splatam_amd import _capi
    from splatam_amd.mesh_clean import clean_mesh
    from splatam_amd.mesh_score import score_mesh
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    sparse = name == "sparse"
    entry = {"tetrahedra": L.splat_tsdf_sparse_triangles if sparse else L.splat_tsdf_triangles,
             "cubes": L.splat_tsdf_sparse_cubes if sparse else L.splat_tsdf_cubes}
    out = {"part": name, "voxel": volume.voxel_size, "dims": list(volume.dims), "launches": args.launches}
    if sparse:
        out["slots"] = volume.slots
    meshes, keys, count = {}, {}, torch.zeros(1, dtype=torch.int64, device="cuda")
    for m in METHODS:
        meshes[m] = volume.extract(method=m)
        n = volume.last_triangle_count
        keys[m] = torch.empty(n, 3, dtype=torch.int64, device="cuda")
        entry[m](C.byref(volume.struct), 1.0, keys[m].data_ptr(), n, count.data_ptr(), stream)
        clean_mesh(meshes[m])                               # (the process's first calls warm the allocator and the libraries up: not timed)
        score_mesh(meshes[m], meshes[m], samples=args.samples)
        out[m] = {"triangles": n, "vertices": int(meshes[m].vertices.shape[0]), "pass_us": [], "weld_us": [], "extract_ms": [], "clean_ms": [], "score_ms": []}
    for _ in range(args.repeats):
        for m in METHODS:                                   # alternating: neither method has the warmer machine
            n = keys[m].shape[0]
            out[m]["pass_us"].append(round(timed(lambda: entry[m](C.byref(volume.struct), 1.0, keys[m].data_ptr(), n, count.data_ptr(), stream), args.launches), 1))
            out[m]["weld_us"].append(round(timed(lambda: weld(keys[m]), args.launches), 1))
            out[m]["extract_ms"].append(wall_ms(lambda: volume.extract(method=m), args.launches))
            out[m]["clean_ms"].append(wall_ms(lambda: clean_mesh(meshes[m]), args.launches))
            out[m]["score_ms"].append(wall_ms(lambda: score_mesh(meshes[m], meshes[m], samples=args.samples), args.launches))
    tets, cubes = out["tetrahedra"], out["cubes"]
    out["triangle_ratio"] = round(cubes["triangles"] / max(tets["triangles"], 1), 4)
    out["vertex_ratio"] = round(cubes["vertices"] / max(tets["vertices"], 1), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="dense,sparse")
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--fine-voxel", type=float, default=0.005)
    ap.add_argument("--sil-thres", type=float, default=0.5)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=200_000)
    args = ap.parse_args()
    eng, view = scene(args.views)
    views = views_of(args, eng, view)
    for part in args.parts.split(","):
        volume = fuse_dense(args, eng, views, args.voxel) if part == "dense" else fuse_sparse(args, eng, views, args.fine_voxel)[0]
        print(json.dumps(measure(args, volume, part)), flush=True)
        del volume


if __name__ == "__main__":
    main()
