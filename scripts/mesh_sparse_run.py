"""What the sparse volume saves and costs (csrc/tsdf_sparse.hip; ``splatam_amd.mesh.SparseTsdfVolume``) against the dense one, in one process,
on ``scripts/mesh_run.py``'s map (workload B: 300 000 Gaussians, 1200 x 680), views and launch-repeat scheme.  One JSON line per part:

  shapes   for each brick shape the library accepts, after two-phase fusion of the views: bricks marked, allocated and STRICTLY NEEDED
           (from the dense volume: the bricks that meet the 3 x 3 x 3 dilation of ``tsdf < 0``), pool + tables bytes against the dense
           volume's, and the pool's occupancy (share of its points with weight > 0).  The default shape is the one that needs fewer bytes.
  kernels  microseconds per launch of S1 (mark) and S2 (integrate) per view against T1, S3 (triangles) against T2 and S4 (vertices)
           against T3, hipEvents around ``--launches`` back-to-back launches, ``--repeats`` times; the slot reset against T0; S2 per
           view on either brick shape; a SHA-256 of either volume's arrays after the first view into fresh ones.
  whole    ``extract_mesh`` end to end, dense and sparse, wall clock; the two meshes are compared tensor for tensor, and a SHA-256 of
           each mesh's three tensors says whether another build of the library (``SPLAT_HIP_LIB``) gives the same bits.
  fine     the same map at ``--fine-voxel`` (default 0.005): the dense volume ``plan_volume`` refuses under the default 8 GiB, the sparse
           volume's bytes and ``extract_mesh(..., sparse=True)`` wall clock.

    python scripts/mesh_sparse_run.py [--parts shapes,kernels,whole,fine] [--voxel 0.01] [--sil-thres 0.5] [--views 4] [--launches 20] [--repeats 3]
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

from mesh_run import FX, FY, CX, CY, H, W, digest, scene, timed  # noqa: E402

INTR = (FX, FY, CX, CY)


def plan(eng, voxel, sparse=False):
    from splatam_amd import mesh
    trunc = 4 * voxel
    bounds = mesh.default_bounds(eng.params['means3D'][:eng.P], eng.params['logit_opacities'][:eng.P], trunc + voxel)
    origin, dims = mesh.plan_volume(bounds, voxel, sparse=sparse)
    return origin, dims, trunc


def views_of(args, eng, view):
    """[(planes, w2c)] of the views, cloned off the view camera."""
    import torch
    out = []
    with torch.no_grad():
        for t in range(args.views):
            img = eng.render_view(view, time_idx=t, intrinsics=INTR, rgb8=False)
            assert int(img.truncated.item()) == 0
            out.append((img.out6.clone(), view.w2c.clone()))
    return out


def fuse_sparse(args, eng, views, voxel, brick=None):
    from splatam_amd import mesh
    origin, dims, trunc = plan(eng, voxel, sparse=True)
    volume = mesh.SparseTsdfVolume(origin, dims, voxel, trunc, device=eng.dev, brick=brick)
    for planes, w2c in views:
        volume.mark(planes, w2c, INTR, sil_thres=args.sil_thres)
    marked = volume.marked_count()
    volume.allocate(count=marked)
    for planes, w2c in views:
        volume.integrate(planes, w2c, INTR, sil_thres=args.sil_thres)
    return volume, marked


def fuse_dense(args, eng, views, voxel):
    from splatam_amd import mesh
    origin, dims, trunc = plan(eng, voxel)
    volume = mesh.TsdfVolume(origin, dims, voxel, trunc, eng.dev)
    for planes, w2c in views:
        volume.integrate(planes, w2c, INTR, sil_thres=args.sil_thres)
    return volume


def needed_bricks(dense, brick):
    """Bricks of shape ``brick`` that meet the 3 x 3 x 3 dilation of the dense volume's ``tsdf < 0``."""
    import torch.nn.functional as F
    near = dense.tsdf < 0
    for axis in range(3):                                   # a box dilation is separable: one index either way along each axis
        grown = near.clone()
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        grown[tuple(lo)] |= near[tuple(hi)]
        grown[tuple(hi)] |= near[tuple(lo)]
        near = grown
    bx, by, bz = brick
    nz, ny, nx = near.shape
    near = F.pad(near, (0, -nx % bx, 0, -ny % by, 0, -nz % bz))
    return int(near.view(near.shape[0] // bz, bz, near.shape[1] // by, by, near.shape[2] // bx, bx).any(5).any(3).any(1).sum().item())


def part_shapes(args, eng, view):
    import torch
    from splatam_amd import mesh
    views = views_of(args, eng, view)
    dense = fuse_dense(args, eng, views, args.voxel)
    want = dense.extract()
    out = {"part": "shapes", "voxel": args.voxel, "dims": list(dense.dims), "dense_bytes": mesh.volume_bytes(dense.dims),
           "negative_points": int((dense.tsdf < 0).sum().item()), "updated_points": int((dense.weight > 0).sum().item()), "shapes": []}
    for brick in mesh.brick_shapes():
        volume, marked = fuse_sparse(args, eng, views, args.voxel, brick)
        got = volume.extract()
        same = all(torch.equal(a, b) for a, b in zip(got, want))
        out["shapes"].append({"brick": list(brick), "bricks": volume.num_bricks, "marked": marked, "allocated": volume.slots,
                              "strictly_needed": needed_bricks(dense, brick), "bytes": volume.bytes(),
                              "pool_bytes": 20 * mesh.BRICK_POINTS * volume.slots, "tables_bytes": volume.bytes() - 20 * mesh.BRICK_POINTS * volume.slots,
                              "share_of_dense": round(volume.bytes() / mesh.volume_bytes(dense.dims), 4),
                              "occupancy": round(float((volume.arrays()["weight"] > 0).float().mean().item()), 4),
                              "mesh_equals_dense": same, "faces": int(got.faces.shape[0])})
        del volume
    return out


def part_kernels(args, eng, view):
    import numpy as np
    import torch
    from splatam_amd import _capi, mesh
    views = views_of(args, eng, view)
    dense = fuse_dense(args, eng, views, args.voxel)
    sparse, marked = fuse_sparse(args, eng, views, args.voxel)
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    rep = lambda fn, launches=args.launches: [round(timed(fn, launches), 1) for _ in range(args.repeats)]      # noqa: E731
    out = {"part": "kernels", "voxel": args.voxel, "brick": list(sparse.brick), "slots": sparse.slots, "launches": args.launches, "views": []}
    for t, (planes, w2c) in enumerate(views):
        kw = dict(sil_thres=args.sil_thres)
        out["views"].append({"time_idx": t, "T1_us": rep(lambda: dense.integrate(planes, w2c, INTR, **kw)),
                             "S1_us": rep(lambda: sparse.mark(planes, w2c, INTR, **kw)),
                             "S2_us": rep(lambda: sparse.integrate(planes, w2c, INTR, **kw))})
    # what one view updates in either volume, and S2 on the other brick shapes (the same points of the grid, another footprint per wave)
    planes, w2c = views[0]
    for volume, name in ((dense, "dense"), (sparse, "sparse")):
        if volume is dense:
            dense.reset()
        else:
            L.splat_tsdf_sparse_reset_slots(C.byref(sparse.struct), 0, sparse.slots, stream)
        volume.integrate(planes, w2c, INTR, sil_thres=args.sil_thres)
        out[f"view0_updated_points_{name}"] = int((volume.arrays()["weight"] > 0).sum().item())
        out[f"volume_sha256_after_view0_{name}"] = digest(volume.arrays().values())
    out["sparse_pool_points"] = sparse.slots * mesh.BRICK_POINTS
    out["S2_view0_us_by_shape"] = {}
    for brick in mesh.brick_shapes():
        other, _ = fuse_sparse(args, eng, views, args.voxel, brick)
        out["S2_view0_us_by_shape"]["x".join(map(str, brick))] = {
            "slots": other.slots, "us": rep(lambda: other.integrate(planes, w2c, INTR, sil_thres=args.sil_thres)),
            "us_per_view": [rep(lambda: other.integrate(p, m, INTR, sil_thres=args.sil_thres)) for p, m in views]}
        del other
    out["T0_us"] = rep(dense.reset)
    out["reset_slots_us"] = rep(lambda: L.splat_tsdf_sparse_reset_slots(C.byref(sparse.struct), 0, sparse.slots, stream))
    # (the timing loops integrated the views many times over and reset the volumes: fuse again for the surface)
    dense.reset()
    for planes, w2c in views:
        dense.integrate(planes, w2c, INTR, sil_thres=args.sil_thres)
        sparse.integrate(planes, w2c, INTR, sil_thres=args.sil_thres)
    dense.extract()
    sparse.extract()
    n, uniq = dense.last_triangle_count, dense.last_keys
    assert sparse.last_triangle_count == n and torch.equal(sparse.last_keys, uniq)
    keys = torch.empty(n, 3, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    verts, cols = torch.empty(uniq.numel(), 3, device="cuda"), torch.empty(uniq.numel(), 3, device="cuda")
    out.update({"triangles": n, "vertices": int(uniq.numel()),
                "T2_us": rep(lambda: L.splat_tsdf_triangles(C.byref(dense.struct), 1.0, keys.data_ptr(), n, count.data_ptr(), stream), 5),
                "S3_us": rep(lambda: L.splat_tsdf_sparse_triangles(C.byref(sparse.struct), 1.0, keys.data_ptr(), n, count.data_ptr(), stream), 5),
                "T3_us": rep(lambda: L.splat_tsdf_vertices(C.byref(dense.struct), uniq.data_ptr(), uniq.numel(), verts.data_ptr(), cols.data_ptr(), stream), 5),
                "S4_us": rep(lambda: L.splat_tsdf_sparse_vertices(C.byref(sparse.struct), uniq.data_ptr(), uniq.numel(), verts.data_ptr(), cols.data_ptr(), stream), 5)})
    out["medians"] = {k: float(np.median(v)) for k, v in out.items() if k.endswith("_us")}
    return out


def whole(args, eng, view, voxel, sparse):
    import torch
    from splatam_amd import mesh
    vals = []
    for n in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            m, volume = mesh.extract_mesh(eng, list(range(args.views)), (W, H), INTR, voxel_size=voxel, view=view, sil_thres=args.sil_thres,
                                          sparse=sparse, return_volume=True)
        torch.cuda.synchronize()
        vals.append(round(1e3 * (time.perf_counter() - t0), 1))
        if n + 1 < args.repeats:
            del volume
    return vals, m, volume


def part_whole(args, eng, view):
    import torch
    dense_ms, want, dense = whole(args, eng, view, args.voxel, False)
    del dense
    sparse_ms, got, volume = whole(args, eng, view, args.voxel, True)
    return {"part": "whole", "voxel": args.voxel, "views": args.views, "extract_mesh_dense_wall_ms": dense_ms, "extract_mesh_sparse_wall_ms": sparse_ms,
            "vertices": int(got.vertices.shape[0]), "faces": int(got.faces.shape[0]), "sparse_bytes": volume.bytes(),
            "mesh_equals_dense": all(torch.equal(a, b) for a, b in zip(got, want)), "mesh_sha256_dense": digest(want), "mesh_sha256_sparse": digest(got)}


def part_fine(args, eng, view):
    from splatam_amd import mesh
    origin, dims, trunc = plan(eng, args.fine_voxel, sparse=True)
    try:
        plan(eng, args.fine_voxel)
        refusal = None
    except ValueError as e:
        refusal = str(e)
    ms, m, volume = whole(args, eng, view, args.fine_voxel, True)
    return {"part": "fine", "voxel": args.fine_voxel, "dims": list(dims), "dense_bytes": mesh.volume_bytes(dims), "dense_refusal": refusal,
            "brick": list(volume.brick), "bricks": volume.num_bricks, "allocated": volume.slots, "sparse_bytes": volume.bytes(),
            "pool_bytes": 20 * mesh.BRICK_POINTS * volume.slots, "occupancy": round(float((volume.arrays()["weight"] > 0).float().mean().item()), 4),
            "extract_mesh_sparse_wall_ms": ms, "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="shapes,kernels,whole,fine")
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--fine-voxel", type=float, default=0.005)
    ap.add_argument("--sil-thres", type=float, default=0.5, help="0.5: 93 %% of this synthetic map's pixels pass, as nearly all of a real map's do at 0.99")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    eng, view = scene(args.views)
    for part in args.parts.split(","):
        print(json.dumps({"shapes": part_shapes, "kernels": part_kernels, "whole": part_whole, "fine": part_fine}[part](args, eng, view)), flush=True)


if __name__ == "__main__":
    main()
