"""What a mesh of the map costs (csrc/tsdf.hip; ``splatam_amd.mesh``).  One JSON line per part, on ``bench.py``'s workload-B map
(300 000 Gaussians, 1200 x 680) in a volume of ``--voxel`` metres (default 0.01) over the map's default bounds:

  integrate  T1 per view: hipEvents around ``--launches`` back-to-back ``TsdfVolume.integrate`` calls on the planes of one rendered view,
             for ``--views`` poses on a small arc, ``--repeats`` times each; microseconds per launch, the grid points a launch updates,
             its ALGORITHMIC bytes (40 per updated grid point: five arrays read and written; plus the five planes once) and their share
             of the HBM peak (6.29 TB/s measured with a float4 copy, 8.0 TB/s on the data sheet).  T0 (reset) alongside, for scale: it
             writes every array once.
  extract    T2 (one pass at a capacity that fits, and the count-only pass at capacity 0), ``torch.unique`` + the three sorts, and T3,
             each with hipEvents; then ``extract()`` as a whole with its host read.
             ``--sil-thres`` defaults to 0.5 here: the synthetic map is thin (10 % of its pixels have a silhouette above 0.99, 93 % above
             0.5), a map SLAM has built is opaque nearly everywhere, and the share of the grid a view updates is what T1's traffic scales with.
  whole      ``extract_mesh`` over the views end to end (render + integrate per view, one read, extract), wall clock.

``integrate`` also gives a SHA-256 of the volume's five arrays after the first view into a fresh volume, ``whole`` one of the mesh's three
tensors: run against two builds of the library (``SPLAT_HIP_LIB``), the lines say whether they compute the same bits.  The volume's
digest copies one array at a time to the host, once and outside every timed loop: about 0.5 GB of host memory at the default 1 cm.

    python scripts/mesh_run.py [--parts integrate,extract,whole] [--voxel 0.01] [--sil-thres 0.5] [--views 4] [--launches 20] [--repeats 3]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, W, H, FX, FY, CX, CY = 300_000, 1200, 680, 600.0, 600.0, 599.5, 339.5         # bench.py WORKLOADS["B"]
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def timed(fn, launches):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / launches          # microseconds per call


def digest(tensors):
    """SHA-256 over the bytes of ``tensors``, in order: two builds of the library give the same volume or mesh when their lines agree."""
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def scene(views):
    import numpy as np
    import torch
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables = slam.synthetic_params(N, W, H, FX, FY, CX, CY, num_frames=views, seed=0, device="cuda")
    with torch.no_grad():
        for t in range(1, views):                   # keyframe views on a small arc, as bench.py places them
            ang, tr = math.radians(0.3 * t), 0.02 * t
            params['cam_unnorm_rots'][..., t] = torch.tensor([[math.cos(ang / 2), 0.0, math.sin(ang / 2), 0.0]], device="cuda")
            params['cam_trans'][..., t] = torch.tensor([[tr, -tr / 2, tr / 2]], device="cuda")
        cam = slam.setup_camera(W, H, [[FX, 0, CX], [0, FY, CY], [0, 0, 1]], np.eye(4, dtype=np.float32), device="cuda")
        eng = FusedEngine(params, cam, variables=variables)
        view = eng.view_camera(W, H)
        for _ in range(3):
            eng.render_view(view, time_idx=0, intrinsics=(FX, FY, CX, CY), rgb8=False)
            if not view.check_overflow():
                break
    return eng, view


def volume_for(eng, voxel):
    from splatam_amd import mesh
    trunc = 4 * voxel
    bounds = mesh.default_bounds(eng.params['means3D'][:eng.P], eng.params['logit_opacities'][:eng.P], trunc + voxel)
    origin, dims = mesh.plan_volume(bounds, voxel)
    return mesh.TsdfVolume(origin, dims, voxel, trunc, eng.dev)


def part_integrate(args, eng, view):
    import numpy as np
    import torch
    volume = volume_for(eng, args.voxel)
    points = volume.dims[0] * volume.dims[1] * volume.dims[2]
    intr = (FX, FY, CX, CY)
    out = {"part": "integrate", "voxel": args.voxel, "sil_thres": args.sil_thres, "dims": list(volume.dims), "volume_bytes": 20 * points, "size": [W, H], "launches": args.launches,
           "views": []}
    reset_us = [timed(volume.reset, args.launches) for _ in range(args.repeats)]
    out["reset"] = {"us_per_launch": [round(v, 1) for v in reset_us], "bytes": 20 * points,
                    "share_of_measured_peak": round(20 * points / (float(np.median(reset_us)) * 1e-6) / HBM_MEASURED, 3)}
    with torch.no_grad():
        for t in range(args.views):
            img = eng.render_view(view, time_idx=t, intrinsics=intr, rgb8=False)
            assert int(img.truncated.item()) == 0
            planes, w2c = img.out6.clone(), view.w2c.clone()
            volume.reset()
            volume.integrate(planes, w2c, intr, sil_thres=args.sil_thres)
            updated = int((volume.weight > 0).sum().item())
            if t == 0:
                out["volume_sha256_after_view0"] = digest(volume.arrays().values())
            nbytes = 40 * updated + 20 * W * H
            vals = [timed(lambda: volume.integrate(planes, w2c, intr, sil_thres=args.sil_thres), args.launches) for _ in range(args.repeats)]
            med = float(np.median(vals))
            out["views"].append({"time_idx": t, "us_per_launch": [round(v, 1) for v in vals], "median_us": round(med, 1), "updated_points": updated,
                                 "updated_share": round(updated / points, 4), "algorithmic_bytes": nbytes,
                                 "GB_per_s": round(nbytes / (med * 1e-6) / 1e9, 1),
                                 "share_of_measured_peak": round(nbytes / (med * 1e-6) / HBM_MEASURED, 3),
                                 "share_of_spec_peak": round(nbytes / (med * 1e-6) / HBM_SPEC, 3)})
    return out


def part_extract(args, eng, view):
    import ctypes as C
    import numpy as np
    import torch
    from splatam_amd import _capi
    volume = volume_for(eng, args.voxel)
    intr = (FX, FY, CX, CY)
    with torch.no_grad():
        for t in range(args.views):
            volume.integrate_view(eng, view, time_idx=t, intrinsics=intr, sil_thres=args.sil_thres)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = volume.extract()
    torch.cuda.synchronize()
    whole_ms = 1e3 * (time.perf_counter() - t0)
    n = volume.last_triangle_count
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    keys = torch.empty(n, 3, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    t2 = [timed(lambda: L.splat_tsdf_triangles(C.byref(volume.struct), 1.0, keys.data_ptr(), n, count.data_ptr(), stream), 5) for _ in range(args.repeats)]
    t2_count = [timed(lambda: L.splat_tsdf_triangles(C.byref(volume.struct), 1.0, None, 0, count.data_ptr(), stream), 5) for _ in range(args.repeats)]
    uniq = volume.last_keys
    verts, cols = torch.empty(uniq.numel(), 3, device="cuda"), torch.empty(uniq.numel(), 3, device="cuda")
    t3 = [timed(lambda: L.splat_tsdf_vertices(C.byref(volume.struct), uniq.data_ptr(), uniq.numel(), verts.data_ptr(), cols.data_ptr(), stream), 5)
          for _ in range(args.repeats)]

    def weld():
        u, inv = torch.unique(keys.reshape(-1), return_inverse=True)
        f = inv.view(n, 3)
        for col in (2, 1, 0):
            f = f[torch.sort(f[:, col], stable=True).indices]
    welds = [timed(weld, 2) for _ in range(args.repeats)]
    points = volume.dims[0] * volume.dims[1] * volume.dims[2]
    return {"part": "extract", "voxel": args.voxel, "dims": list(volume.dims), "triangles": n, "vertices": int(mesh.vertices.shape[0]),
            "T2_us": [round(v, 1) for v in t2], "T2_count_only_us": [round(v, 1) for v in t2_count],
            "T2_GB_per_s_of_4_bytes_per_point": round(4 * points / (float(np.median(t2)) * 1e-6) / 1e9, 1),
            "unique_and_sorts_us": [round(v, 1) for v in welds], "T3_us": [round(v, 1) for v in t3], "extract_wall_ms": round(whole_ms, 2)}


def part_whole(args, eng, view):
    import torch
    from splatam_amd import mesh
    vals = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            m = mesh.extract_mesh(eng, list(range(args.views)), (W, H), (FX, FY, CX, CY), voxel_size=args.voxel, view=view, sil_thres=args.sil_thres)
        torch.cuda.synchronize()
        vals.append(1e3 * (time.perf_counter() - t0))
    return {"part": "whole", "voxel": args.voxel, "views": args.views, "extract_mesh_wall_ms": [round(v, 1) for v in vals],
            "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0]), "mesh_sha256": digest(m)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="integrate,extract,whole")
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--sil-thres", type=float, default=0.5, help="0.5: 93 %% of this synthetic map's pixels pass, as nearly all of a real map's do at 0.99")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    eng, view = scene(args.views)
    for part in args.parts.split(","):
        print(json.dumps({"integrate": part_integrate, "extract": part_extract, "whole": part_whole}[part](args, eng, view)), flush=True)


if __name__ == "__main__":
    main()
