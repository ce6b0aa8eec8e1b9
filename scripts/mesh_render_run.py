"""What rendering a mesh costs (csrc/meshrender.hip; ``splatam_amd.mesh_render``).  One JSON line per part, on a mesh of ``bench.py``'s
workload-B map (300 000 Gaussians, 1200 x 680; ``extract_mesh`` at ``--voxel`` metres), hipEvents over ``--launches`` back-to-back calls
after a warm-up, ``--repeats`` times:

  render     R (``splat_mesh_depth``: clear, raster, finish) at 1200 x 680 from the first frame's pose and from a pose inside the mesh's
             box, at the library's threshold between the two triangle paths and at a quarter and four times it: time per render, how
             many faces take either path and how many pixel tests each makes, the ALGORITHMIC bytes (faces, the vertices they name, one
             plane written by the clear, one read and written by the finish, 4 bytes read per pixel test, 4 more per stored hit counted
             as tests: an upper bound) and their share of the HBM peak (6.29 TB/s measured with a float4 copy); the clear and the finish
             alone; the same render with a load in front of the atomic min that filters the hits and with a plain store in its place
             (``splat_debug_option(6, .)``), which is what the z-buffer's atomic costs.  The thresholds go through
             ``splat_debug_option(5, .)``.  Per view the SHA-256 of the product's plane (``mesh_run.digest``), taken once and outside
             every timed loop: two builds of the library render the same when these lines agree.
  seen       S (``splat_mesh_seen``) on the mesh's vertices x ``--poses`` ring poses, in chunks of ``--chunk`` views, without and with
             depth planes: vertex-views per second; the torch expression of the same predicate (batched matmul and masks) alongside,
             and whether both count the same.
  depth_l1   ``depth_l1`` end to end for ``--views`` views, wall clock.

    python scripts/mesh_render_run.py [--parts render,seen,depth_l1] [--voxel 0.02] [--poses 2000] [--chunk 100] [--views 100] [--splits 4,16,64]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_MEASURED = 6.29e12
SPLIT = 16


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


def the_mesh(args):
    import torch
    import mesh_run
    from splatam_amd import mesh
    eng, view = mesh_run.scene(4)
    with torch.no_grad():
        m = mesh.extract_mesh(eng, [0, 1, 2, 3], (mesh_run.W, mesh_run.H), (mesh_run.FX, mesh_run.FY, mesh_run.CX, mesh_run.CY),
                              voxel_size=args.voxel, view=view, sil_thres=0.5)
    return m, (mesh_run.FX, mesh_run.FY, mesh_run.CX, mesh_run.CY), (mesh_run.W, mesh_run.H)


def look_at(origin, target, up=(0.0, -1.0, 0.0)):
    import numpy as np
    from splatam_amd.mesh_render import _look_at
    return _look_at(np.asarray(origin, dtype=np.float64), np.asarray(target, dtype=np.float64), np.asarray(up, dtype=np.float64))


def ring(m, n):
    """``n`` poses on a ring about the mesh's box, looking at its centre (the map's frame: y down, z forward)."""
    import numpy as np
    import torch
    box = torch.stack((m.vertices.min(dim=0).values, m.vertices.max(dim=0).values)).double().cpu().numpy()
    centre, radius = 0.5 * (box[0] + box[1]), 0.75 * float(np.linalg.norm(box[1] - box[0]))
    out = []
    for k in range(n):
        a = 2 * math.pi * k / n
        out.append(look_at(centre + radius * np.array([math.sin(a), 0.1 * math.sin(3 * a), -math.cos(a)]), centre))
    return np.stack(out), box


def path_account(m, w2c, intr, size, near, split):
    """Faces and pixel tests per path, by the torch expression of the header's box rule (float32; the counts can differ from the
    kernel's by the few faces whose box changes size in the last bit).  Faces with a vertex at z <= near are counted on their own:
    the wave walks the box of their near-clipped part, which this account does not restate, so their tests are not in the sums."""
    import torch
    fx, fy, cx, cy = intr
    W, H = size
    M = torch.as_tensor(w2c, dtype=torch.float32, device="cuda").reshape(4, 4)
    pc = m.vertices @ M[:3, :3].T + M[:3, 3]
    p = pc[m.faces.long()]                                            # [F, 3, 3]
    z = p[..., 2]
    nothing = (z < near).all(dim=1)
    crossing = ~(z > near).all(dim=1) & ~nothing
    u, v = fx * p[..., 0] / z + cx, fy * p[..., 1] / z + cy
    i0, i1 = torch.ceil(u.min(dim=1).values - 0.5).clamp(0, W - 1), torch.floor(u.max(dim=1).values + 0.5).clamp(0, W - 1)
    j0, j1 = torch.ceil(v.min(dim=1).values - 0.5).clamp(0, H - 1), torch.floor(v.max(dim=1).values + 0.5).clamp(0, H - 1)
    outside = (u.max(dim=1).values + 0.5 < 0) | (u.min(dim=1).values - 0.5 > W - 1) | (v.max(dim=1).values + 0.5 < 0) | (v.min(dim=1).values - 0.5 > H - 1)
    area = ((i1 - i0 + 1).clamp(min=0) * (j1 - j0 + 1).clamp(min=0)).double()
    live = ~nothing & ~crossing & ~outside & (area > 0)
    small, large = live & (area <= split), live & (area > split)
    return {"faces_small": int(small.sum()), "faces_large": int(large.sum()), "faces_crossing_near": int(crossing.sum()),
            "faces_nothing": int((~live & ~crossing).sum()),
            "tests_small": int(area[small].sum()), "tests_large": int(area[large].sum()),
            "largest_box": int(area[live].max()) if live.any() else 0}


def part_render(args, m, intr, size):
    import mesh_run
    import numpy as np
    import torch
    from splatam_amd import mesh_render as MR
    W, H = size
    F, V = int(m.faces.shape[0]), int(m.vertices.shape[0])
    rep = lambda fn: [round(timed(fn, args.launches), 1) for _ in range(args.repeats)]      # noqa: E731
    out = {"part": "render", "faces": F, "vertices": V, "size": [W, H], "views": {}}
    from splatam_amd import _capi
    L = _capi.lib()
    poses, box = ring(m, 8)
    inside = look_at(0.5 * (box[0] + box[1]), box[1])
    plane = torch.empty(H, W, dtype=torch.float32, device="cuda")
    empty_v, empty_f = m.vertices[:0].contiguous(), m.faces[:0].contiguous()
    eye = MR._poses(np.eye(4), m.vertices.device)                       # (on the device, as every timed call's pose: nothing is uploaded)
    out["clear_and_finish_us"] = rep(lambda: MR.render_depth(empty_v, empty_f, eye, intr, size, out=plane))
    try:
        for name, w2c in (("first_frame", np.eye(4)), ("ring_0", poses[0]), ("inside_box", inside)):
            dev_pose = MR._poses(w2c, m.vertices.device)
            row = {}
            for split in args.splits:
                L.splat_debug_option(5, split)
                acct = path_account(m, w2c, intr, size, MR.NEAR, split)
                us = rep(lambda: MR.render_depth(m.vertices, m.faces, dev_pose, intr, size, out=plane))
                tests = acct["tests_small"] + acct["tests_large"]
                nbytes = 12 * F + 12 * V + 3 * 4 * W * H + 8 * tests
                med = float(np.median(us))
                row[f"split_{split}"] = dict(acct, us=us, algorithmic_bytes=int(nbytes), GB_per_s=round(nbytes / (med * 1e-6) / 1e9, 1),
                                             share_of_measured_peak=round(nbytes / (med * 1e-6) / HBM_MEASURED, 4),
                                             pixel_tests_per_us=round(tests / med, 1))
            L.splat_debug_option(5, 0)
            row["holes"] = int((plane == 0).sum())
            # what the integer atomic min costs: the product (every hit to the atomic), a load in front that filters the hits, a plain store
            for bits, label in ((0, "product"), (1, "load_filters_the_atomic"), (2, "plain_store_no_atomic")):
                L.splat_debug_option(6, bits)
                row[f"zbuffer_{label}_us"] = rep(lambda: MR.render_depth(m.vertices, m.faces, dev_pose, intr, size, out=plane))
            L.splat_debug_option(6, 0)
            row["hits"] = hit_account(m, dev_pose, intr, size, plane)
            row["sha256_depth"] = mesh_run.digest([plane])              # (the product's plane; outside every timed loop)
            out["views"][name] = row
    finally:
        L.splat_debug_option(5, 0)
        L.splat_debug_option(6, 0)
    return out


def hit_account(m, dev_pose, intr, size, plane):
    """Pixels that hold a depth after a render: the least number of atomics any order of the faces needs."""
    from splatam_amd import mesh_render as MR
    MR.render_depth(m.vertices, m.faces, dev_pose, intr, size, out=plane)
    return {"pixels_with_depth": int((plane > 0).sum())}


def torch_seen(vertices, poses, intr, size, edge, depth, eps, chunk=16):
    """The seen predicate as torch expressions: [V] int32 counts.  Batched matmul, masks, a gather for the planes."""
    import torch
    fx, fy, cx, cy = intr
    W, H = size
    count = torch.zeros(vertices.shape[0], dtype=torch.int32, device=vertices.device)
    for s in range(0, poses.shape[0], chunk):
        M = poses[s:s + chunk].reshape(-1, 4, 4)
        pc = torch.einsum("kij,vj->kvi", M[:, :3, :3], vertices) + M[:, None, :3, 3]
        z = pc[..., 2]
        i, j = torch.floor(fx * pc[..., 0] / z + cx + 0.5), torch.floor(fy * pc[..., 1] / z + cy + 0.5)
        ok = (z > 0) & (i >= edge) & (i <= W - 1 - edge) & (j >= edge) & (j <= H - 1 - edge)
        if depth is not None:
            o = (j.clamp(0, H - 1) * W + i.clamp(0, W - 1)).long()
            d = torch.gather(depth[s:s + chunk].reshape(M.shape[0], -1), 1, torch.where(ok, o, torch.zeros_like(o)))
            ok &= (d > 0) & (z <= d + eps)
        count += ok.sum(dim=0).to(torch.int32)
    return count


def part_seen(args, m, intr, size):
    import numpy as np
    import torch
    from splatam_amd import mesh_render as MR
    W, H = size
    V = int(m.vertices.shape[0])
    poses_np, _ = ring(m, args.poses)
    poses = MR._poses(poses_np, m.vertices.device)
    k = min(args.chunk, args.poses)
    planes = torch.empty(k, H, W, dtype=torch.float32, device="cuda")
    for i in range(k):
        MR.render_depth(m.vertices, m.faces, poses[i], intr, size, out=planes[i])
    seen = torch.zeros(V, dtype=torch.int32, device="cuda")
    rep = lambda fn, n=3: [round(timed(fn, n), 1) for _ in range(args.repeats)]      # noqa: E731
    out = {"part": "seen", "vertices": V, "poses": args.poses, "chunk": k}
    all_us = rep(lambda: MR.seen_counts(m.vertices, poses, intr, size, out=seen))
    out["frusta_all_poses_us"] = all_us
    out["frusta_vertex_views_per_s"] = round(V * args.poses / (float(np.median(all_us)) * 1e-6), 0)
    chunk_us = rep(lambda: MR.seen_counts(m.vertices, poses[:k], intr, size, depth=planes, eps=0.03, out=seen), 10)
    out["planes_one_chunk_us"] = chunk_us
    out["planes_vertex_views_per_s"] = round(V * k / (float(np.median(chunk_us)) * 1e-6), 0)
    t_all = rep(lambda: torch_seen(m.vertices, poses, intr, size, 0, None, 0.0), 1)
    out["torch_frusta_all_poses_us"] = t_all
    t_chunk = rep(lambda: torch_seen(m.vertices, poses[:k], intr, size, 0, planes, 0.03), 3)
    out["torch_planes_one_chunk_us"] = t_chunk
    out["torch_over_kernel"] = {"frusta": round(float(np.median(t_all)) / float(np.median(all_us)), 1),
                                "planes": round(float(np.median(t_chunk)) / float(np.median(chunk_us)), 1)}
    ours = MR.seen_counts(m.vertices, poses[:k], intr, size, depth=planes, eps=0.03)
    theirs = torch_seen(m.vertices, poses[:k], intr, size, 0, planes, 0.03)
    out["vertices_counted_differently_by_torch"] = int((ours != theirs).sum())
    out["seen_by_some_view_of_the_chunk"] = int((ours > 0).sum())
    return out


def part_depth_l1(args, m, intr, size):
    import torch
    from splatam_amd import mesh as M
    from splatam_amd import mesh_render as MR
    poses_np, _ = ring(m, args.views)
    shifted = M.Mesh(m.vertices + torch.tensor([0.01, -0.005, 0.0033], device="cuda"), m.faces, m.colors)
    vals = []
    for _ in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score = MR.depth_l1(shifted, m, poses_np, intr, size)
        vals.append(round(1e3 * (time.perf_counter() - t0), 2))
    return {"part": "depth_l1", "views": args.views, "faces": int(m.faces.shape[0]), "depth_l1_wall_ms": vals, "score": score}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="render,seen,depth_l1")
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--splits", type=lambda t: [int(x) for x in t.split(",")], default=[SPLIT // 4, SPLIT, SPLIT * 4],
                    help="thresholds between the two triangle paths to time (default: the library's, a quarter of it and four times it)")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    m, intr, size = the_mesh(args)
    for part in args.parts.split(","):
        print(json.dumps({"render": part_render, "seen": part_seen, "depth_l1": part_depth_l1}[part](args, m, intr, size)), flush=True)


if __name__ == "__main__":
    main()
