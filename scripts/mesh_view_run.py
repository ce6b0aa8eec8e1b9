"""What picturing a mesh costs (csrc/meshshade.hip; ``splatam_amd.mesh_view``) next to the depth render it is built on.  One JSON line,
on ``scripts/mesh_render_run.py``'s mesh (``bench.py``'s workload-B map, 300 000 Gaussians, ``extract_mesh`` at ``--voxel`` metres) at
1200 x 680, from that script's three views (the first frame's pose, a ring pose outside the mesh's box, a pose inside it).  hipEvents
over ``--launches`` back-to-back calls after a warm-up; the parts of one view are timed in turn, ``--repeats`` rounds of all of them, so
that every part meets the same neighbours on the machine:

  depth           ``mesh_render.render_depth`` (clear, raster with a 4-byte atomic min, finish): THE YARDSTICK, on the parent commit too.
  visibility      ``splat_mesh_visibility`` alone (clear of the 8-byte plane, raster with an 8-byte atomic min).
  picture_1       ``MeshViewer.render`` at samples 1: visibility + shade.        picture_2: at samples 2 (a 2400 x 1360 key plane).
  normals         ``vertex_normals`` (clear, faces, vertices).
  compare         ``mesh_render.compare_depth`` of the view's depth plane with the second ring pose's.

Per view, once and outside every timed loop, the SHA-256 of the depth plane, the key plane, both pictures, the normals and the compare
row (``mesh_run.digest``): two builds of the library render the same when these lines agree.

Every part is reported in microseconds per call (all repeats) and as the ratio of its median to the depth render's median in the same
view, with the largest and smallest ratio over the repeats as the spread.  Pose uploads are part of a ``MeshViewer.render`` call (64
bytes, host to device), as they are for a user; ``depth`` and ``visibility`` read a pose that is on the device already.

    python scripts/mesh_view_run.py [--voxel 0.02] [--launches 50] [--repeats 5] [--mode shaded]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", default="shaded")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mesh_render_run as base
    from mesh_run import digest
    from splatam_amd import mesh_render as MR
    from splatam_amd import mesh_view as MV
    m, intr, size = base.the_mesh(args)
    W, H = size
    F, V = int(m.faces.shape[0]), int(m.vertices.shape[0])
    poses, box = base.ring(m, 8)
    views = (("first_frame", np.eye(4)), ("ring_0", poses[0]), ("inside_box", base.look_at(0.5 * (box[0] + box[1]), box[1])))
    one, two = MV.MeshViewer(m, size, intr, samples=1), MV.MeshViewer(m, size, intr, samples=2)
    plane, other = torch.empty(H, W, dtype=torch.float32, device="cuda"), torch.empty(H, W, dtype=torch.float32, device="cuda")
    cmp_row = torch.zeros(8, dtype=torch.float64, device="cuda")
    accum, normals = torch.empty(V, 3, dtype=torch.int64, device="cuda"), torch.empty(V, 3, dtype=torch.float32, device="cuda")
    out = {"faces": F, "vertices": V, "size": [W, H], "mode": args.mode, "launches": args.launches, "views": {}}
    for name, w2c in views:
        pose = MR._poses(w2c, m.vertices.device)
        MR.render_depth(m.vertices, m.faces, MR._poses(poses[1], m.vertices.device), intr, size, out=other)     # what `compare` compares with
        parts = {
            "depth": lambda: MR.render_depth(m.vertices, m.faces, pose, intr, size, out=plane),
            "visibility": lambda: MV.render_keys(m.vertices, m.faces, pose.data_ptr(), one.view, one.keys),
            "picture_1": lambda: one.render(w2c, mode=args.mode),
            "picture_2": lambda: two.render(w2c, mode=args.mode),
            "normals": lambda: MV.vertex_normals(m.vertices, m.faces, out=normals, accum=accum),
            "compare": lambda: MR.compare_depth(plane, other, cmp_row),
        }
        us = {k: [] for k in parts}
        for _ in range(args.repeats):
            for k, fn in parts.items():
                us[k].append(round(base.timed(fn, args.launches), 1))
        row = {}
        for k in parts:
            ratios = [a / b for a, b in zip(us[k], us["depth"])]
            row[k] = {"us": us[k], "over_depth": round(float(np.median(us[k])) / float(np.median(us["depth"])), 2),
                      "over_depth_spread": [round(min(ratios), 2), round(max(ratios), 2)]}
        picture = one.render(w2c, mode=args.mode)
        # once per view, outside every timed loop: two builds of the library render the same when these lines agree
        row["sha256"] = {"depth": digest([plane]), "keys": digest([one.keys]), "picture_1": digest([picture]),
                         "picture_2": digest([two.render(w2c, mode=args.mode)]), "normals": digest([normals]),
                         "compare_row": digest([cmp_row])}
        row["pixels_with_a_face"] = int((one.keys != -1).sum())
        row["distinct_colours"] = int(torch.unique(picture.reshape(-1, 3), dim=0).shape[0])
        out["views"][name] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
