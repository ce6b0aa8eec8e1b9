"""Depth images of triangle meshes, and what the NICE-SLAM mesh protocol builds on them: culling a mesh to what a run saw, and depth L1
between two meshes rendered at the same virtual views.

Everything runs on the device (csrc/meshrender.hip, arithmetic in csrc/meshrender_math.h): a z-buffer rasteriser (``render_depth``:
homogeneous edge functions in camera space, no near-plane clipping, an integer atomic min on the floats' bits, the same bits on every
run), a per-vertex visibility count over many views (``seen_counts``: frusta alone, or against depth planes) and the sums of a depth
comparison (``compare_depth``).  On top of them, with torch for the bookkeeping:

``cull_mesh``    removes the faces whose vertices no view of the run saw -- frusta alone, or occlusion-aware against renders of the mesh
                 itself (``occlusion="self"``) or against the frames' own depth planes.
``depth_l1``     the protocol's fourth figure: the mean over virtual views of the mean absolute depth difference, holes counting as 0.
``sample_views`` virtual views inside the ground truth's bounding box from which the ground truth shows no hole.

The camera convention is ``splat_tsdf_integrate``'s: ``w2c`` is row-major world-to-camera, pixel (i, j) looks along
((i - cx) / fx, (j - cy) / fy, 1).  ``intrinsics`` is (fx, fy, cx, cy) or a 3 x 3 matrix; ``size`` is (width, height).

What is NOT the protocol's: its script is not part of this project, so its constants are recalled, not read -- ``eps`` of the occlusion
test, the shrink of the bounding box and the up vector of the virtual views are parameters with documented defaults, and its random
stream is not reproduced.  Figures produced here are comparable with each other, and with published tables only as far as those
parameters match.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._mesh_common import _device, _loaded, _mesh_arrays, _on_device, _pose_tensor, _ptr, _stream, _tensor, _transform  # noqa: F401
from .mesh import Mesh

NEAR = 0.01


def parse_size(text):
    """(width, height) of ``"WxH"``."""
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.strip().isdigit() for p in parts) or int(parts[0]) <= 0 or int(parts[1]) <= 0:
        raise ValueError(f"a size is WIDTHxHEIGHT in pixels (got {text!r})")
    return int(parts[0]), int(parts[1])


def _intrinsics(intrinsics):
    k = np.asarray(intrinsics.detach().cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics, dtype=np.float64)
    if k.shape == (4,):
        fx, fy, cx, cy = k
    elif k.ndim == 2 and k.shape[0] >= 3 and k.shape[1] >= 3:
        fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    else:
        raise ValueError("intrinsics are (fx, fy, cx, cy) or a 3 x 3 matrix")
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx != 0 and fy != 0):
        raise ValueError("intrinsics must be finite, with non-zero focal lengths")
    return float(fx), float(fy), float(cx), float(cy)


def _view(intrinsics, size, near=NEAR):
    fx, fy, cx, cy = _intrinsics(intrinsics)
    W, H = int(size[0]), int(size[1])
    if W <= 0 or H <= 0 or W * H > 0x3fffffff:
        raise ValueError(f"a view needs a positive size of fewer than 2^30 pixels (got {W} x {H})")
    v = _capi.SplatMeshView()
    v.width, v.height, v.fx, v.fy, v.cx, v.cy, v.near_z = W, H, fx, fy, cx, cy, float(near)
    return v


def _poses(w2c, dev):
    """[n, 16] float32 on ``dev`` of one or many 4 x 4 world-to-camera matrices (host arrays are rounded once, from float64)."""
    t = _pose_tensor(w2c).to(device=dev, dtype=torch.float32)
    if t.numel() % 16 != 0:
        raise ValueError("poses are 4 x 4 matrices")
    return t.reshape(-1, 16).contiguous()


def to_device_mesh(mesh, device="cuda:0", transform=None):
    """``mesh`` (a ``Mesh`` tuple of device tensors or host arrays, or the path of a PLY) as a ``Mesh`` of float32 / int32 tensors on
    ``device``; ``transform`` (4 x 4) is applied to the vertices in float64 and rounded once.  Colours stay ``None`` when there are none."""
    dev = _device(device, "mesh rendering")
    mesh = _loaded(mesh)
    vertices, faces = mesh[0], mesh[1]
    colors = mesh[2] if len(mesh) > 2 else None

    def tensor(a, dtype):
        if isinstance(a, torch.Tensor):
            return a.detach().to(dev)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)

    v = tensor(vertices, np.float32).reshape(-1, 3)
    if transform is not None:
        m = torch.from_numpy(_transform(transform)).to(dev)
        v = v.double() @ m[:3, :3].T + m[:3, 3]
    f = tensor(faces, np.int64).reshape(-1, 3)
    c = None if colors is None else tensor(colors, np.float32).reshape(-1, 3).float().contiguous()
    return Mesh(v.float().contiguous(), f.to(torch.int32).contiguous(), c)


# ---------------------------------------------------------------------------------------------------------------- the device layer
def render_depth(vertices, faces, w2c, intrinsics, size, near=NEAR, out=None):
    """R: the depth image [H, W] float32 of the mesh ``vertices`` [V, 3] float32 / ``faces`` [F, 3] int32 (device tensors) seen from
    ``w2c`` (4 x 4): per pixel the smallest camera-space z >= ``near`` at which its ray meets a triangle -- either face of it -- and 0 where
    it meets none.  Faces with an index outside the vertices or a non-finite vertex render nothing; a mesh without faces gives a plane of
    zeros.  ``out``: a contiguous float32 [H, W] to render into (one plane of a [k, H, W] chunk, say).  Enqueued on the current stream; nothing
    is read."""
    dev = vertices.device
    _on_device(dev, "render_depth")
    vertices, faces = _mesh_arrays(vertices, faces, dev)
    view = _view(intrinsics, size, near)
    if not (float(near) > 0 and np.isfinite(float(near))):
        raise ValueError("near must be a positive number")
    pose = _poses(w2c, dev)
    if pose.shape[0] != 1:
        raise ValueError("render_depth renders one view: w2c is one 4 x 4 matrix")
    W, H = view.width, view.height
    out = torch.empty(H, W, dtype=torch.float32, device=dev) if out is None else _tensor(out, "out", torch.float32, (H, W), dev, contiguous=True)
    view.w2c = pose.data_ptr()
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_depth(_ptr(vertices, V), V, _ptr(faces, F), F, view, out.data_ptr(), _stream(dev)), "splat_mesh_depth")
    return out


def seen_counts(vertices, w2c, intrinsics, size, edge=0, depth=None, eps=0.0, out=None):
    """S: int32 [V], per vertex the number of the views ``w2c`` [n, 4, 4] in which it has z > 0 and lands on a pixel at least ``edge``
    pixels inside the image and -- with ``depth`` [n, H, W] float32 -- at a depth z <= d + ``eps`` of a pixel with d > 0.  ``out`` is
    INCREMENTED (a long sequence is fed in chunks).  Exact, no atomics.  Enqueued; nothing is read."""
    dev = vertices.device
    _on_device(dev, "seen_counts")
    vertices = _tensor(vertices, "vertices", torch.float32, ("V", 3), dev).contiguous()
    view = _view(intrinsics, size)
    poses = _poses(w2c, dev)
    n, V = int(poses.shape[0]), int(vertices.shape[0])
    if int(edge) < 0 or not float(eps) >= 0:
        raise ValueError("seen_counts needs edge >= 0 and eps >= 0")
    if depth is not None:
        _tensor(depth, "depth", torch.float32, (n, view.height, view.width), dev, contiguous=True)
    out = torch.zeros(V, dtype=torch.int32, device=dev) if out is None else _tensor(out, "out", torch.int32, (V,), dev, contiguous=True)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_seen(_ptr(vertices, V), V, view, _ptr(poses, n), n, int(edge), _ptr(depth, depth is not None and n),
                                                float(eps), _ptr(out, V), _stream(dev)), "splat_mesh_seen")
    return out


def compare_depth(a, b, row, partials=None):
    """D: ``row`` (8 float64 on the device) = (sum |a - b| over all pixels with holes as 0, sum |a - b| where both are > 0, the count of
    those, holes of ``a``, holes of ``b``, pixels, max |a - b|, 0) of two depth planes of one size: a fixed order, no atomics, the same
    bits on every run.  Enqueued; nothing is read."""
    dev = a.device
    for t in (a, b):
        if not (t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.numel() == a.numel()):
            raise RuntimeError("the planes must be contiguous float32 tensors of one size on one device")
    _tensor(row, "row", torch.float64, 8, dev)
    if partials is None:
        partials = torch.empty(_capi.SPLAT_MESH_COMPARE_PARTIALS, dtype=torch.float64, device=dev)
    n = int(a.numel())
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_depth_compare(_ptr(a, n), _ptr(b, n), n, partials.data_ptr(), row.data_ptr(), _stream(dev)),
                    "splat_mesh_depth_compare")
    return row


# ---------------------------------------------------------------------------------------------------------------- culling
def _compact(keep, count):
    """The indices of the ``count`` true elements of ``keep``, in order, without a host read (a stable sort; ``count`` is known)."""
    return torch.argsort((~keep).to(torch.int8), stable=True)[:count]


def cull_mesh(mesh, w2c, intrinsics, size, occlusion=None, eps=0.03, edge=0, rule="all", chunk=16, transform=None, near=NEAR, device="cuda:0"):
    """``mesh`` without what the views ``w2c`` [n, 4, 4] (the poses a run saw, world-to-camera in the mesh's frame) did not see, as a
    ``Mesh`` on the device.  A vertex is seen by a view when it lies in front of the camera on a pixel at least ``edge`` pixels inside
    the image (S) and, with ``occlusion``, no deeper than ``eps`` metres behind that pixel's depth:

    ``occlusion=None``    frusta alone;
    ``occlusion="self"``  against renders of the mesh itself (R), ``chunk`` views at a time -- what testing against a dataset's depth
                          amounts to where that depth is a render of the ground-truth mesh, as on Replica;
    a tensor [n, H, W]    the frames' own depth planes (float32, on the device), or a callable ``(start, stop) -> [stop - start, H, W]``
                          that delivers them chunk by chunk.

    A face survives when all of its vertices were seen by at least one view (``rule="all"``, the protocol's rule) or any of them
    (``rule="any"``); faces that name no vertex are dropped.  Surviving faces keep their order, the vertices they name are renumbered
    densely in their order and colours travel with them; vertices no surviving face names are dropped.  A mesh no view sees comes back
    as an EMPTY ``Mesh`` (0 vertices, 0 faces).  ``transform`` (4 x 4) is applied to the vertices first.  One host read, of the surviving
    sizes.  ``eps`` = 0.03 is recalled from the protocol's script, which is not part of this project: no parity is claimed."""
    if isinstance(occlusion, str) and occlusion != "self":
        raise ValueError(f"occlusion is None, \"self\", a tensor of depth planes or a callable (got {occlusion!r})")
    m = to_device_mesh(mesh, device, transform)
    return cull_meshes([m], w2c, intrinsics, size, occlusion=0 if isinstance(occlusion, str) else occlusion, eps=eps, edge=edge, rule=rule,
                       chunk=chunk, near=near, device=device)[0]


def cull_meshes(meshes, w2c, intrinsics, size, occlusion=None, eps=0.03, edge=0, rule="all", chunk=16, near=NEAR, device="cuda:0"):
    """``cull_mesh`` of several meshes in one frame against the SAME depth planes, which are made once per chunk of views: a list of
    ``Mesh``.  ``occlusion``: ``None``, an int -- the planes are renders of ``meshes[occlusion]`` (a reconstruction and a ground truth
    both tested against what the ground truth hides) --, a tensor [n, H, W] or a callable, as in ``cull_mesh``.  One host read per mesh."""
    if rule not in ("all", "any"):
        raise ValueError(f"rule is \"all\" or \"any\" (got {rule!r})")
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    meshes = [to_device_mesh(m, device, None) for m in meshes]
    dev = _device(device, "mesh rendering")
    poses = _poses(w2c, dev)
    n = int(poses.shape[0])
    view = _view(intrinsics, size, near)
    rendered = isinstance(occlusion, int) and not isinstance(occlusion, bool)
    if rendered and not 0 <= occlusion < len(meshes):
        raise ValueError(f"occlusion names mesh {occlusion} of {len(meshes)}")
    if not (occlusion is None or rendered or callable(occlusion) or isinstance(occlusion, torch.Tensor)):
        raise ValueError(f"occlusion is None, the index of a mesh, a tensor of depth planes or a callable (got {occlusion!r})")
    planes = torch.empty(min(chunk, max(n, 1)), view.height, view.width, dtype=torch.float32, device=dev) if rendered else None
    seen = [torch.zeros(int(m.vertices.shape[0]), dtype=torch.int32, device=dev) for m in meshes]
    for s in range(0, n, chunk):
        p = poses[s:s + chunk]
        k = int(p.shape[0])
        if occlusion is None:
            d = None
        elif rendered:
            for i in range(k):
                render_depth(meshes[occlusion].vertices, meshes[occlusion].faces, p[i], intrinsics, size, near=near, out=planes[i])
            d = planes[:k]
        else:
            d = occlusion(s, s + k) if callable(occlusion) else occlusion[s:s + k]
            d = d.to(device=dev, dtype=torch.float32).contiguous()
        for m, count in zip(meshes, seen):
            seen_counts(m.vertices, p, intrinsics, size, edge=edge, depth=d, eps=eps if d is not None else 0.0, out=count)
    return [_keep_seen(m, count, rule) for m, count in zip(meshes, seen)]


def _keep_seen(mesh, seen, rule):
    """The faces of ``mesh`` whose vertices (all / any of them) have ``seen`` > 0, compacted: one host read, of the surviving sizes."""
    v, f, c = mesh
    V, F = int(v.shape[0]), int(f.shape[0])
    if F == 0 or V == 0:
        return Mesh(v[:0], f[:0], None if c is None else c[:0])
    valid = ((f >= 0) & (f < V)).all(dim=1)
    idx = f.clamp(0, V - 1).long()
    fv = (seen > 0)[idx]
    keep = (fv.all(dim=1) if rule == "all" else fv.any(dim=1)) & valid
    return _keep_faces(mesh, idx, keep)


def _keep_faces(mesh, idx, keep, extra=None):
    """The faces of ``mesh`` flagged in ``keep`` [F] (``idx``: its faces as int64 indices inside the vertices), compacted: surviving faces
    keep their order, the vertices they name are renumbered densely in their order and colours travel with them.  ONE host read, of the
    surviving sizes, with ``extra`` (int64 values on the device, or None) behind them; with ``extra`` the result is (the ``Mesh``, those
    values on the host).  ``cull_mesh`` and ``mesh_clean.clean_mesh`` share it."""
    v, f, c = mesh
    V, F = int(v.shape[0]), int(f.shape[0])
    named = torch.zeros(V, dtype=torch.int32, device=v.device)
    named.index_add_(0, idx.reshape(-1), keep[:, None].expand(F, 3).reshape(-1).to(torch.int32))
    used = named > 0
    sizes = torch.stack((keep.sum(), used.sum()))
    got = (sizes if extra is None else torch.cat((sizes, extra.to(torch.int64).reshape(-1)))).cpu()      # the one read
    nF, nV = int(got[0]), int(got[1])
    fi, vi = _compact(keep, nF), _compact(used, nV)
    renumber = torch.cumsum(used, 0) - 1
    out = Mesh(v[vi].contiguous(), renumber[idx[fi]].to(torch.int32).contiguous(), None if c is None else c[vi].contiguous())
    return out if extra is None else (out, got[2:])


# ---------------------------------------------------------------------------------------------------------------- depth L1
def depth_l1(rec, gt, w2c, intrinsics, size, transform=None, near=NEAR, device="cuda:0"):
    """Depth L1 between the reconstruction ``rec`` and the ground truth ``gt`` (``Mesh`` tuples or PLY paths) rendered at the views
    ``w2c`` [n, 4, 4]: per view R on both meshes, then D into one row of a device table, which is read ONCE at the end.  A dict of

    ``depth_l1_cm``        the mean over the views of the per-view mean of |d_gt - d_rec| over ALL pixels, a hole counting as depth 0, in
                           cm -- the protocol's definition, which charges a hole its full depth;
    ``depth_l1_valid_cm``  the same over the pixels where both meshes have depth, averaged over the views that have such pixels (NaN
                           when none has);
    ``holes_gt`` / ``holes_rec``  pixels without depth, summed over the views; ``max_abs_m``, the largest difference; ``views``.

    ``transform`` (4 x 4) is applied to the reconstruction's vertices, as in ``score_mesh``."""
    r = to_device_mesh(rec, device, transform)
    g = to_device_mesh(gt, device, None)
    dev = r.vertices.device
    poses = _poses(w2c, dev)
    n = int(poses.shape[0])
    if n == 0:
        raise ValueError("depth_l1 needs at least one view")
    view = _view(intrinsics, size, near)
    planes = torch.empty(2, view.height, view.width, dtype=torch.float32, device=dev)
    table = torch.zeros(n, 8, dtype=torch.float64, device=dev)
    partials = torch.empty(_capi.SPLAT_MESH_COMPARE_PARTIALS, dtype=torch.float64, device=dev)
    for k in range(n):
        render_depth(g.vertices, g.faces, poses[k], intrinsics, size, near=near, out=planes[0])
        render_depth(r.vertices, r.faces, poses[k], intrinsics, size, near=near, out=planes[1])
        compare_depth(planes[0], planes[1], table[k], partials)
    t = table.cpu().numpy()                                             # the one read
    with_both = t[:, 2] > 0
    valid = float(np.mean(t[with_both, 1] / t[with_both, 2])) if with_both.any() else float("nan")
    return {"depth_l1_cm": 100.0 * float(np.mean(t[:, 0] / t[:, 5])), "depth_l1_valid_cm": 100.0 * valid, "holes_gt": int(t[:, 3].sum()),
            "holes_rec": int(t[:, 4].sum()), "max_abs_m": float(t[:, 6].max()), "views": n}


# ---------------------------------------------------------------------------------------------------------------- virtual views
def _look_at(origin, target, up):
    z = target - origin
    norm = np.linalg.norm(z)
    z = z / norm if norm > 1e-12 else np.array([1.0, 0.0, 0.0])
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-9:                                        # looking along `up`: any horizontal axis will do
        x = np.cross(z, np.roll(up, 1))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, :3] = np.stack((x, y, z))
    m[:3, 3] = -m[:3, :3] @ origin
    return m


def candidate_views(lo, hi, n, seed=0, shrink=0.7, up=(0.0, 0.0, 1.0), rng=None):
    """[n, 4, 4] float64 world-to-camera look-at poses (x right, y down, z forward; ``up`` is the world's up): origin and target drawn
    uniformly in the box ``lo`` .. ``hi`` shrunk by ``shrink`` about its centre, six numbers per view from ``numpy.random.default_rng(seed)``
    (or from ``rng``, to continue a stream)."""
    rng = np.random.default_rng(seed) if rng is None else rng
    lo, hi, up = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), np.asarray(up, dtype=np.float64)
    centre, half = 0.5 * (lo + hi), 0.5 * float(shrink) * (hi - lo)
    out = np.empty((int(n), 4, 4))
    for k in range(int(n)):
        u = rng.random(6)
        out[k] = _look_at(centre + (2 * u[:3] - 1) * half, centre + (2 * u[3:] - 1) * half, up)
    return out


def sample_views(gt, n, intrinsics, size, seed=0, shrink=0.7, up=(0.0, 0.0, 1.0), max_tries=None, chunk=16, near=NEAR, device="cuda:0"):
    """``n`` virtual views [n, 4, 4] (float32 world-to-camera, on the device) for ``depth_l1``: candidates from ``candidate_views`` are
    rendered against the ground truth ``gt``, ``chunk`` at a time, and one is kept when its render has no hole -- the camera is inside
    the room and sees surface everywhere.  One host read per chunk: this is set-up, not a frame loop.  At most ``max_tries`` candidates
    (default 10 n) are tried; running out raises ``ValueError``.  Deterministic in ``seed``.  ``shrink`` = 0.7 and ``up`` = +z are this
    project's defaults (Replica's rooms stand on z); the protocol's own random stream is not reproduced."""
    g = to_device_mesh(gt, device, None)
    dev = g.vertices.device
    n = int(n)
    max_tries = 10 * n if max_tries is None else int(max_tries)
    if n <= 0 or int(chunk) <= 0:
        raise ValueError("sample_views needs n > 0 and chunk > 0")
    if g.vertices.shape[0] == 0 or g.faces.shape[0] == 0:
        raise ValueError("sample_views needs a mesh with faces")
    box = torch.stack((g.vertices.min(dim=0).values, g.vertices.max(dim=0).values)).double().cpu().numpy()
    view = _view(intrinsics, size, near)
    rng = np.random.default_rng(seed)
    planes = torch.empty(int(chunk), view.height, view.width, dtype=torch.float32, device=dev)
    kept, tries = [], 0
    while len(kept) < n and tries < max_tries:
        k = min(int(chunk), max_tries - tries)
        cand = candidate_views(box[0], box[1], k, shrink=shrink, up=up, rng=rng)
        poses = _poses(cand, dev)
        for i in range(k):
            render_depth(g.vertices, g.faces, poses[i], intrinsics, size, near=near, out=planes[i])
        whole = (planes[:k] > 0).flatten(1).all(dim=1).cpu().numpy()    # the chunk's read
        tries += k
        kept += [poses[i] for i in range(k) if whole[i]]
    if len(kept) < n:
        raise ValueError(f"sample_views: {len(kept)} of {n} hole-free views after {tries} candidates; the mesh is not a closed room seen from "
                           f"inside its box (shrink {shrink}), or max_tries is too small")
    return torch.stack(kept[:n]).reshape(n, 4, 4)


def load_poses(path, every=1):
    """[n, 4, 4] float64 WORLD-TO-CAMERA matrices from a text file of camera-to-world matrices, 16 numbers per line (a Replica
    ``traj.txt``), every ``every``-th line."""
    rows = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            if not line.strip():
                continue
            try:
                vals = [float(x) for x in line.split()]
            except ValueError:
                raise ValueError(f"{path}:{number}: not a line of numbers") from None
            if len(vals) != 16:
                raise ValueError(f"{path}:{number}: a pose is 16 numbers, the line has {len(vals)}")
            rows.append(vals)
    if int(every) <= 0:
        raise ValueError("every must be positive")
    c2w = np.array(rows[::int(every)], dtype=np.float64).reshape(-1, 4, 4)
    if len(c2w) == 0:
        raise ValueError(f"{path}: no poses")
    if not np.isfinite(c2w).all():
        raise ValueError(f"{path}: a pose is not finite")
    return np.linalg.inv(c2w)
