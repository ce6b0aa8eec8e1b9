"""A reconstructed mesh against a ground-truth mesh: ``python -m splatam_amd.mesh_score REC.ply GT.ply [--samples N] [--threshold M]
[--seed S] [--transform FILE] [--device DEV] [--cull-poses TRAJ.txt [--cull-every N] [--cull-size WxH] [--cull-intrinsics FX FY CX CY]
[--occlusion]] [--depth-l1 N] [--align [--align-threshold M] [--align-iterations N]] [--clean [--min-vertices N]]``.

The three figures of the NICE-SLAM evaluation protocol, which SplaTAM's comparison tables use: ACCURACY, the mean distance in cm from
the reconstruction to the ground truth; COMPLETION, the mean distance in cm from the ground truth to the reconstruction; COMPLETION
RATIO, the percentage of ground-truth samples within 5 cm of the reconstruction -- each over 200 000 points sampled uniformly by area
on either surface -- and the precision / recall / F-score at the same threshold.

Everything runs on the device (csrc/meshscore.hip, arithmetic in csrc/meshscore_math.h): triangle areas, a counter-based sampler
(Philox4x32-10: sample ``i`` depends on ``(seed, i)`` alone), a uniform grid over the targets (cell keys, ``torch.sort``, cell starts,
16-byte records) and an exact nearest-neighbour search that walks shells of cells outward, then a reduction without atomics.  Both
meshes are sampled with the SAME seed, so a mesh scored against itself gives exactly 0.

The map lives in the first camera's frame and a ground-truth mesh in the world frame: ``transform`` (``--transform``, a text file of
4 x 4 numbers) is the first frame's ABSOLUTE camera-to-world pose, applied to the reconstruction's vertices.  The dataset loaders make
poses relative to frame 0 and keep no absolute pose: for Replica the matrix is the first line of the sequence's ``traj.txt`` (16
numbers, row-major).

The protocol's preprocessing and its fourth figure live in ``splatam_amd.mesh_render``: ``--cull-poses`` removes from BOTH meshes what
the trajectory's frusta did not see (``--occlusion``: nor what the ground truth itself hides in every frame) before a point is sampled,
and ``--depth-l1 N`` adds the depth L1 between the two meshes rendered at ``N`` virtual views.  Both are off unless asked for.

The protocol's registration step is ``align_icp`` (csrc/icp.hip, arithmetic in csrc/icp_math.h): ``--align`` registers the
reconstruction's vertices to the ground truth's by point-to-point ICP -- after ``--transform`` and the culling, before a point is sampled
-- and prints an ``Alignment:`` line in front of the figures.  Off unless asked for.

Floaters: ``--clean`` (``score_with_views(..., clean=True)`` or a dict of ``mesh_clean.clean_mesh`` keywords) removes the small connected
components of the RECONSTRUCTION alone (csrc/meshclean.hip) -- after ``--transform``, before the culling, the ICP and the samples -- and
prints a ``Cleaning:`` line ahead of ``Alignment:``; the score gains ``cleaning``.  Off unless asked for.

Not here: point-to-plane or coloured ICP, scale, a global registration in front of the ICP.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import sys

import numpy as np
import torch

from . import _capi
from ._mesh_common import _device, _loaded, _on_device, _ptr, _stream, _tensor, _transform
from .mesh import Mesh          # noqa: F401  (re-exported: what score_mesh takes)

MAX_CELLS = _capi.SPLAT_NN_MAX_CELLS
# points per non-empty cell the default cell size aims for (profiles/mesh_score.md 4: 1 .. 16 measured at 200 000 x 200 000; the box's
# own area underestimates a room's surface, so the cells end up holding somewhat more)
POINTS_PER_CELL = 2.0
KEYS = ("accuracy_cm", "completion_cm", "completion_ratio", "precision", "recall", "fscore", "max_rec_to_gt", "max_gt_to_rec", "samples")


def _dims(lo, hi, cell):
    return tuple(int(math.floor((h - l) / cell)) + 1 for l, h in zip(lo, hi))


def plan_grid(lo, hi, count, cell=None, per_cell=POINTS_PER_CELL):
    """(lo, cell, dims) of the grid over the box ``lo`` .. ``hi`` of ``count`` targets: ``lo`` and ``cell`` as float32 values, ``dims`` =
    floor(extent / cell) + 1 per axis.  ``cell=None``: the targets are taken to lie on a surface of about the box's own area
    A = 2 (ex ey + ey ez + ez ex), which has A / cell^2 non-empty cells: cell = sqrt(per_cell A / count).  Whatever the cell, it grows
    until the grid has at most 2^21 cells, so the walk of a stray query is bounded."""
    lo = tuple(float(np.float32(v)) for v in lo)
    hi = tuple(float(np.float32(v)) for v in hi)
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in lo + hi) or not all(h >= l for l, h in zip(lo, hi)):
        raise ValueError(f"a grid needs a finite box (got {lo} .. {hi})")
    e = [h - l for l, h in zip(lo, hi)]
    if cell is None:
        area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
        cell = math.sqrt(per_cell * area / max(int(count), 1)) if area > 0 else max(e) / max(int(count), 1)
        if not cell > 0:
            cell = 1.0
    cell = float(np.float32(cell))
    if not (cell > 0 and math.isfinite(cell)):
        raise ValueError(f"a grid needs a positive cell size (got {cell})")
    cell = max(cell, float(np.float32(max(e) / 2.0 ** 30)))             # (dims stay far inside int32)
    dims = _dims(lo, hi, cell)
    while dims[0] * dims[1] * dims[2] > MAX_CELLS:
        cell = float(np.float32(cell * 1.125))
        dims = _dims(lo, hi, cell)
    return lo, cell, dims


def _points(t, dev, what):
    return _tensor(t, what, torch.float32, ("n", 3), dev).contiguous()


def surface_prefix(vertices, faces):
    """The inclusive double prefix sum of the triangle areas (M0, then ``torch.cumsum``) of a mesh on the device: [F] float64."""
    dev = vertices.device
    L = _capi.lib()
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    area = torch.empty(F, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _capi.check(L.splat_mesh_areas(_ptr(vertices, V), V, _ptr(faces, F), F, _ptr(area, F), _stream(dev)), "splat_mesh_areas")
    return area, torch.cumsum(area, 0)


def sample_surface(vertices, faces, n, seed=0, prefix=None):
    """``n`` points uniformly by area on the mesh ``vertices`` [V, 3] float32, ``faces`` [F, 3] int32 (device tensors): ``(points [n, 3]
    float32, face [n] int32)``.  Sample ``i`` depends on ``(seed, i)`` alone -- not on ``n``, not on the launch.  Zero-area triangles
    get no sample.  Enqueued on the current stream; nothing is read."""
    dev = vertices.device
    _on_device(dev, "sample_surface")
    vertices = _points(vertices, dev, "vertices")
    faces = _tensor(faces, "faces", torch.int32, ("F", 3), dev).contiguous()
    V, F, n = int(vertices.shape[0]), int(faces.shape[0]), int(n)
    if F == 0 or n < 0:
        raise ValueError("sample_surface needs a mesh with faces and n >= 0")
    if prefix is None:
        prefix = surface_prefix(vertices, faces)[1]
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_sample(_ptr(vertices, V), V, faces.data_ptr(), F, prefix.data_ptr(), int(seed) & (2 ** 64 - 1), n,
                                                  _ptr(points, n), _ptr(face, n), _stream(dev)), "splat_mesh_sample")
    return points, face


class NearestGrid:
    """A uniform grid over ``targets`` [M, 3] float32 on the device for exact nearest-neighbour queries.  ``cell=None`` picks the cell
    size from the target count and bounding box (``plan_grid``); ``bounds`` = (lo, hi) of the targets when the caller knows them
    (otherwise ONE host read of the box).  Built by three enqueued steps: cell keys (M2), ``torch.sort(stable=True)``, cell starts and
    records (M3)."""

    def __init__(self, targets, cell=None, bounds=None):
        dev = targets.device if isinstance(targets, torch.Tensor) else None
        if dev is None or dev.type != "cuda":
            raise RuntimeError("NearestGrid needs a float32 tensor [M, 3] on a CUDA/HIP device; the HIP library has no CPU path")
        self.dev = dev
        self.targets = targets = _points(targets, dev, "targets")
        M = self.count = int(targets.shape[0])
        if M >= 2 ** 31:
            raise ValueError(f"{M} targets do not fit int32 indices")
        if bounds is None:
            if M:
                box = torch.stack((targets.min(dim=0).values, targets.max(dim=0).values)).double().cpu().numpy()
                bounds = (box[0], box[1])
            else:
                bounds = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        self.lo, self.cell, self.dims = plan_grid(bounds[0], bounds[1], M, cell)
        self.cells = self.dims[0] * self.dims[1] * self.dims[2]
        g = self.struct = _capi.SplatNnGrid()
        g.lo[:] = self.lo
        g.cell = self.cell
        g.dims[:] = self.dims
        g.count = M
        self.L = _capi.lib()
        self.records = torch.empty(max(M, 1), 4, dtype=torch.float32, device=dev)
        self.start = torch.empty(self.cells + 1, dtype=torch.int32, device=dev)
        key, order = self._sorted_keys(targets)
        with torch.cuda.device(dev):
            _capi.check(self.L.splat_nn_cell_starts(C.byref(g), _ptr(key, M), _ptr(order, M),
                                                    _ptr(targets, M), self.records.data_ptr(), self.start.data_ptr(),
                                                    _stream(dev)), "splat_nn_cell_starts")
        g.records, g.start = self.records.data_ptr(), self.start.data_ptr()

    def _sorted_keys(self, points):
        n = int(points.shape[0])
        key = torch.empty(n, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_nn_cell_keys(C.byref(self.struct), _ptr(points, n), n, _ptr(key, n),
                                                  _stream(self.dev)), "splat_nn_cell_keys")
        key, order = torch.sort(key, stable=True)
        return key, order.to(torch.int32)

    def cell_order(self, points):
        """The permutation that sorts ``points`` by cell (int32 [n]): what ``query`` computes for itself unless given one."""
        return self._sorted_keys(_points(points, self.dev, "points"))[1]

    def query(self, points, account=False, sort=True, order=None):
        """``(dist2 [n] float32, index [n] int32)`` of ``points`` [n, 3] float32, in their order: the squared distance to the nearest
        target (``(dx dx + dy dy) + dz dz`` in float32) and its index, the lowest among equals.  Exact.  The queries are sorted by cell
        first (``sort=False``: taken as they come), so that a wave's lanes read the same cells.  ``account=True`` adds an int32 [n, 2]
        of (candidates evaluated, shells walked).  ``order`` (int32 [n], a permutation, e.g. an earlier ``cell_order``) replaces the sort:
        it only sets the processing order, never the result.  Enqueued; nothing is read."""
        points = _points(points, self.dev, "points")
        n = int(points.shape[0])
        dist2 = torch.empty(n, dtype=torch.float32, device=self.dev)
        index = torch.empty(n, dtype=torch.int32, device=self.dev)
        acc = torch.empty(n, 2, dtype=torch.int32, device=self.dev) if account else None
        if order is not None:
            if not (isinstance(order, torch.Tensor) and order.dtype == torch.int32 and order.device == self.dev and order.shape == (n,)
                    and order.is_contiguous()):
                raise RuntimeError(f"order must be a contiguous int32 vector of {n} on {self.dev}")
        else:
            order = self._sorted_keys(points)[1] if sort and n else None
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_nn_query(C.byref(self.struct), _ptr(points, n), order.data_ptr() if order is not None else None,
                                              n, _ptr(dist2, n), _ptr(index, n),
                                              acc.data_ptr() if account and n else None, _stream(self.dev)), "splat_nn_query")
        return (dist2, index, acc) if account else (dist2, index)


def reduce_distances(dist2, threshold, row, partials=None):
    """M5: ``row`` (4 float64 on the device) = (sum of d, count of d < threshold, max of d, n) over d = sqrt((double)dist2): a fixed
    order, no atomics, the same bits on every run.  Enqueued; nothing is read."""
    dev = dist2.device
    if not (dist2.dtype == torch.float32 and dist2.dim() == 1 and dist2.is_contiguous()):
        raise RuntimeError("dist2 must be a contiguous float32 vector")
    _tensor(row, "row", torch.float64, 4, dev)
    if partials is None:
        partials = torch.empty(3 * _capi.SPLAT_NN_REDUCE_ROWS, dtype=torch.float64, device=dev)
    n = int(dist2.shape[0])
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_nn_reduce(_ptr(dist2, n), n, float(threshold), partials.data_ptr(), row.data_ptr(),
                                                _stream(dev)), "splat_nn_reduce")
    return row


ICP_STATUS = ("running", "converged", "iteration limit", "fewer than three correspondences")
# the queries are re-sorted by cell when this many iterations have passed since the last sort (profiles/icp.md 3)
ICP_RESORT_EVERY = 5


def _rigid(init):
    m = np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError("init must be a finite 4 x 4 matrix")
    R = m[:3, :3]
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or not np.linalg.det(R) > 0 or not np.array_equal(m[3], (0.0, 0.0, 0.0, 1.0)):
        raise ValueError("init must be a rigid motion: a proper rotation, a translation and the bottom row 0 0 0 1")
    return m


def motion_of(T):
    """(translation in cm, rotation in degrees) of the rigid motion ``T`` [4, 4]."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    skew = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 100.0 * float(np.linalg.norm(T[:3, 3])), math.degrees(math.atan2(float(np.linalg.norm(skew)), 0.5 * (float(np.trace(R)) - 1.0)))


def apply_state(source, state, out=None):
    """I1: ``float32(R p + t)`` of ``source`` [n, 3] float32, the motion read from the ICP state row on the device (one rounding).
    Enqueued; nothing is read."""
    dev = source.device
    n = int(source.shape[0])
    moved = torch.empty(n, 3, dtype=torch.float32, device=dev) if out is None else out
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_icp_transform(_ptr(source, n), n, state.data_ptr(), _ptr(moved, n),
                                                    _stream(dev)), "splat_icp_transform")
    return moved


def accumulate_moments(source, targets, dist2, index, threshold, origin, state, partials=None):
    """I2: ``partials`` [SPLAT_ICP_ROWS, 17] float64 of the correspondences among ``source`` (``dist2`` / ``index``: what the grid's query
    returned for the moved source).  Enqueued; nothing is read."""
    dev = source.device
    n, m = int(source.shape[0]), int(targets.shape[0])
    if partials is None:
        partials = torch.zeros(_capi.SPLAT_ICP_ROWS, _capi.SPLAT_ICP_SUMS, dtype=torch.float64, device=dev)
    c = (C.c_double * 3)(*[float(v) for v in origin])
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_icp_accumulate(_ptr(source, n), _ptr(targets, m), m,
                                                     _ptr(dist2, n), _ptr(index, n), n, float(threshold), c,
                                                     state.data_ptr(), partials.data_ptr(), _stream(dev)), "splat_icp_accumulate")
    return partials


def align_icp(source, target, threshold=0.1, init=None, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, check_every=5,
              grid=None, target_bounds=None):
    """Point-to-point ICP of ``source`` [n, 3] onto ``target`` [m, 3] (float32 device tensors) as the NICE-SLAM protocol runs it (Open3D's
    ``registration_icp`` settings: correspondences closer than ``threshold`` metres, start at ``init`` or the identity, at most
    ``max_iterations`` updates, stop when fitness and inlier RMSE both change by less than ``relative_*``): a dict of ``transformation``
    ([4, 4] float64 numpy, source -> target), ``fitness`` (correspondences / n), ``inlier_rmse`` (metres), ``correspondences``,
    ``iterations`` (updates applied), ``status`` (1 converged, 2 iteration limit, 3 fewer than three correspondences) and ``history``
    ([k, 4]: count, fitness, inlier RMSE, status per evaluation).

    Each iteration is I1 (move by the device's T), the grid's exact query, I2 (17 moments, no atomics), I3 (stop test, Horn's solve,
    T <- U T), all enqueued; ``check_every`` iterations go between two host reads of the state row, and because T freezes on the device
    once the loop has stopped the result is the same bits whatever ``check_every``.  ``grid``: a ``NearestGrid`` over ``target`` built
    earlier; ``target_bounds`` = (lo, hi) spares the grid's one read of the box."""
    dev = source.device if isinstance(source, torch.Tensor) else None
    if dev is None or dev.type != "cuda" or not isinstance(target, torch.Tensor) or target.device.type != "cuda":
        raise RuntimeError("align_icp needs float32 tensors [n, 3] on a CUDA/HIP device; the HIP library has no CPU path")
    source, target = _points(source, dev, "source"), _points(target, dev, "target")
    n, m = int(source.shape[0]), int(target.shape[0])
    if n == 0 or m == 0:
        raise ValueError("align_icp needs at least one source and one target point")
    threshold, max_iterations, check_every = float(threshold), int(max_iterations), int(check_every)
    if not (threshold > 0 and math.isfinite(threshold)):
        raise ValueError(f"align_icp needs a positive finite threshold (got {threshold})")
    if max_iterations < 0 or check_every < 1 or not (relative_fitness >= 0 and relative_rmse >= 0):
        raise ValueError("align_icp needs max_iterations >= 0, check_every >= 1 and relative_fitness, relative_rmse >= 0")
    T0 = np.eye(4) if init is None else _rigid(init)
    if grid is None:
        grid = NearestGrid(target, bounds=target_bounds)
    elif grid.dev != dev or grid.count != m:
        raise ValueError("grid was not built over these targets")
    origin = [grid.lo[k] + 0.5 * grid.cell * grid.dims[k] for k in range(3)]             # about the centre of the targets' box
    L = _capi.lib()
    ns, rows = _capi.SPLAT_ICP_STATE, max_iterations + 1
    host = np.zeros(ns + 4 * rows)
    host[:16] = T0.reshape(-1)
    buf = torch.from_numpy(host).to(dev)                                # the state row and the history behind it: one read fetches both
    state, history = buf[:ns], buf[ns:]
    partials = torch.empty(_capi.SPLAT_ICP_ROWS, _capi.SPLAT_ICP_SUMS, dtype=torch.float64, device=dev)
    moved = torch.empty(n, 3, dtype=torch.float32, device=dev)
    c = (C.c_double * 3)(*origin)
    order, done, got = None, 0, None
    for _ in range(-(-rows // check_every)):
        for _ in range(min(check_every, rows - done)):
            apply_state(source, state, out=moved)
            if done % ICP_RESORT_EVERY == 0:
                order = grid.cell_order(moved)
            dist2, index = grid.query(moved, order=order)
            accumulate_moments(source, target, dist2, index, threshold, origin, state, partials)
            with torch.cuda.device(dev):
                _capi.check(L.splat_icp_solve(partials.data_ptr(), n, max_iterations, float(relative_fitness), float(relative_rmse), c,
                                              state.data_ptr(), history.data_ptr(), _stream(dev)), "splat_icp_solve")
            done += 1
        got = buf.cpu().numpy()                                         # the one read of this block
        if got[_capi.SPLAT_ICP_STATUS] != 0:
            break
    assert got is not None and got[_capi.SPLAT_ICP_STATUS] != 0, "the iteration limit ends the loop"
    it = int(got[_capi.SPLAT_ICP_ITERATION])
    return {"transformation": got[:16].reshape(4, 4).copy(), "fitness": float(got[_capi.SPLAT_ICP_FITNESS]),
            "inlier_rmse": float(got[_capi.SPLAT_ICP_RMSE]), "correspondences": int(got[_capi.SPLAT_ICP_COUNT]), "iterations": it,
            "status": int(got[_capi.SPLAT_ICP_STATUS]), "history": got[ns:].reshape(rows, 4)[:it + 1].copy()}


def align_vertices(rec_vertices, gt_vertices, align, gt_bounds=None):
    """The protocol's registration step: ``align_icp`` of the reconstruction's vertices onto the ground truth's (``align``: True or a dict
    of ``align_icp`` keywords), then the motion found applied to the reconstruction's vertices in double, rounded once (I1).  Returns
    (aligned vertices, the ``align_icp`` dict plus ``translation_cm`` and ``rotation_deg``)."""
    keywords = dict(align) if isinstance(align, dict) else {}
    keywords.setdefault("target_bounds", gt_bounds)
    found = align_icp(rec_vertices, gt_vertices, **keywords)
    state = torch.from_numpy(np.concatenate((found["transformation"].reshape(-1), np.zeros(_capi.SPLAT_ICP_STATE - 16)))).to(rec_vertices.device)
    found["translation_cm"], found["rotation_deg"] = motion_of(found["transformation"])
    return apply_state(rec_vertices, state), found


def _load(mesh, dev, transform, what):
    """(vertices float32 [V, 3] on dev, faces int32 [F, 3] on dev, bounds or None): a path or host arrays go through numpy (bounds known
    without a device read), device tensors stay there."""
    mesh = _loaded(mesh)
    vertices, faces = mesh[0], mesh[1]
    if isinstance(vertices, torch.Tensor) and vertices.device.type == "cuda":
        v = vertices.detach().to(dev).reshape(-1, 3)
        if transform is not None:
            m = torch.as_tensor(np.asarray(transform, dtype=np.float64), device=dev)
            v = (v.double() @ m[:3, :3].T + m[:3, 3]).float()
        v, f, bounds = v.float().contiguous(), faces.detach().to(dev).to(torch.int32).reshape(-1, 3).contiguous(), None
    else:
        v = np.asarray(vertices.detach().cpu() if isinstance(vertices, torch.Tensor) else vertices, dtype=np.float32).reshape(-1, 3)
        f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).reshape(-1, 3)
        if transform is not None:
            m = np.asarray(transform, dtype=np.float64)
            v = (v.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
        if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
            raise ValueError(f"{what}: faces index vertices that do not exist")
        bounds = (v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)) if v.shape[0] else None
        v, f = torch.from_numpy(np.ascontiguousarray(v)).to(dev), torch.from_numpy(np.ascontiguousarray(f.astype(np.int32))).to(dev)
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError(f"{what}: a mesh without faces cannot be sampled")
    return v, f, bounds


def score_mesh(rec, gt, samples=200_000, threshold=0.05, seed=0, transform=None, device="cuda:0", cell=None, align=False):
    """The reconstruction ``rec`` against the ground truth ``gt`` (each a ``Mesh`` tuple -- device tensors or host arrays -- or the path
    of a PLY): a dict of ``accuracy_cm`` (mean distance rec -> gt, cm), ``completion_cm`` (gt -> rec, cm), ``completion_ratio`` (percent
    of gt samples with a distance below ``threshold`` metres), ``precision`` / ``recall`` / ``fscore`` at ``threshold`` (fractions),
    ``max_rec_to_gt`` / ``max_gt_to_rec`` (metres) and ``samples``.  ``transform``: a 4 x 4 applied to the reconstruction's vertices (in
    float64, rounded once) -- the first frame's absolute camera-to-world pose, for a map in the first camera's frame.

    ``samples`` points are drawn on either surface with the same ``seed``; both directions are enqueued and the table of their rows is
    read with ONE host read (meshes given as device tensors cost one more read before, of their boxes).  No engine and no map is
    touched: the inputs are meshes.

    ``align`` (True, or a dict of ``align_icp`` keywords): the protocol's registration -- after ``transform``, the reconstruction's
    VERTICES are registered to the ground truth's by point-to-point ICP and moved by what it finds before a point is sampled; the score
    gains ``alignment``, the ``align_icp`` dict plus ``translation_cm`` and ``rotation_deg`` of that motion.

    Cleaning the reconstruction first: ``score_with_views(..., clean=True)``; this function's signature is as it was."""
    return _score_mesh(rec, gt, samples, threshold, seed, transform, device, cell, align, None)


def _score_mesh(rec, gt, samples, threshold, seed, transform, device, cell, align, clean):
    """``score_mesh`` with ``clean`` (None, True, or a dict of ``mesh_clean.clean_mesh`` keywords): the RECONSTRUCTION alone loses its
    small connected components after ``transform`` and before everything else (one more host read); the score gains ``cleaning``,
    ``clean_mesh``'s report.  A reconstruction given as host arrays or a path keeps the box of the uncleaned mesh for its search grid,
    which changes no figure."""
    from .mesh_clean import clean_options
    clean = clean_options(clean)
    dev = _device(device, "the mesh score")
    samples = int(samples)
    if samples <= 0 or not float(threshold) > 0:
        raise ValueError("score_mesh needs samples > 0 and threshold > 0")
    rv, rf, rb = _load(rec, dev, _transform(transform), "the reconstruction")
    gv, gf, gb = _load(gt, dev, None, "the ground truth")
    cleaning = None
    if clean is not None:
        from .mesh_clean import clean_mesh
        cleaned, cleaning = clean_mesh(Mesh(rv, rf, None), device=dev, report=True, **clean)
        rv, rf = cleaned.vertices, cleaned.faces
        if rf.shape[0] == 0:
            raise ValueError("the reconstruction: cleaning removed every component")
    if rb is None or gb is None:                                        # device meshes: both boxes with one read
        box = torch.stack((rv.min(dim=0).values, rv.max(dim=0).values, gv.min(dim=0).values, gv.max(dim=0).values)).double().cpu().numpy()
        rb, gb = (box[0], box[1]), (box[2], box[3])
    alignment = None
    if align:
        rv, alignment = align_vertices(rv, gv, align, gt_bounds=gb)
        box = torch.stack((rv.min(dim=0).values, rv.max(dim=0).values)).double().cpu().numpy()
        rb = (box[0], box[1])
    table = torch.zeros(3, 4, dtype=torch.float64, device=dev)          # rec -> gt, gt -> rec, (area rec, area gt, 0, 0)
    partials = torch.empty(3 * _capi.SPLAT_NN_REDUCE_ROWS, dtype=torch.float64, device=dev)
    pts = []
    for n, (v, f) in enumerate(((rv, rf), (gv, gf))):
        prefix = surface_prefix(v, f)[1]
        table[2, n:n + 1].copy_(prefix[-1:])
        pts.append(sample_surface(v, f, samples, seed, prefix=prefix)[0])
    for n, (queries, targets, bounds) in enumerate(((pts[0], pts[1], gb), (pts[1], pts[0], rb))):
        dist2, _ = NearestGrid(targets, cell=cell, bounds=bounds).query(queries)
        reduce_distances(dist2, threshold, table[n], partials)
    t = table.cpu().numpy()                                             # the one read
    if not (t[2, 0] > 0 and t[2, 1] > 0 and np.isfinite(t[2, :2]).all()):
        raise ValueError(f"a mesh without surface area cannot be scored (areas {t[2, 0]}, {t[2, 1]})")
    n = float(samples)
    precision, recall = t[0, 1] / n, t[1, 1] / n
    score = {"accuracy_cm": 100.0 * t[0, 0] / n, "completion_cm": 100.0 * t[1, 0] / n, "completion_ratio": 100.0 * recall,
             "precision": precision, "recall": recall, "fscore": 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0,
             "max_rec_to_gt": float(t[0, 2]), "max_gt_to_rec": float(t[1, 2]), "samples": samples}
    if cleaning is not None:
        score["cleaning"] = cleaning
    if alignment is not None:
        score["alignment"] = alignment
    return score


def score_culled_in_map_frame(rec, gt, w2c, intrinsics, size, gt_transform=None, device="cuda:0", **score):
    """``score_mesh`` of a reconstruction in the MAP's frame against a ground truth in the world frame, both culled first to the frusta of
    ``w2c`` ([n, 4, 4] world-to-camera poses in the map's frame: a run's own).  ``gt_transform`` is what ``score_mesh`` would apply to the
    reconstruction, the first frame's absolute camera-to-world pose; its INVERSE brings the ground truth into the map's frame, where
    both are culled and scored -- distances do not change under a rigid motion.  Further keywords go to ``score_mesh``; ``clean``
    among them cleans the reconstruction BEFORE it is culled."""
    from .mesh_clean import clean_mesh, clean_options
    from .mesh_render import cull_mesh
    to_map = None if gt_transform is None else np.linalg.inv(_transform(gt_transform))
    clean, cleaning = clean_options(score.pop("clean", None)), None
    if clean is not None:
        rec, cleaning = clean_mesh(rec, device=device, report=True, **clean)
    rec_c = cull_mesh(rec, w2c, intrinsics, size, device=device)
    gt_c = cull_mesh(gt, w2c, intrinsics, size, transform=to_map, device=device)
    for m, what in ((rec_c, "reconstruction"), (gt_c, "ground truth")):
        if m.faces.shape[0] == 0:
            raise ValueError(f"the run's views see nothing of the {what}: is the transform the first frame's camera-to-world pose?")
    result = score_mesh(rec_c, gt_c, device=device, **score)
    if cleaning is not None:
        result["cleaning"] = cleaning
    return result


def load_transform(path):
    """A 4 x 4 matrix from a text file of 16 numbers (any whitespace; further lines -- a whole ``traj.txt`` -- are ignored)."""
    with open(path) as f:
        values = f.read().split()[:16]
    try:
        m = np.array([float(v) for v in values], dtype=np.float64)
    except ValueError:
        raise ValueError(f"{path}: not a matrix of numbers") from None
    if m.size != 16:
        raise ValueError(f"{path}: a 4 x 4 matrix needs 16 numbers, the file has {m.size}")
    return m.reshape(4, 4)


def format_alignment(a):
    return (f"Alignment: fitness {a['fitness']:.6f}, inlier RMSE {100.0 * a['inlier_rmse']:.4f} cm, {a['iterations']} iterations "
            f"({ICP_STATUS[a['status']]}), translation {a['translation_cm']:.4f} cm, rotation {a['rotation_deg']:.4f} deg")


def format_score(score):
    text = ""
    if score.get("cleaning") is not None:
        from .mesh_clean import format_cleaning
        text += format_cleaning(score["cleaning"]) + "\n"
    if score.get("alignment") is not None:
        text += format_alignment(score["alignment"]) + "\n"
    text += (f"Accuracy: {score['accuracy_cm']:.4f} cm\nCompletion: {score['completion_cm']:.4f} cm\n"
            f"Completion ratio: {score['completion_ratio']:.4f} %\nF-score: {score['fscore']:.6f} "
            f"(precision {score['precision']:.6f}, recall {score['recall']:.6f}; {score['samples']} samples)")
    if score.get("depth_l1_cm") is not None:                            # (only when mesh_render.depth_l1 was asked for)
        text += (f"\nDepth L1: {score['depth_l1_cm']:.4f} cm (where both have depth {score['depth_l1_valid_cm']:.4f} cm; holes "
                 f"{score['holes_gt']} gt, {score['holes_rec']} rec; {score['views']} views)")
    return text


# Replica as the NICE-SLAM protocol renders it: 1200 x 680, focal length 600, the principal point at the image's centre
CULL_SIZE, CULL_INTRINSICS = "1200x680", (600.0, 600.0, 599.5, 339.5)


def score_with_views(rec, gt, samples=200_000, threshold=0.05, seed=0, transform=None, device="cuda:0", cull_w2c=None, intrinsics=CULL_INTRINSICS,
                     size=(1200, 680), occlusion=False, depth_l1_views=0, clean=None, align=False):
    """``score_mesh`` behind the protocol's preprocessing: with ``cull_w2c`` ([n, 4, 4] world-to-camera in the ground truth's frame) both
    meshes are culled to those views first (``mesh_render.cull_mesh``; ``occlusion``: each against renders of the ground truth), and
    ``depth_l1_views`` > 0 adds ``mesh_render.depth_l1`` at that many views from ``mesh_render.sample_views`` (same ``seed``).  Without
    either this is ``score_mesh``.  ``align`` (``score_mesh``'s): the ICP runs on the CULLED meshes' vertices, and the samples, the
    distances and the depth L1 are those of the aligned reconstruction.  ``clean`` (``score_mesh``'s): the reconstruction is cleaned
    after ``transform`` and before it is culled -- the order is ``transform``, clean, cull, ICP, samples."""
    from . import mesh_render as MR
    from .mesh_clean import clean_mesh, clean_options
    if cull_w2c is None and not depth_l1_views:
        return _score_mesh(rec, gt, samples, threshold, seed, transform, device, None, align, clean)
    clean, cleaning = clean_options(clean), None
    r, g = MR.to_device_mesh(rec, device, _transform(transform)), MR.to_device_mesh(gt, device, None)
    if clean is not None:
        r, cleaning = clean_mesh(r, device=device, report=True, **clean)
        if r.faces.shape[0] == 0:
            raise ValueError("the reconstruction: cleaning removed every component")
    if cull_w2c is not None:                                            # (occlusion: both against ONE set of renders of the ground truth)
        r, g = MR.cull_meshes([r, g], cull_w2c, intrinsics, size, occlusion=1 if occlusion else None, device=device)
        for m, what in ((r, "reconstruction"), (g, "ground truth")):
            if m.faces.shape[0] == 0:
                raise ValueError(f"the views see nothing of the {what}: are the poses in the ground truth's frame (--transform)?")
    alignment = None
    if align:
        aligned, alignment = align_vertices(r.vertices, g.vertices, align)
        r = Mesh(aligned, r.faces, r.colors)
    score = score_mesh(r, g, samples=samples, threshold=threshold, seed=seed, device=device)
    if cleaning is not None:
        score["cleaning"] = cleaning
    if alignment is not None:
        score["alignment"] = alignment
    if depth_l1_views:
        views = MR.sample_views(g, depth_l1_views, intrinsics, size, seed=seed, device=device)
        score.update(MR.depth_l1(r, g, views, intrinsics, size, device=device))
    return score


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.mesh_score", description=__doc__.split("\n\n")[1])
    parser.add_argument("rec", help="the reconstruction (PLY)")
    parser.add_argument("gt", help="the ground truth (PLY)")
    parser.add_argument("--samples", type=int, default=200_000, help="points sampled on either surface")
    parser.add_argument("--threshold", type=float, default=0.05, help="metres: completion ratio and F-score")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--transform", default=None, metavar="FILE",
                        help="text file of a 4 x 4 matrix applied to the reconstruction: the first frame's absolute camera-to-world pose")
    parser.add_argument("--device", default="cuda:0")
    parser.add_argument("--cull-poses", default=None, metavar="FILE",
                        help="text file of 4 x 4 camera-to-world matrices, one per line (a Replica traj.txt), in the ground truth's frame: "
                             "both meshes are culled to these frusta first")
    parser.add_argument("--cull-every", type=int, default=1, metavar="N", help="use every N-th pose of --cull-poses")
    parser.add_argument("--cull-size", default=CULL_SIZE, metavar="WxH", help="image size of the culling and depth L1 views")
    parser.add_argument("--cull-intrinsics", type=float, nargs=4, default=CULL_INTRINSICS, metavar=("FX", "FY", "CX", "CY"))
    parser.add_argument("--occlusion", action="store_true", help="with --cull-poses: also cull what the ground truth hides in every frame")
    parser.add_argument("--depth-l1", type=int, default=0, metavar="N", help="add depth L1 over N virtual views rendered from both meshes")
    parser.add_argument("--align", action="store_true",
                        help="register the reconstruction's vertices to the ground truth's by point-to-point ICP before scoring")
    parser.add_argument("--align-threshold", type=float, default=None, metavar="M", help="with --align: correspondence distance in metres (0.1)")
    parser.add_argument("--align-iterations", type=int, default=None, metavar="N", help="with --align: at most N updates (30)")
    parser.add_argument("--clean", action="store_true",
                        help="remove the reconstruction's small connected components first (splatam_amd.mesh_clean); prints a Cleaning: line")
    parser.add_argument("--min-vertices", type=int, default=None, metavar="N", help="with --clean: components with fewer vertices go (200)")
    args = parser.parse_args(argv)
    if args.min_vertices is not None and not args.clean:
        parser.error("--min-vertices needs --clean")
    cleaning = {}
    if args.clean:
        cleaning = {"clean": {"min_vertices": args.min_vertices} if args.min_vertices is not None else True}
    if args.occlusion and not args.cull_poses:
        parser.error("--occlusion needs --cull-poses")
    if (args.align_threshold is not None or args.align_iterations is not None) and not args.align:
        parser.error("--align-threshold and --align-iterations need --align")
    align = False
    if args.align:
        align = {k: v for k, v in (("threshold", args.align_threshold), ("max_iterations", args.align_iterations)) if v is not None} or True
    try:
        transform = load_transform(args.transform) if args.transform else None
        if args.cull_poses or args.depth_l1:
            from .mesh_render import load_poses, parse_size
            score = score_with_views(args.rec, args.gt, samples=args.samples, threshold=args.threshold, seed=args.seed, transform=transform,
                                     device=args.device, cull_w2c=load_poses(args.cull_poses, args.cull_every) if args.cull_poses else None,
                                     intrinsics=tuple(args.cull_intrinsics), size=parse_size(args.cull_size), occlusion=args.occlusion,
                                     depth_l1_views=args.depth_l1, align=align, **cleaning)
        elif cleaning:
            score = score_with_views(args.rec, args.gt, samples=args.samples, threshold=args.threshold, seed=args.seed, transform=transform,
                                     device=args.device, align=align, **cleaning)
        else:
            score = score_mesh(args.rec, args.gt, samples=args.samples, threshold=args.threshold, seed=args.seed, transform=transform,
                               device=args.device, align=align)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e)) from None
    print(format_score(score), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
