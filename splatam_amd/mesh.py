"""A triangle mesh of the map: ``python -m splatam_amd.mesh PARAMS.npz --out mesh.ply [--voxel M] [--trunc M] [--every N] [--size WxH]
[--sil-thres S] [--depth-max M] [--bounds X0 Y0 Z0 X1 Y1 Z1] [--sparse] [--method {tetrahedra,cubes}] [--clean [--min-vertices N] [--min-area M2] [--keep-largest K]]``.

Depth rendered at the estimated poses is fused into a truncated signed distance volume and the volume's zero surface is extracted,
all on the device (csrc/tsdf.hip, arithmetic in csrc/tsdf_math.h): the usual deliverable of a dense RGB-D SLAM system, and what the
methods SplaTAM is compared with are scored on.  ``FusedEngine.render_view(..., rgb8=False)`` leaves a view's six planes and its
``w2c`` in device buffers; ``TsdfVolume.integrate`` takes them from there, gated on the device by the view's truncation status.

The surface is marching tetrahedra on Kuhn's split of every cell (six tetrahedra, translation invariant, so neighbouring cells agree
on their shared faces and the mesh is closed wherever the volume was seen); vertices are named by the grid edge they lie on, so
welding is a ``torch.unique`` over integer keys and the result is canonical: vertices sorted by key, faces lexicographically -- the
same volume always gives the same bytes.  ``--method cubes`` (``method="cubes"``) extracts the same surface by marching cubes
instead: vertices on the grid's axis edges only -- the tetrahedra's own vertices there, bit for bit --, at most 5 triangles a cell
against 12, a third of the triangles and a third to a half of the vertices, closed by the same kind of argument (csrc/tsdf_math.h "SURFACE, cubes": one
rule on every face's four signs, which the neighbouring cell reads reversed).  No asymptotic decider (MC33), no parity with another
library's table, no dual contouring.

The dense ``TsdfVolume`` holds five floats for every grid point of the box and is refused beyond ``max_bytes``; ``--sparse``
(``SparseTsdfVolume``, csrc/tsdf_sparse.hip) stores only the bricks of 2048 grid points within the truncation band of a surface some
view saw and gives the same mesh bit for bit: an apartment at 1 cm, a room at 5 mm, a walk down a corridor.

``--clean`` (``extract_mesh(..., clean=True)`` or a dict of ``mesh_clean.clean_mesh`` keywords) removes the mesh's small connected
components -- the floaters of rendered depth -- on the device before it is returned or written.  Off by default.

``--simplify CELL [--simplify-placement quadric|mean]`` (``mesh_from_params(..., simplify=CELL)``) merges the vertices in each cell of
a grid of that edge, placed by the cell's quadrics, after the cleaning and before the file (``mesh_simplify.simplify_mesh``).  Off by
default.

The command loads a ``params.npz`` as ``python -m splatam_amd.run`` writes it; poses come from the map, frames from
``keyframe_time_indices`` when present (otherwise every ``--every``-th), size and intrinsics from ``org_width`` / ``org_height`` /
``intrinsics``.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import sys
from collections import namedtuple

import numpy as np
import torch

from . import _capi

Mesh = namedtuple("Mesh", "vertices faces colors")
Mesh.__doc__ = """``vertices`` [V, 3] float32, ``faces`` [F, 3] int32 (wound with the normal towards free space), ``colors`` [V, 3] float32 in
0..1, on the volume's device."""

MAX_POINTS = 1 << 40                 # (csrc/tsdf_math.h kTsdfMaxPoints)
BRICK_POINTS = 2048                  # (csrc/tsdf_math.h kTsdfBrickPoints)
DEFAULT_MAX_BYTES = 8 << 30
VOLUME_ARRAYS = ("tsdf", "weight", "r", "g", "b")


def volume_bytes(dims):
    """Bytes of a volume's five float32 arrays."""
    nx, ny, nz = (int(d) for d in dims)
    return 20 * nx * ny * nz


def default_bounds(means3D, logit_opacities, pad):
    """((x0, y0, z0), (x1, y1, z1)): the box of ``means3D`` over the rows with sigmoid(logit_opacities) > 0.5, grown by ``pad`` on every
    side.  One host read."""
    keep = logit_opacities.detach().reshape(-1) > 0          # sigmoid(x) > 0.5 <=> x > 0
    pts = means3D.detach()[keep]
    if pts.shape[0] == 0:
        raise ValueError("default bounds: the map has no Gaussian with opacity above 0.5; pass bounds")
    box = torch.stack((pts.min(dim=0).values, pts.max(dim=0).values)).double().cpu().numpy()
    return tuple(float(v) - pad for v in box[0]), tuple(float(v) + pad for v in box[1])


def _beyond_max_bytes(dims, voxel_size, need, max_bytes, bricks=None, advice=True):
    """The ValueError for a volume of ``dims`` grid points (a sparse one with ``bricks`` bricks) that needs ``need`` bytes."""
    nx, ny, nz = dims
    what = f"a {nx} x {ny} x {nz} volume at voxel size {voxel_size}" if bricks is None else \
        f"a sparse {nx} x {ny} x {nz} volume at voxel size {voxel_size} with {bricks} bricks of {BRICK_POINTS} grid points"
    return ValueError(f"{what} needs {need} bytes ({need / 2 ** 30:.2f} GiB), beyond max_bytes = {max_bytes}"
                      + (": raise the voxel size, pass tighter bounds or a larger max_bytes" if advice else ""))


def plan_volume(bounds, voxel_size, max_bytes=DEFAULT_MAX_BYTES, sparse=False):
    """(origin, dims) of the grid that covers ``bounds`` at ``voxel_size``: grid points from the lower corner, one past the upper.
    ValueError, with the size it would need, for a volume beyond ``max_bytes`` (or beyond the library's 2^40 grid points).
    ``sparse``: the grid is a ``SparseTsdfVolume``'s virtual one, whose bytes ``allocate`` checks; only the 2^40 points hold here."""
    lo, hi = (tuple(float(v) for v in b) for b in bounds)
    voxel_size = float(voxel_size)
    if not voxel_size > 0 or len(lo) != 3 or len(hi) != 3 or not all(h > l for l, h in zip(lo, hi)):
        raise ValueError(f"a volume needs a positive voxel size and bounds with a positive extent (got {voxel_size}, {lo} .. {hi})")
    dims = tuple(int(math.ceil((h - l) / voxel_size - 1e-9)) + 1 for l, h in zip(lo, hi))      # (an extent of n voxels is n + 1 points)
    need = volume_bytes(dims)
    if (need > max_bytes and not sparse) or dims[0] * dims[1] * dims[2] >= MAX_POINTS:
        raise _beyond_max_bytes(dims, voxel_size, need, max_bytes)
    return lo, dims


METHODS = ("tetrahedra", "cubes")


def check_method(method):
    """``method`` if it names a surface extractor; ValueError otherwise."""
    if method not in METHODS:
        raise ValueError(f"unknown surface method {method!r}: one of {', '.join(METHODS)}")
    return method


def cubes_table():
    """The library's marching-cubes case table, [256, 16] int8 (include/splat_hip.h splat_tsdf_cubes_table)."""
    table = np.zeros((256, 16), dtype=np.int8)
    _capi.check(_capi.lib().splat_tsdf_cubes_table(table.ctypes.data), "splat_tsdf_cubes_table")
    return table


class _Surface:
    """What ``TsdfVolume`` and ``SparseTsdfVolume`` share: the grid's parameters, the launches, fusing a view and ``extract``.  A volume
    class names its entry points (``_prefix``: ``_launch("reset")`` calls ``splat_tsdf_reset`` or ``splat_tsdf_sparse_reset``), gives
    ``_Surface.__init__`` its C struct and has ``_default_capacity()``."""

    _prefix = None

    def __init__(self, struct, origin, dims, voxel_size, trunc, device):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs a CUDA/HIP device; the HIP library has no CPU path")
        self.origin = tuple(float(v) for v in origin)
        self.dims = tuple(int(d) for d in dims)
        self.voxel_size = float(voxel_size)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        self.struct = struct
        self.L = _capi.lib()
        self.skipped = torch.zeros(1, dtype=torch.int32, device=self.dev)          # ``integrate`` launches a non-zero ``skip`` turned away
        self._keep = None

    def _grid_to_struct(self):
        v = self.struct
        v.nx, v.ny, v.nz = self.dims
        v.origin[:] = self.origin
        v.voxel, v.trunc = self.voxel_size, self.trunc

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _launch(self, name, *args):
        """The entry point ``_prefix + name`` on this volume's struct, ``args`` and the current stream; an error status raises."""
        name = self._prefix + name
        with torch.cuda.device(self.dev):
            _capi.check(getattr(self.L, name)(C.byref(self.struct), *args, self._stream()), name)

    def integrate(self, out6, w2c, intrinsics, sil_thres=0.99, depth_max=0.0, weight_max=0.0, skip=None):
        """One view into the volume (a sparse volume: into every allocated brick, the same arithmetic, the same bits): ``out6``
        [>= 5, H, W] float32 on the device (r, g, b, depth, silhouette as the composite leaves them: depth is sum w z, divided by the
        silhouette here; a view into a larger buffer is fine), ``w2c`` float32 [4, 4] on the device, ``intrinsics`` a 3 x 3 or
        (fx, fy, cx, cy) on the host.  ``skip``: int32 [1] on the device (a ``ViewImage.truncated``); non-zero when the launch runs: the
        volume stays as it is and ``skipped`` counts one.  One launch, nothing read."""
        w, keep = _tsdf_view(out6, w2c, intrinsics, sil_thres, depth_max, weight_max, skip, self.skipped, self.dev)
        self._launch("integrate", C.byref(w))
        self._keep = keep
        return self

    def _render_then(self, step, engine, view, time_idx, w2c, intrinsics, first_w2c, near, far, **kw):
        """``engine.render_view(view, ..., rgb8=False)``, then ``step`` (``integrate`` or ``mark``) of the view's planes at the view's own
        ``w2c`` buffer with its truncation status as ``skip``.  Returns the ``ViewImage``."""
        with torch.no_grad():
            img = engine.render_view(view, w2c=w2c, time_idx=time_idx, intrinsics=intrinsics, first_w2c=first_w2c, near=near, far=far, rgb8=False)
        step(img.out6, view.w2c, intrinsics, skip=img.truncated, **kw)
        return img

    def integrate_view(self, engine, view, time_idx=None, w2c=None, intrinsics=None, first_w2c=None, near=0.01, far=100, **kw):
        """``engine.render_view(view, ..., rgb8=False)`` at a pose of the map (``time_idx``, with ``first_w2c``) or at ``w2c``, then
        ``integrate`` of the view's planes at the view's own ``w2c`` buffer with its truncation status as ``skip``: four launches,
        nothing read on the host.  Returns the ``ViewImage``."""
        return self._render_then(self.integrate, engine, view, time_idx, w2c, intrinsics, first_w2c, near, far, **kw)

    def _triangles(self, min_weight, keys, count, method="tetrahedra"):
        cap = 0 if keys is None else int(keys.shape[0])
        self._launch("cubes" if method == "cubes" else "triangles", float(min_weight), keys.data_ptr() if cap else None, cap, count.data_ptr())

    def _vertices(self, uniq, vertices, colors):
        self._launch("vertices", uniq.data_ptr(), uniq.numel(), vertices.data_ptr(), colors.data_ptr())

    def extract(self, min_weight=1.0, capacity=None, method="tetrahedra"):
        """The zero surface over the cells whose eight corners have ``weight >= min_weight`` as a ``Mesh`` on the device.  One pass over
        the cells into ``capacity`` triangle slots (default: a guess from the grid's size), ONE host read of the count, a second pass
        at the reported size if they did not fit; vertices welded by ``torch.unique`` over their keys, positions and colours by one
        launch.  Canonical: vertices sorted by key, faces lexicographically.

        ``method``: ``"tetrahedra"`` (marching tetrahedra on Kuhn's split: up to 12 triangles a cell, vertices on face and body
        diagonals too) or ``"cubes"`` (marching cubes: at most 5 triangles a cell, vertices on axis edges only -- the subset of the
        tetrahedra's vertices on those edges, bit for bit -- about a third of the triangles).  Anything else: ValueError."""
        check_method(method)
        if capacity is None:
            capacity = self._default_capacity()
        capacity = max(int(capacity), 0)
        count = torch.zeros(1, dtype=torch.int64, device=self.dev)
        keys = torch.empty(capacity, 3, dtype=torch.int64, device=self.dev) if capacity else None
        self._triangles(min_weight, keys, count, method)
        n = int(count.item())
        if n > capacity:
            keys = torch.empty(n, 3, dtype=torch.int64, device=self.dev)
            self._triangles(min_weight, keys, count, method)
        self.last_triangle_count = n
        if n == 0:
            z = torch.zeros(0, 3, dtype=torch.float32, device=self.dev)
            return Mesh(z, torch.zeros(0, 3, dtype=torch.int32, device=self.dev), z.clone())
        uniq, inverse = torch.unique(keys[:n].reshape(-1), return_inverse=True)
        if uniq.numel() >= 2 ** 31:
            raise RuntimeError(f"{uniq.numel()} vertices do not fit int32 faces: extract a smaller volume")
        faces = inverse.view(n, 3)
        for col in (2, 1, 0):                               # lexicographic rows: three stable sorts, last column first
            faces = faces[torch.sort(faces[:, col], stable=True).indices]
        vertices = torch.empty(uniq.numel(), 3, dtype=torch.float32, device=self.dev)
        colors = torch.empty_like(vertices)
        self._vertices(uniq, vertices, colors)
        self.last_keys = uniq
        return Mesh(vertices, faces.to(torch.int32).contiguous(), colors)


def _tsdf_view(out6, w2c, intrinsics, sil_thres, depth_max, weight_max, skip, skipped, dev):
    """(``_capi.SplatTsdfView`` of one view's planes, the tensors it points into)."""
    from .fused import _device_mat4, _intrinsics4
    if not (isinstance(out6, torch.Tensor) and out6.dtype == torch.float32 and out6.device == dev and out6.dim() == 3
            and out6.shape[0] >= 5 and out6.is_contiguous()):
        raise RuntimeError(f"out6 must be a contiguous float32 tensor [>= 5, H, W] on {dev}")
    if skip is not None and not (isinstance(skip, torch.Tensor) and skip.dtype == torch.int32 and skip.device == dev and skip.numel() >= 1):
        raise RuntimeError(f"skip must be an int32 tensor on {dev}")
    keep = [out6, skip]
    w = _capi.SplatTsdfView()
    w.height, w.width = int(out6.shape[1]), int(out6.shape[2])
    w.fx, w.fy, w.cx, w.cy = _intrinsics4(intrinsics)
    w.sil_thres, w.depth_max, w.weight_max = float(sil_thres), float(depth_max), float(weight_max)
    w.out6, w.w2c = out6.data_ptr(), _device_mat4(w2c, "w2c", dev, keep).data_ptr()
    w.skip = skip.data_ptr() if skip is not None else None
    w.skipped = skipped.data_ptr()
    return w, keep


class TsdfVolume(_Surface):
    """A truncated signed distance volume on the device: grid points ``origin + voxel_size (i, j, k)``, ``dims = (nx, ny, nz)`` of them,
    x fastest; ``tsdf``, ``weight``, ``r``, ``g``, ``b`` are [nz, ny, nx] float32 views of one allocation.  Every method enqueues on the
    current stream; only ``extract`` reads (one count)."""

    _prefix = "splat_tsdf_"

    def __init__(self, origin, dims, voxel_size, trunc=None, device="cuda:0"):
        super().__init__(_capi.SplatTsdfVolume(), origin, dims, voxel_size, trunc, device)
        self._grid_to_struct()
        need = int(self.L.splat_tsdf_bytes(C.byref(self.struct)))
        if len(self.origin) != 3 or len(self.dims) != 3 or need == 0:
            raise ValueError(f"a volume needs positive dims (fewer than 2^40 grid points), voxel size and trunc (got {self.dims}, {self.voxel_size}, {self.trunc})")
        nx, ny, nz = self.dims
        self.data = torch.empty(5, nz, ny, nx, dtype=torch.float32, device=self.dev)
        assert self.data.numel() * 4 == need
        self.tsdf, self.weight, self.r, self.g, self.b = self.data.unbind(0)
        v = self.struct
        v.tsdf, v.weight, v.r, v.g, v.b = (t.data_ptr() for t in self.data.unbind(0))
        self.reset()

    def arrays(self):
        return dict(zip(VOLUME_ARRAYS, self.data.unbind(0)))

    def reset(self):
        """tsdf = 1, weight and colours 0, the skipped counter 0."""
        self._launch("reset")
        self.skipped.zero_()
        return self

    def _default_capacity(self):                            # a closed surface crosses O(n^2) of n^3 cells, ~4 triangles each
        nx, ny, nz = self.dims
        return 16 * (nx * ny + ny * nz + nz * nx) + 4096


def brick_shapes():
    """The brick shapes the library accepts, each (x, y, z) grid points; the first is the default."""
    L = _capi.lib()
    shape = (C.c_int32 * 3)()
    return [tuple(shape) for n in range(L.splat_tsdf_sparse_brick_shape(0, shape)) if L.splat_tsdf_sparse_brick_shape(n, shape)]


class SparseTsdfVolume(_Surface):
    """``TsdfVolume``'s grid, of which only BRICKS near observed surfaces are stored (csrc/tsdf_sparse.hip): a brick is 2048 grid points
    (``brick`` = its shape, default ``brick_shapes()[0]``), 8 KiB per array in a pool; ``directory`` (int32, one entry per brick of the
    grid, x fastest) holds a brick's slot in the pool or -1, ``brick_of_slot`` the reverse.  ``dims`` may be far beyond what a dense
    volume could hold: memory follows the surfaces, not the box.

    The order that gives the dense volume's mesh BIT FOR BIT: ``mark`` every view, ``allocate`` once, ``integrate`` every view,
    ``extract`` (``extract_mesh(..., sparse=True)`` does that).  ``mark`` flags every brick that meets the 3 x 3 x 3 neighbourhood of a
    grid point the view can update with a negative value -- every cell that can emit a triangle has its eight corners there -- and a
    brick that then receives every view holds the dense volume's bits.  ``allocate`` may also be called again and again (mark,
    allocate, integrate view by view: the pool grows); a brick allocated late has missed the earlier views' free-space updates, so the
    result may then differ from the dense one.

    Every method enqueues on the current stream; ``marked_count`` and ``extract`` read one number each.  ``capacity_bricks``: room in
    the pool from the start (it grows by reallocation otherwise)."""

    _prefix = "splat_tsdf_sparse_"

    def __init__(self, origin, dims, voxel_size, trunc=None, capacity_bricks=0, device="cuda:0", brick=None):
        super().__init__(_capi.SplatTsdfSparse(), origin, dims, voxel_size, trunc, device)
        self.brick = tuple(int(b) for b in (brick or brick_shapes()[0]))
        if len(self.origin) != 3 or len(self.dims) != 3 or len(self.brick) != 3:
            raise ValueError(f"a volume needs three dims, an origin and a brick shape (got {self.dims}, {self.origin}, {self.brick})")
        self._grid_to_struct()
        v = self.struct
        v.brick[:] = self.brick
        v.slots = 0
        if int(self.L.splat_tsdf_sparse_bytes(C.byref(v))) == 0:
            raise ValueError(f"a sparse volume needs positive dims (fewer than 2^40 grid points, 2^31 bricks), voxel size and trunc and a brick shape "
                             f"of {brick_shapes()} (got {self.dims}, {self.voxel_size}, {self.trunc}, {self.brick})")
        self.bricks_per_axis = tuple(-(-d // b) for d, b in zip(self.dims, self.brick))
        self.num_bricks = self.bricks_per_axis[0] * self.bricks_per_axis[1] * self.bricks_per_axis[2]
        self.directory = torch.full((self.num_bricks,), -1, dtype=torch.int32, device=self.dev)
        self.flags = torch.zeros(self.num_bricks, dtype=torch.int32, device=self.dev)
        self.slots = 0
        self.pool = self.brick_of_slot = None
        self._capacity = 0
        self.mark_skipped = torch.zeros(1, dtype=torch.int32, device=self.dev)     # ``mark`` launches a non-zero ``skip`` turned away
        v.directory = self.directory.data_ptr()
        if capacity_bricks:
            self._reserve(int(capacity_bricks))

    def _bind(self):
        v = self.struct
        v.slots = self.slots
        v.directory = self.directory.data_ptr()
        if self.pool is not None:
            v.brick_of_slot = self.brick_of_slot.data_ptr()
            v.tsdf, v.weight, v.r, v.g, v.b = (t.data_ptr() for t in self.pool.unbind(0))

    def _reserve(self, capacity):
        """Room for ``capacity`` bricks in the pool; what is there is kept."""
        if capacity <= self._capacity:
            return
        pool = torch.empty(5, capacity, BRICK_POINTS, dtype=torch.float32, device=self.dev)
        table = torch.empty(capacity + 1, dtype=torch.int32, device=self.dev)      # (one entry more: where ``allocate`` drops the bricks it skips)
        if self.slots:
            pool[:, :self.slots].copy_(self.pool[:, :self.slots])
            table[:self.slots].copy_(self.brick_of_slot[:self.slots])
        self.pool, self.brick_of_slot, self._capacity = pool, table, capacity
        self._bind()

    def bytes_for(self, slots):
        """Device bytes of this volume with ``slots`` bricks in the pool: the pool, ``brick_of_slot``, the directory and the flags."""
        return (20 * BRICK_POINTS + 4) * int(slots) + 8 * self.num_bricks

    def bytes(self):
        return self.bytes_for(self.slots)

    def arrays(self):
        """tsdf, weight, r, g, b of the pool: each [slots, 2048]."""
        if self.pool is None:
            return {k: torch.zeros(0, BRICK_POINTS, device=self.dev) for k in VOLUME_ARRAYS}
        return dict(zip(VOLUME_ARRAYS, self.pool[:, :self.slots].unbind(0)))

    def mark(self, out6, w2c, intrinsics, sil_thres=0.99, depth_max=0.0, skip=None):
        """Flags the bricks one view needs (``integrate``'s arguments; ``weight_max`` plays no part).  A non-zero ``skip`` leaves the
        flags as they are and ``mark_skipped`` counts one.  One launch, nothing read."""
        w, keep = _tsdf_view(out6, w2c, intrinsics, sil_thres, depth_max, 0.0, skip, self.mark_skipped, self.dev)
        self._launch("mark", C.byref(w), self.flags.data_ptr())
        self._keep = keep
        return self

    def mark_view(self, engine, view, time_idx=None, w2c=None, intrinsics=None, first_w2c=None, near=0.01, far=100, weight_max=0.0, **kw):
        """``integrate_view`` with ``mark`` in place of ``integrate``.  Returns the ``ViewImage``."""
        return self._render_then(self.mark, engine, view, time_idx, w2c, intrinsics, first_w2c, near, far, **kw)

    def _new(self):
        return (self.flags != 0) & (self.directory < 0)

    def marked_count_tensor(self):
        """int64 [1] on the device: marked bricks that have no slot yet."""
        return self._new().sum().reshape(1)

    def marked_count(self):
        """Marked bricks that have no slot yet.  One host read."""
        return int(self.marked_count_tensor().item())

    def allocate(self, max_bytes=DEFAULT_MAX_BYTES, count=None):
        """Slots for the marked bricks that have none, in brick order, reset to tsdf = 1, weight = r = g = b = 0.  ``count``: their
        number when the caller has read it already (``marked_count()`` otherwise: the one read).  ValueError, with the bytes it would
        need, when the volume would grow beyond ``max_bytes``.  Returns the number of new slots."""
        count = self.marked_count() if count is None else int(count)
        total = self.slots + count
        need = self.bytes_for(total)
        if need > max_bytes or total >= 2 ** 31:
            raise _beyond_max_bytes(self.dims, self.voxel_size, need, max_bytes, bricks=total)
        if count == 0:
            return 0
        self._reserve(max(total, self._capacity))
        new = self._new()
        slot = (self.slots - 1 + torch.cumsum(new, 0)).to(torch.int32)             # (of the new bricks; deterministic: brick order)
        self.directory.copy_(torch.where(new, slot, self.directory))
        # brick_of_slot without a host read: every brick writes its number at its new slot, the others into the spare last entry
        where = torch.where(new, slot.long(), torch.full_like(slot, self._capacity, dtype=torch.int64))
        self.brick_of_slot.scatter_(0, where, torch.arange(self.num_bricks, dtype=torch.int32, device=self.dev))
        first, self.slots = self.slots, total
        self._bind()
        self._launch("reset_slots", first, count)
        return count

    def _default_capacity(self):                            # the band is several bricks thick and the surface crosses some of them
        return 768 * self.slots + 4096

    def point_offsets(self):
        """int64 [nz, ny, nx]: every grid point's offset in the pool's arrays (slot 2048 + local), -1 where its brick is not allocated.
        For tests and small volumes."""
        bx, by, bz = self.brick
        i, j, k = (torch.arange(d, device=self.dev) for d in self.dims)
        brick = ((k // bz)[:, None, None] * self.bricks_per_axis[1] + (j // by)[None, :, None]) * self.bricks_per_axis[0] + (i // bx)[None, None, :]
        local = ((k % bz)[:, None, None] * by + (j % by)[None, :, None]) * bx + (i % bx)[None, None, :]
        slot = self.directory[brick].long()
        return torch.where(slot >= 0, slot * BRICK_POINTS + local, torch.full_like(slot, -1))

    def to_dense(self, max_bytes=DEFAULT_MAX_BYTES):
        """A ``TsdfVolume`` of the same grid with this volume's values, the reset values where no brick is allocated.  For tests and
        small volumes: ValueError beyond ``max_bytes``, like ``plan_volume``."""
        need = volume_bytes(self.dims)
        if need > max_bytes:
            raise _beyond_max_bytes(self.dims, self.voxel_size, need, max_bytes, advice=False)
        dense = TsdfVolume(self.origin, self.dims, self.voxel_size, self.trunc, self.dev)
        if self.slots:
            at = self.point_offsets()
            have = at >= 0
            flat = self.pool.view(5, -1)
            for n, t in enumerate(dense.data.unbind(0)):
                t[have] = flat[n][at[have]]
        return dense


def _views_pass(frames, run, skipped, view, extra=None):
    """``run(frame)`` (a render and what follows it; returns the ``ViewImage``) for every frame, each view's truncation status kept in a
    device table that is read ONCE at the end, with the ``skipped`` counter and ``extra`` (an int64 [1] tensor made after the loop, or
    None) behind it; the views whose lists did not fit -- turned away on the device -- then get ``view.check_overflow()`` and go
    again (``map_pass.run_pass``).  Returns (the frames repeated, ``extra``'s value or None)."""
    from .map_pass import fit_lists, run_pass
    table = torch.zeros(len(frames) + 2, dtype=torch.int64, device=skipped.device)       # a flag per frame, the skipped counter, ``extra``
    host = []

    def read():
        table[len(frames):len(frames) + 1].copy_(skipped)
        if extra is not None:
            table[len(frames) + 1:].copy_(extra())
        host[:] = table.cpu().tolist()                      # the one read
        flagged = [n for n in range(len(frames)) if host[n]]
        if host[len(frames)] != len(flagged):
            raise RuntimeError(f"{host[len(frames)]} views were turned away on the device but {len(flagged)} are flagged")
        if flagged:
            view.check_overflow()                           # (digests the latest render; clears the camera's status either way)
        return flagged

    repeated = run_pass(frames, lambda n, fr: table[n:n + 1].copy_(run(fr).truncated), read,
                        lambda n, fr: fit_lists(lambda: run(fr), view.check_overflow,   # (True: the lists are grown, the view goes again)
                                                f"frame {fr}: the per-tile lists could not be sized for its view"))
    return repeated, (host[-1] if extra is not None else None)


def extract_mesh(engine, frames, size, intrinsics, voxel_size=0.01, trunc=None, bounds=None, max_bytes=DEFAULT_MAX_BYTES, sil_thres=0.99,
                 depth_max=0.0, weight_max=0.0, min_weight=1.0, first_w2c=None, view=None, return_volume=False, sparse=False, method="tetrahedra", clean=None):
    """A ``Mesh`` of ``engine``'s map from renders at ``frames``: each a time index of the map (seen through ``first_w2c``, default the
    identity) or a float32 [4, 4] ``w2c`` on the device.  ``size`` = (width, height) of the renders, ``intrinsics`` theirs (host).
    ``bounds`` = ((x0, y0, z0), (x1, y1, z1)); default ``default_bounds`` of the map padded by ``trunc + voxel_size`` (one host read).
    A volume beyond ``max_bytes`` is refused with the size it would need (ValueError).

    One view camera (``view``, or a new one) moves from pose to pose; every frame is enqueued -- render, integrate, its truncation
    status kept in a device table -- and the table is read ONCE at the end.  Views whose lists did not fit were turned away on the
    device; they get ``view.check_overflow()`` and are integrated again.  The map, its Adam state, ``variables`` and the current camera
    are left as they were (``render_view``'s contract).  Between iterations, like every view render.

    ``sparse=True``: the same mesh, bit for bit, from a ``SparseTsdfVolume``, whose memory follows the surfaces instead of the box --
    ``max_bytes`` then bounds its pool and tables, and a box far beyond what a dense volume could hold is fine.  Two passes over the
    frames: render + ``mark`` (one read: the table, with the number of bricks marked), ``allocate``, then render + ``integrate`` as
    above.  A render costs less than the dense volume's integration of it.

    ``method``: the surface extractor, ``"tetrahedra"`` (default) or ``"cubes"`` (``_Surface.extract``): marching cubes gives a third
    of the triangles and a third to a half of the vertices of the same surface, which everything downstream -- scoring, culling, alignment, cleaning,
    the PLY -- then carries.  Dense and sparse volumes alike; an unknown name is a ValueError before anything is launched.

    ``clean`` (True, or a dict of ``mesh_clean.clean_mesh`` keywords): the mesh is ``clean_mesh`` of what was extracted -- its small
    connected components are removed on the device, with one more host read.  ``None``: the mesh as extracted."""
    from .mesh_clean import clean_options
    check_method(method)
    clean = clean_options(clean)
    trunc = 4.0 * float(voxel_size) if trunc is None else float(trunc)
    if bounds is None:
        bounds = default_bounds(engine.params['means3D'][:engine.P], engine.params['logit_opacities'][:engine.P], trunc + float(voxel_size))
    origin, dims = plan_volume(bounds, voxel_size, max_bytes, sparse=sparse)
    frames = list(frames)
    W, H = int(size[0]), int(size[1])
    if view is None:
        view = engine.view_camera(W, H)
    elif (view.W, view.H) != (W, H):
        raise ValueError(f"the view camera is {view.W} x {view.H}, not {W} x {H}")
    volume = (SparseTsdfVolume if sparse else TsdfVolume)(origin, dims, voxel_size, trunc, device=engine.dev)
    kw = dict(intrinsics=intrinsics, sil_thres=sil_thres, depth_max=depth_max, weight_max=weight_max)

    def pose(fr):
        return dict(w2c=fr) if isinstance(fr, torch.Tensor) else dict(time_idx=int(fr), first_w2c=first_w2c)

    if sparse:
        volume.repeated_marks, count = _views_pass(frames, lambda fr: volume.mark_view(engine, view, **pose(fr), **kw), volume.mark_skipped, view,
                                                   extra=volume.marked_count_tensor)
        volume.allocate(max_bytes, count=None if volume.repeated_marks else count)      # (views marked again: the count is read again)
    volume.repeated, _ = _views_pass(frames, lambda fr: volume.integrate_view(engine, view, **pose(fr), **kw), volume.skipped, view)
    mesh = _cleaned(volume.extract(min_weight, method=method), clean, engine.dev)
    return (mesh, volume) if return_volume else mesh


def _cleaned(mesh, clean, device, cleaning=None):
    """``mesh`` as ``clean`` (what ``clean_options`` returned) asks for it: as it is (None), or ``clean_mesh`` of it with those
    keywords; ``cleaning``, a dict, then receives the report."""
    if clean is None:
        return mesh
    from .mesh_clean import clean_mesh
    mesh, found = clean_mesh(mesh, device=device, report=True, **clean)
    if cleaning is not None:
        cleaning.update(found)
    return mesh


def mesh_from_params(path, out, voxel_size=0.01, trunc=None, every=5, size=None, sil_thres=0.99, depth_max=0.0, bounds=None,
                     max_bytes=DEFAULT_MAX_BYTES, device="cuda:0", verbose=True, sparse=False, clean=None, cleaning=None, method="tetrahedra", views=None,
                     views_mode="shaded", simplify=None, simplification=None):
    """``extract_mesh`` of a ``params.npz`` written to ``out`` (a PLY); returns the ``Mesh``.  ``method``: ``extract_mesh``'s.  ``clean`` (True or a dict of
    ``mesh_clean.clean_mesh`` keywords): the mesh is cleaned before it is written; ``cleaning``, a dict, then receives the report.
    ``simplify`` (a cell size in metres, or a dict of ``mesh_simplify.simplify_mesh`` keywords that names ``cell``): the mesh is simplified
    -- after the cleaning, so that no floater is merged into the surface it floats over, and before it is written and pictured;
    ``simplification``, a dict, then receives the report.
    ``views`` (a directory): pictures ``mesh_%04d.png`` of the mesh that was written, in ``views_mode``, at every ``every``-th estimated
    pose of the run (``mesh_view.render_trajectory``)."""
    from . import slam
    from .export import save_mesh_ply
    from .fused import FusedEngine
    from .mesh_clean import clean_options, format_cleaning
    from .mesh_simplify import _simplified, format_simplification, simplify_options
    from .view import _scaled_intrinsics, load_map
    check_method(method)
    clean = clean_options(clean)
    found = {} if cleaning is None else cleaning
    simplify = simplify_options(simplify)
    simplified = {} if simplification is None else simplification
    dev = torch.device(device)
    params, variables, k, first_w2c, (W0, H0), more = load_map(path, dev, extras=("keyframe_time_indices",))
    keyframes = [int(t) for t in more["keyframe_time_indices"]] if more["keyframe_time_indices"] is not None else []
    W, H = size or (W0, H0)
    intrinsics = _scaled_intrinsics(k, (W, H), (W0, H0))
    with torch.no_grad():
        cam = slam.setup_camera(W0, H0, k, first_w2c.cpu().numpy(), device=dev)
        engine = FusedEngine(params, cam, variables=variables)
        frames = keyframes or list(range(0, engine.num_frames, max(int(every), 1)))
        mesh = extract_mesh(engine, frames, (W, H), intrinsics, voxel_size=voxel_size, trunc=trunc, bounds=bounds, max_bytes=max_bytes,
                            sil_thres=sil_thres, depth_max=depth_max, first_w2c=first_w2c.contiguous(), sparse=sparse, method=method)
        mesh = _cleaned(mesh, clean, dev, found)            # (not through extract_mesh: the report is wanted)
        mesh = _simplified(mesh, simplify, dev, simplified)
    save_mesh_ply(out, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.colors.cpu().numpy())
    if verbose:
        print(f"{out}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces from {len(frames)} views", flush=True)
        if clean is not None:
            print(format_cleaning(found), flush=True)
        if simplify is not None:
            print(format_simplification(simplified), flush=True)
    if views is not None:
        from . import mesh_view
        poses, _, _ = mesh_view.params_poses(path)
        written = mesh_view.render_trajectory(mesh, poses, views, intrinsics, (W, H), every=max(int(every), 1), device=dev, mode=views_mode)
        if verbose:
            print(f"{views}: {len(written)} pictures of the mesh ({views_mode})", flush=True)
    return mesh


def _parser():
    from .view import _size
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.mesh", description=__doc__.split("\n\n")[0])
    parser.add_argument("params", help="params.npz of a run")
    parser.add_argument("--out", required=True, help="the PLY to write")
    parser.add_argument("--voxel", type=float, default=0.01, help="voxel size in metres")
    parser.add_argument("--trunc", type=float, default=None, help="truncation distance in metres (default 4 voxels)")
    parser.add_argument("--every", type=int, default=5, help="every N-th pose, for a map without keyframe_time_indices")
    parser.add_argument("--size", type=_size, default=None, help="WIDTHxHEIGHT of the renders (default: the run's frame size)")
    parser.add_argument("--sil-thres", type=float, default=0.99, help="pixels with a silhouette at or below this are not fused")
    parser.add_argument("--depth-max", type=float, default=0.0, help="depth beyond this is not fused (0: no limit)")
    parser.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                        help="the volume's box in metres (default: the opaque Gaussians' box)")
    parser.add_argument("--max-bytes", type=int, default=DEFAULT_MAX_BYTES)
    parser.add_argument("--sparse", action="store_true", help="a sparse volume: the same mesh, memory only near surfaces (for boxes a dense volume cannot hold)")
    parser.add_argument("--method", choices=METHODS, default="tetrahedra",
                        help="the surface extractor: marching tetrahedra, or marching cubes (about a third of the triangles)")
    parser.add_argument("--clean", action="store_true", help="remove the mesh's small connected components before it is written")
    parser.add_argument("--min-vertices", type=int, default=None, metavar="N", help="with --clean: components with fewer vertices go (200)")
    parser.add_argument("--min-area", type=float, default=None, metavar="M2", help="with --clean: components with less area in m^2 go (0)")
    parser.add_argument("--keep-largest", type=int, default=None, metavar="K", help="with --clean: keep at most the K components with the most faces")
    parser.add_argument("--simplify", type=float, default=None, metavar="CELL",
                        help="merge the vertices in each cell of a grid of this edge (metres) before the mesh is written (python -m splatam_amd.mesh_simplify)")
    parser.add_argument("--simplify-placement", default=None, choices=("quadric", "mean"), help="with --simplify: where a cell's vertex sits (quadric)")
    parser.add_argument("--views", default=None, metavar="DIR",
                        help="also write pictures mesh_%%04d.png of the mesh at every --every-th estimated pose (python -m splatam_amd.mesh_view)")
    parser.add_argument("--views-mode", default=None, choices=("shaded", "shaded-color", "color", "normal", "depth"), help="with --views (default shaded)")
    parser.add_argument("--device", default="cuda:0")
    return parser


def main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    options = {k: v for k, v in (("min_vertices", args.min_vertices), ("min_area", args.min_area), ("keep_largest", args.keep_largest)) if v is not None}
    if options and not args.clean:
        parser.error("--min-vertices, --min-area and --keep-largest need --clean")
    if args.views_mode and not args.views:
        parser.error("--views-mode needs --views")
    if args.simplify_placement and args.simplify is None:
        parser.error("--simplify-placement needs --simplify")
    simplify = {} if args.simplify is None else {"simplify": dict(cell=args.simplify, **({"placement": args.simplify_placement} if args.simplify_placement else {}))}
    bounds = (args.bounds[:3], args.bounds[3:]) if args.bounds else None
    try:
        mesh_from_params(args.params, args.out, voxel_size=args.voxel, trunc=args.trunc, every=args.every, size=args.size,
                         sil_thres=args.sil_thres, depth_max=args.depth_max, bounds=bounds, max_bytes=args.max_bytes, device=args.device,
                         sparse=args.sparse, method=args.method, **({"clean": options or True} if args.clean else {}),
                         **({"views": args.views, "views_mode": args.views_mode or "shaded"} if args.views else {}), **simplify)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
