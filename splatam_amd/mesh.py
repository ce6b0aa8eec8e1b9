"""A triangle mesh of the map: ``python -m splatam_amd.mesh PARAMS.npz --out mesh.ply [--voxel M] [--trunc M] [--every N] [--size WxH]
[--sil-thres S] [--depth-max M] [--bounds X0 Y0 Z0 X1 Y1 Z1]``.

Depth rendered at the estimated poses is fused into a truncated signed distance volume and the volume's zero surface is extracted,
all on the device (csrc/tsdf.hip, arithmetic in csrc/tsdf_math.h): the usual deliverable of a dense RGB-D SLAM system, and what the
methods SplaTAM is compared with are scored on.  ``FusedEngine.render_view(..., rgb8=False)`` leaves a view's six planes and its
``w2c`` in device buffers; ``TsdfVolume.integrate`` takes them from there, gated on the device by the view's truncation status.

The surface is marching tetrahedra on Kuhn's split of every cell (six tetrahedra, translation invariant, so neighbouring cells agree
on their shared faces and the mesh is closed wherever the volume was seen); vertices are named by the grid edge they lie on, so
welding is a ``torch.unique`` over integer keys and the result is canonical: vertices sorted by key, faces lexicographically -- the
same volume always gives the same bytes.

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


def plan_volume(bounds, voxel_size, max_bytes=DEFAULT_MAX_BYTES):
    """(origin, dims) of the grid that covers ``bounds`` at ``voxel_size``: grid points from the lower corner, one past the upper.
    ValueError, with the size it would need, for a volume beyond ``max_bytes`` (or beyond the library's 2^40 grid points)."""
    lo, hi = (tuple(float(v) for v in b) for b in bounds)
    voxel_size = float(voxel_size)
    if not voxel_size > 0 or len(lo) != 3 or len(hi) != 3 or not all(h > l for l, h in zip(lo, hi)):
        raise ValueError(f"a volume needs a positive voxel size and bounds with a positive extent (got {voxel_size}, {lo} .. {hi})")
    dims = tuple(int(math.ceil((h - l) / voxel_size - 1e-9)) + 1 for l, h in zip(lo, hi))      # (an extent of n voxels is n + 1 points)
    need = volume_bytes(dims)
    if need > max_bytes or dims[0] * dims[1] * dims[2] >= MAX_POINTS:
        raise ValueError(f"a {dims[0]} x {dims[1]} x {dims[2]} volume at voxel size {voxel_size} needs {need} bytes ({need / 2 ** 30:.2f} GiB), "
                         f"beyond max_bytes = {max_bytes}: raise the voxel size, pass tighter bounds or a larger max_bytes")
    return lo, dims


class TsdfVolume:
    """A truncated signed distance volume on the device: grid points ``origin + voxel_size (i, j, k)``, ``dims = (nx, ny, nz)`` of them,
    x fastest; ``tsdf``, ``weight``, ``r``, ``g``, ``b`` are [nz, ny, nx] float32 views of one allocation.  Every method enqueues on the
    current stream; only ``extract`` reads (one count)."""

    def __init__(self, origin, dims, voxel_size, trunc=None, device="cuda:0"):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("TsdfVolume needs a CUDA/HIP device; the HIP library has no CPU path")
        self.origin = tuple(float(v) for v in origin)
        self.dims = tuple(int(d) for d in dims)
        self.voxel_size = float(voxel_size)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        v = self.struct = _capi.SplatTsdfVolume()
        v.nx, v.ny, v.nz = self.dims
        v.origin[:] = self.origin
        v.voxel, v.trunc = self.voxel_size, self.trunc
        self.L = _capi.lib()
        need = int(self.L.splat_tsdf_bytes(C.byref(v)))
        if len(self.origin) != 3 or len(self.dims) != 3 or need == 0:
            raise ValueError(f"a volume needs positive dims (fewer than 2^40 grid points), voxel size and trunc (got {self.dims}, {self.voxel_size}, {self.trunc})")
        nx, ny, nz = self.dims
        self.data = torch.empty(5, nz, ny, nx, dtype=torch.float32, device=self.dev)
        assert self.data.numel() * 4 == need
        self.tsdf, self.weight, self.r, self.g, self.b = self.data.unbind(0)
        v.tsdf, v.weight, v.r, v.g, v.b = (t.data_ptr() for t in self.data.unbind(0))
        self.skipped = torch.zeros(1, dtype=torch.int32, device=self.dev)          # launches a non-zero ``skip`` turned away
        self._keep = None
        self.reset()

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def arrays(self):
        return dict(zip(VOLUME_ARRAYS, self.data.unbind(0)))

    def reset(self):
        """tsdf = 1, weight and colours 0, the skipped counter 0."""
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_tsdf_reset(C.byref(self.struct), self._stream()), "splat_tsdf_reset")
        self.skipped.zero_()
        return self

    def integrate(self, out6, w2c, intrinsics, sil_thres=0.99, depth_max=0.0, weight_max=0.0, skip=None):
        """One view into the volume: ``out6`` [>= 5, H, W] float32 on the device (r, g, b, depth, silhouette as the composite leaves
        them: depth is sum w z, divided by the silhouette here; a view into a larger buffer is fine), ``w2c`` float32 [4, 4] on the
        device, ``intrinsics`` a 3 x 3 or (fx, fy, cx, cy) on the host.  ``skip``: int32 [1] on the device (a ``ViewImage.truncated``);
        non-zero when the launch runs: the volume stays as it is and ``skipped`` counts one.  One launch, nothing read."""
        from .fused import _device_mat4, _intrinsics4
        if not (isinstance(out6, torch.Tensor) and out6.dtype == torch.float32 and out6.device == self.dev and out6.dim() == 3
                and out6.shape[0] >= 5 and out6.is_contiguous()):
            raise RuntimeError(f"out6 must be a contiguous float32 tensor [>= 5, H, W] on {self.dev}")
        if skip is not None and not (isinstance(skip, torch.Tensor) and skip.dtype == torch.int32 and skip.device == self.dev and skip.numel() >= 1):
            raise RuntimeError(f"skip must be an int32 tensor on {self.dev}")
        keep = [out6, skip]
        w = _capi.SplatTsdfView()
        w.height, w.width = int(out6.shape[1]), int(out6.shape[2])
        w.fx, w.fy, w.cx, w.cy = _intrinsics4(intrinsics)
        w.sil_thres, w.depth_max, w.weight_max = float(sil_thres), float(depth_max), float(weight_max)
        w.out6, w.w2c = out6.data_ptr(), _device_mat4(w2c, "w2c", self.dev, keep).data_ptr()
        w.skip = skip.data_ptr() if skip is not None else None
        w.skipped = self.skipped.data_ptr()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_tsdf_integrate(C.byref(self.struct), C.byref(w), self._stream()), "splat_tsdf_integrate")
        self._keep = keep
        return self

    def integrate_view(self, engine, view, time_idx=None, w2c=None, intrinsics=None, first_w2c=None, near=0.01, far=100, **kw):
        """``engine.render_view(view, ..., rgb8=False)`` at a pose of the map (``time_idx``, with ``first_w2c``) or at ``w2c``, then
        ``integrate`` of the view's planes at the view's own ``w2c`` buffer with its truncation status as ``skip``: four launches,
        nothing read on the host.  Returns the ``ViewImage``."""
        with torch.no_grad():
            img = engine.render_view(view, w2c=w2c, time_idx=time_idx, intrinsics=intrinsics, first_w2c=first_w2c, near=near, far=far, rgb8=False)
        self.integrate(img.out6, view.w2c, intrinsics, skip=img.truncated, **kw)
        return img

    def _triangles(self, min_weight, keys, count):
        cap = 0 if keys is None else int(keys.shape[0])
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_tsdf_triangles(C.byref(self.struct), float(min_weight), keys.data_ptr() if cap else None, cap,
                                                    count.data_ptr(), self._stream()), "splat_tsdf_triangles")

    def extract(self, min_weight=1.0, capacity=None):
        """The zero surface over the cells whose eight corners have ``weight >= min_weight`` as a ``Mesh`` on the device.  One pass over
        the cells into ``capacity`` triangle slots (default: a guess from the grid's size), ONE host read of the count, a second pass
        at the reported size if they did not fit; vertices welded by ``torch.unique`` over their keys, positions and colours by one
        launch.  Canonical: vertices sorted by key, faces lexicographically."""
        nx, ny, nz = self.dims
        if capacity is None:                                # a closed surface crosses O(n^2) of n^3 cells, ~4 triangles each
            capacity = 16 * (nx * ny + ny * nz + nz * nx) + 4096
        capacity = max(int(capacity), 0)
        count = torch.zeros(1, dtype=torch.int64, device=self.dev)
        keys = torch.empty(capacity, 3, dtype=torch.int64, device=self.dev) if capacity else None
        self._triangles(min_weight, keys, count)
        n = int(count.item())
        if n > capacity:
            keys = torch.empty(n, 3, dtype=torch.int64, device=self.dev)
            self._triangles(min_weight, keys, count)
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
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_tsdf_vertices(C.byref(self.struct), uniq.data_ptr(), uniq.numel(), vertices.data_ptr(), colors.data_ptr(),
                                                   self._stream()), "splat_tsdf_vertices")
        self.last_keys = uniq
        return Mesh(vertices, faces.to(torch.int32).contiguous(), colors)


def _scaled_intrinsics(intrinsics, size, org_size):
    from .fused import _intrinsics4
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    sx, sy = size[0] / org_size[0], size[1] / org_size[1]
    return fx * sx, fy * sy, cx * sx, cy * sy


def extract_mesh(engine, frames, size, intrinsics, voxel_size=0.01, trunc=None, bounds=None, max_bytes=DEFAULT_MAX_BYTES, sil_thres=0.99,
                 depth_max=0.0, weight_max=0.0, min_weight=1.0, first_w2c=None, view=None, return_volume=False):
    """A ``Mesh`` of ``engine``'s map from renders at ``frames``: each a time index of the map (seen through ``first_w2c``, default the
    identity) or a float32 [4, 4] ``w2c`` on the device.  ``size`` = (width, height) of the renders, ``intrinsics`` theirs (host).
    ``bounds`` = ((x0, y0, z0), (x1, y1, z1)); default ``default_bounds`` of the map padded by ``trunc + voxel_size`` (one host read).
    A volume beyond ``max_bytes`` is refused with the size it would need (ValueError).

    One view camera (``view``, or a new one) moves from pose to pose; every frame is enqueued -- render, integrate, its truncation
    status kept in a device table -- and the table is read ONCE at the end.  Views whose lists did not fit were turned away on the
    device; they get ``view.check_overflow()`` and are integrated again.  The map, its Adam state, ``variables`` and the current camera
    are left as they were (``render_view``'s contract).  Between iterations, like every view render."""
    trunc = 4.0 * float(voxel_size) if trunc is None else float(trunc)
    if bounds is None:
        bounds = default_bounds(engine.params['means3D'][:engine.P], engine.params['logit_opacities'][:engine.P], trunc + float(voxel_size))
    origin, dims = plan_volume(bounds, voxel_size, max_bytes)
    frames = list(frames)
    W, H = int(size[0]), int(size[1])
    if view is None:
        view = engine.view_camera(W, H)
    elif (view.W, view.H) != (W, H):
        raise ValueError(f"the view camera is {view.W} x {view.H}, not {W} x {H}")
    volume = TsdfVolume(origin, dims, voxel_size, trunc, engine.dev)
    kw = dict(intrinsics=intrinsics, sil_thres=sil_thres, depth_max=depth_max, weight_max=weight_max)

    def pose(fr):
        return dict(w2c=fr) if isinstance(fr, torch.Tensor) else dict(time_idx=int(fr), first_w2c=first_w2c)

    table = torch.zeros(len(frames) + 1, dtype=torch.int32, device=engine.dev)          # a flag per frame, then the skipped counter
    for n, fr in enumerate(frames):
        img = volume.integrate_view(engine, view, **pose(fr), **kw)
        table[n:n + 1].copy_(img.truncated)
    table[len(frames):].copy_(volume.skipped)
    table = table.cpu().tolist()                            # the one read
    flagged = [n for n in range(len(frames)) if table[n]]
    if table[-1] != len(flagged):
        raise RuntimeError(f"{table[-1]} views were turned away on the device but {len(flagged)} are flagged")
    if flagged:
        view.check_overflow()                               # (digests the latest render; clears the camera's status either way)
    for n in flagged:
        for _ in range(3):
            volume.integrate_view(engine, view, **pose(frames[n]), **kw)
            if not view.check_overflow():                   # (True: the lists are grown, the view goes again)
                break
        else:
            raise RuntimeError(f"frame {frames[n]}: the per-tile lists could not be sized for its view")
    volume.repeated = [frames[n] for n in flagged]
    mesh = volume.extract(min_weight)
    return (mesh, volume) if return_volume else mesh


def mesh_from_params(path, out, voxel_size=0.01, trunc=None, every=5, size=None, sil_thres=0.99, depth_max=0.0, bounds=None,
                     max_bytes=DEFAULT_MAX_BYTES, device="cuda:0", verbose=True):
    """``extract_mesh`` of a ``params.npz`` written to ``out`` (a PLY); returns the ``Mesh``."""
    from . import slam
    from .export import save_mesh_ply
    from .fused import FusedEngine
    from .view import load_map
    dev = torch.device(device)
    params, variables, k, first_w2c, (W0, H0) = load_map(path, dev)
    with np.load(path) as z:
        keyframes = [int(t) for t in z['keyframe_time_indices']] if 'keyframe_time_indices' in z else []
    W, H = size or (W0, H0)
    with torch.no_grad():
        cam = slam.setup_camera(W0, H0, k, first_w2c.cpu().numpy(), device=dev)
        engine = FusedEngine(params, cam, variables=variables)
        frames = keyframes or list(range(0, engine.num_frames, max(int(every), 1)))
        mesh = extract_mesh(engine, frames, (W, H), _scaled_intrinsics(k, (W, H), (W0, H0)), voxel_size=voxel_size, trunc=trunc, bounds=bounds,
                            max_bytes=max_bytes, sil_thres=sil_thres, depth_max=depth_max, first_w2c=first_w2c.contiguous())
    save_mesh_ply(out, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.colors.cpu().numpy())
    if verbose:
        print(f"{out}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces from {len(frames)} views", flush=True)
    return mesh


def main(argv=None):
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
    parser.add_argument("--device", default="cuda:0")
    args = parser.parse_args(argv)
    bounds = (args.bounds[:3], args.bounds[3:]) if args.bounds else None
    try:
        mesh_from_params(args.params, args.out, voxel_size=args.voxel, trunc=args.trunc, every=args.every, size=args.size,
                         sil_thres=args.sil_thres, depth_max=args.depth_max, bounds=bounds, max_bytes=args.max_bytes, device=args.device)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
