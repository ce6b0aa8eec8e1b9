"""Picture a mesh: ``python -m splatam_amd.mesh_view MESH.ply --out DIR (--poses traj.txt | --params PARAMS.npz) [--mode shaded|shaded-color|
color|normal|depth] [--flat] [--every N] [--size WxH] [--intrinsics FX FY CX CY] [--samples K] [--black] [--transform FILE]``.

Shaded, colour, normal and depth views of a triangle mesh, rendered on the device (csrc/meshshade.hip, arithmetic in
csrc/meshshade_math.h) on top of the mesh render layer's exact, order-independent z-buffer:

``vertex_normals``   area-weighted vertex normals: per face (b - a) x (c - a) in double, quantised to 2^-40 m^2 and summed by 64-bit
                     integer atomics -- the same bits on every run and for every order of the faces.
``MeshViewer``       uploads a mesh once, computes its normals once and keeps the key plane and the output buffers; ``render`` makes a
                     picture [H, W, 3] uint8 ON THE DEVICE in two launches after a clear: a z-buffer of ((depth bits) << 32 | face) keys
                     (the nearest hit; on a shared edge the lowest face index: deterministic), and a shading pass that sets the winning
                     face up again, derives perspective-correct barycentrics from its edge planes and writes display bytes.
``render_mesh``      the one-shot form; ``render_trajectory`` writes ``mesh_%04d.png`` along a list of poses.

Modes: ``shaded`` (``albedo`` under a two-sided head light, L = ambient + (1 - ambient) |n . d|: winding never blackens a picture),
``shaded-color`` (the vertex colours under the same light), ``color`` (the vertex colours alone), ``normal`` ((n + 1) / 2 in the mesh's
frame, or in the camera's and facing the viewer with ``normal_frame="camera"``), ``depth`` (through a 256-entry table, as
``splatam_amd.view`` shows depth).  ``smooth=False`` (``--flat``) shades every face with its own normal.  ``samples`` = k renders k x k
sub-pixels per pixel and averages them: the only anti-aliasing.  A mesh without colours renders with ``albedo``.

The camera convention is ``mesh_render``'s: ``w2c`` is row-major world-to-camera in the mesh's frame, pixel (i, j) looks along
((i - cx) / fx, (j - cy) / fy, 1); ``intrinsics`` is (fx, fy, cx, cy) or a 3 x 3 matrix; ``size`` is (width, height).

Not here: textures, lights other than the head light, shadows, wireframe, transparency.  The ``face`` plane (``planes=True``) is what
triangle-level culling rules would be built on.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import _capi
from ._mesh_common import _mesh_arrays, _on_device, _pose_tensor, _ptr, _stream, _tensor
from .mesh_render import NEAR, _intrinsics, _view, load_poses, parse_size, to_device_mesh

MODES = {"color": _capi.SPLAT_MESH_SHADE_COLOR, "shaded": _capi.SPLAT_MESH_SHADE_SHADED, "shaded-color": _capi.SPLAT_MESH_SHADE_SHADED_COLOR,
         "normal": _capi.SPLAT_MESH_SHADE_NORMAL, "depth": _capi.SPLAT_MESH_SHADE_DEPTH}
NORMAL_FRAMES = {"world": 0, "camera": 1}
MAX_SAMPLES = 4
DEPTH_RANGE = (0.0, 6.0)                # ``splatam_amd.view``'s


def supersampled(intrinsics, size, samples):
    """((fx, fy, cx, cy), (width, height)) of the key plane of ``samples`` x ``samples`` sub-pixels per pixel: fx s, fy s,
    (cx + 0.5) s - 0.5 and cy alike, in float64 -- the centres of a pixel's sub-pixels then average to the pixel's own centre."""
    fx, fy, cx, cy = _intrinsics(intrinsics)
    s = int(samples)
    if not 1 <= s <= MAX_SAMPLES:
        raise ValueError(f"samples is 1..{MAX_SAMPLES} per axis (got {samples})")
    return (fx * s, fy * s, (cx + 0.5) * s - 0.5, (cy + 0.5) * s - 0.5), (int(size[0]) * s, int(size[1]) * s)


def vertex_normals(vertices, faces, out=None, accum=None):
    """[V, 3] float32 unit normals of ``vertices`` [V, 3] float32 / ``faces`` [F, 3] int32 (device tensors), area-weighted; (0, 0, 0) for
    a vertex no face names or whose faces cancel.  Faces with an index out of range, a non-finite vertex or a normal component of
    2^22 m^2 or more add nothing.  The same bits on every run and for every order of the faces.  ``accum``: int64 [V, 3] scratch.
    Enqueued on the current stream; nothing is read."""
    dev = vertices.device
    _on_device(dev, "vertex_normals")
    vertices, faces = _mesh_arrays(vertices, faces, dev)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    out = torch.empty(V, 3, dtype=torch.float32, device=dev) if out is None else _tensor(out, "out", torch.float32, (V, 3), dev, contiguous=True)
    accum = torch.empty(V, 3, dtype=torch.int64, device=dev) if accum is None else _tensor(accum, "accum", torch.int64, (V, 3), dev, contiguous=True)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_vertex_normals(_ptr(vertices, V), V, _ptr(faces, F), F, _ptr(accum, V), _ptr(out, V), _stream(dev)),
                    "splat_mesh_vertex_normals")
    return out


def render_keys(vertices, faces, w2c_ptr, view, keys):
    """The key plane of a view (a ``SplatMeshView`` whose ``w2c`` is set from ``w2c_ptr``) into ``keys`` [height, width] int64 (the bits of
    the uint64 keys: all ones where no triangle is met).  Enqueued; nothing is read."""
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    view.w2c = w2c_ptr
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_visibility(_ptr(vertices, V), V, _ptr(faces, F), F, view, keys.data_ptr(), _stream(dev)),
                    "splat_mesh_visibility")
    return keys


class MeshViewer:
    """A mesh on the device, ready to be pictured: ``MeshViewer(mesh, size, intrinsics, samples=1)``.  ``mesh``: a ``Mesh`` tuple of device
    tensors or host arrays, or the path of a PLY.  The mesh is uploaded and its normals are computed ONCE; the key plane
    ([height samples, width samples] int64) and the picture are kept, so ``render`` allocates nothing after the first call (the planes
    of ``planes=True`` after the first call that asks for them).  What ``render`` returns are the viewer's own buffers: the next call
    overwrites them."""

    def __init__(self, mesh, size, intrinsics, samples=1, device="cuda:0", near=NEAR, transform=None):
        self.mesh = to_device_mesh(mesh, device, transform)
        self.dev = self.mesh.vertices.device
        self.size = (int(size[0]), int(size[1]))
        self.samples = int(samples)
        self.intrinsics = _intrinsics(intrinsics)
        if not (float(near) > 0 and np.isfinite(float(near))):
            raise ValueError("near must be a positive number")
        k, ksize = supersampled(self.intrinsics, self.size, self.samples)
        _view(self.intrinsics, self.size, near)                          # (refuses a bad output size before the key plane's)
        self.view = _view(k, ksize, near)
        W, H = self.size
        v, f = _mesh_arrays(self.mesh.vertices, self.mesh.faces, self.dev)
        if self.mesh.colors is not None and tuple(self.mesh.colors.shape) != tuple(v.shape):
            raise ValueError(f"{self.mesh.colors.shape[0]} colours for {v.shape[0]} vertices")
        self.normals = vertex_normals(v, f)
        self.keys = torch.empty(ksize[1], ksize[0], dtype=torch.int64, device=self.dev)
        self.rgb8 = torch.empty(H, W, 3, dtype=torch.uint8, device=self.dev)
        self.pose = torch.empty(16, dtype=torch.float32, device=self.dev)
        self.lut = torch.empty(256, 3, dtype=torch.uint8, device=self.dev)
        self._default_lut = None
        self._lut_is_default = False
        self.planes = None
        self.args = _capi.SplatMeshShade()

    def _set_pose(self, w2c):
        t = _pose_tensor(w2c)
        if t.numel() != 16:
            raise ValueError("render renders one view: w2c is one 4 x 4 matrix")
        self.pose.copy_(t.reshape(16))

    def _set_lut(self, lut):
        if lut is None:
            if not self._lut_is_default:
                if self._default_lut is None:
                    from .view import jet_lut
                    self._default_lut = torch.from_numpy(np.ascontiguousarray(jet_lut()))
                self.lut.copy_(self._default_lut)
                self._lut_is_default = True
            return
        t = lut.detach() if isinstance(lut, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(lut, dtype=np.uint8)))
        if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
            raise ValueError("lut is [256, 3] uint8")
        self.lut.copy_(t)
        self._lut_is_default = False

    def render(self, w2c, mode="shaded", smooth=True, background=(1.0, 1.0, 1.0), albedo=(0.8, 0.8, 0.8), ambient=0.25, normal_frame="world",
               depth_range=None, lut=None, planes=False):
        """The picture [H, W, 3] uint8 (on the device) of the mesh seen from ``w2c`` (4 x 4, world-to-camera in the mesh's frame).
        ``depth_range`` defaults to (0, 6) m and ``lut`` ([256, 3] uint8) to ``view.jet_lut()``.  ``planes=True`` (``samples`` 1 only):
        also ``dict(depth, face, normal)`` -- [H, W] float32, bit for bit ``mesh_render.render_depth``'s plane; [H, W] int32, the
        winning face or -1; [H, W, 3] float32, the shading normal in the mesh's frame.  Enqueued on the current stream; nothing is read."""
        if mode not in MODES:
            raise ValueError(f"mode is one of {', '.join(MODES)} (got {mode!r})")
        if normal_frame not in NORMAL_FRAMES:
            raise ValueError(f"normal_frame is \"world\" or \"camera\" (got {normal_frame!r})")
        if planes and self.samples != 1:
            raise ValueError("the depth, face and normal planes are written with samples = 1 only")
        vmin, vmax = DEPTH_RANGE if depth_range is None else (float(depth_range[0]), float(depth_range[1]))
        self._set_pose(w2c)
        if mode == "depth":
            self._set_lut(lut)
        if planes and self.planes is None:
            H, W = self.rgb8.shape[:2]
            self.planes = dict(depth=torch.empty(H, W, dtype=torch.float32, device=self.dev), face=torch.empty(H, W, dtype=torch.int32, device=self.dev),
                               normal=torch.empty(H, W, 3, dtype=torch.float32, device=self.dev))
        a = self.args
        a.mode, a.samples, a.smooth, a.normal_frame = MODES[mode], self.samples, 1 if smooth else 0, NORMAL_FRAMES[normal_frame]
        for k in range(3):
            a.bg[k], a.albedo[k] = float(background[k]), float(albedo[k])
        a.ambient, a.vmin, a.vmax = float(ambient), vmin, vmax
        a.lut = self.lut.data_ptr()
        v, f, c = self.mesh.vertices, self.mesh.faces, self.mesh.colors
        V, F = int(v.shape[0]), int(f.shape[0])
        render_keys(v, f, self.pose.data_ptr(), self.view, self.keys)
        p = self.planes if planes else None
        with torch.cuda.device(self.dev):
            _capi.check(_capi.lib().splat_mesh_shade(_ptr(v, V), V, _ptr(f, F), F, _ptr(c, c is not None and V), _ptr(self.normals, V), self.view,
                                                     self.keys.data_ptr(), a, self.rgb8.data_ptr(), p['depth'].data_ptr() if p else None,
                                                     p['face'].data_ptr() if p else None, p['normal'].data_ptr() if p else None, _stream(self.dev)),
                        "splat_mesh_shade")
        return (self.rgb8, p) if planes else self.rgb8


def render_mesh(mesh, w2c, intrinsics, size, samples=1, device="cuda:0", near=NEAR, transform=None, **kw):
    """One picture of ``mesh`` (a ``Mesh`` or the path of a PLY): ``MeshViewer(mesh, size, intrinsics, samples).render(w2c, **kw)``."""
    return MeshViewer(mesh, size, intrinsics, samples=samples, device=device, near=near, transform=transform).render(w2c, **kw)


def render_trajectory(mesh, poses, out_dir, intrinsics, size, every=1, samples=1, device="cuda:0", transform=None, verbose=False, workers=4,
                      numbers=None, **kw):
    """Writes ``mesh_%04d.png`` (numbered by the pose's index, or by ``numbers[index]``) for every ``every``-th of the ``poses`` [n, 4, 4]
    (world-to-camera in the mesh's frame) into ``out_dir``; returns the files' paths.  ``mesh``: a ``Mesh``, a path or a ``MeshViewer``.  The pictures are rendered on the device, read one by one and encoded to
    PNG on a small thread pool."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    if int(every) <= 0:
        raise ValueError("every must be positive")
    viewer = mesh if isinstance(mesh, MeshViewer) else MeshViewer(mesh, size, intrinsics, samples=samples, device=device, transform=transform)
    poses = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
    poses = poses.reshape(-1, 4, 4)
    os.makedirs(out_dir, exist_ok=True)
    written, jobs = [], []
    with ThreadPoolExecutor(max_workers=max(int(workers), 1)) as pool:
        for t in range(0, len(poses), int(every)):
            image = viewer.render(poses[t], **kw).cpu().numpy()            # (a copy: the viewer's buffer is free for the next pose)
            name = os.path.join(out_dir, f"mesh_{t if numbers is None else int(numbers[t]):04d}.png")
            jobs.append(pool.submit(lambda a=image, n=name: Image.fromarray(a).save(n)))
            written.append(name)
            if verbose:
                print(name, flush=True)
        for job in jobs:
            job.result()                                                 # (a failed write raises here)
    return written


def params_poses(path):
    """(w2c [n, 4, 4] float64, intrinsics [3, 3], (width, height)) of a ``params.npz``: the ESTIMATED poses (``post_opt.estimated_w2c``
    seen through the first frame's ``w2c``), in the map's frame -- the frame of a mesh extracted from that map."""
    from .post_opt import estimated_w2c
    from .view import _check_run_file
    with np.load(path) as z:
        _check_run_file(z, path)
        params = {k: torch.from_numpy(np.ascontiguousarray(z[k], dtype=np.float32)) for k in ("cam_unnorm_rots", "cam_trans")}
        k = np.array(z['intrinsics'], dtype=np.float64)[:3, :3]
        first = np.array(z['w2c'], dtype=np.float64).reshape(4, 4)
        size = (int(z['org_width']), int(z['org_height']))
    n = int(params['cam_trans'].shape[-1])
    poses = np.stack([estimated_w2c(params, t).double().numpy() @ first for t in range(n)])
    return poses, k, size


def _parser():
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.mesh_view", description=__doc__.split("\n\n")[0])
    parser.add_argument("mesh", help="the PLY to picture")
    parser.add_argument("--out", required=True, help="directory for mesh_%%04d.png")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--poses", help="camera-to-world matrices, 16 numbers per line (a Replica traj.txt); needs --size and --intrinsics")
    source.add_argument("--params", help="params.npz of a run: its estimated poses, its intrinsics and its frame size")
    parser.add_argument("--mode", default="shaded", choices=tuple(MODES))
    parser.add_argument("--flat", action="store_true", help="every face its own normal")
    parser.add_argument("--every", type=int, default=1, help="every N-th pose")
    parser.add_argument("--size", type=parse_size, default=None, help="WIDTHxHEIGHT of the pictures (default with --params: the run's frame size)")
    parser.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"), help="of pictures of --size")
    parser.add_argument("--samples", type=int, default=1, choices=range(1, MAX_SAMPLES + 1), help="sub-pixels per axis (supersampling)")
    parser.add_argument("--black", action="store_true", help="a black background instead of the white one")
    parser.add_argument("--transform", default=None, help="a text file of a 4 x 4 matrix applied to the mesh's vertices first")
    parser.add_argument("--device", default="cuda:0")
    return parser


def _resolve(parser, args):
    """(poses, intrinsics, size) of the parsed arguments."""
    if args.every <= 0:
        parser.error("--every must be positive")
    if args.poses is not None:
        if args.size is None or args.intrinsics is None:
            parser.error("--poses needs --size and --intrinsics")
        return load_poses(args.poses), tuple(args.intrinsics), args.size
    from .view import _scaled_intrinsics
    poses, k, size0 = params_poses(args.params)
    size = args.size or size0
    return poses, (tuple(args.intrinsics) if args.intrinsics is not None else _scaled_intrinsics(k, size, size0)), size


def main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    try:
        poses, intrinsics, size = _resolve(parser, args)
        transform = np.loadtxt(args.transform).reshape(4, 4) if args.transform else None
        written = render_trajectory(args.mesh, poses, args.out, intrinsics, size, every=args.every, samples=args.samples, device=args.device,
                                    transform=transform, verbose=True, mode=args.mode, smooth=not args.flat,
                                    background=(0.0, 0.0, 0.0) if args.black else (1.0, 1.0, 1.0))
    except ValueError as e:
        raise SystemExit(str(e)) from None
    print(f"wrote {len(written)} pictures to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
