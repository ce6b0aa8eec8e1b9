"""Look at a map: ``python -m splatam_amd.view PARAMS.npz --out DIR [--mode color|depth|sil|centers] [--replay] [--every N] [--size WxH]
[--white] [--cameras] [--frusta all|current|none] [--gt-trajectory] [--frustum-size M] [--point-size K] [--line-width K] [--no-occlude]``.

Loads a ``params.npz`` as ``python -m splatam_amd.run`` writes it (the reference's entries: the map, ``timestep``, ``intrinsics``,
``w2c``, ``org_width`` / ``org_height``), builds a ``FusedEngine`` around it and writes ``view_%04d.png`` along the estimated
trajectory through ``FusedEngine.render_view`` (csrc/view.hip): the headless counterpart of the reference's viewers.  Without
``--replay`` it is ``viz_scripts/final_recon.py``'s camera on the finished map at every estimated pose; with ``--replay`` it is
``viz_scripts/online_recon.py``: the map as it stood at each time step (the Gaussians with ``timestep <= t``), seen from the follow
camera half a metre behind the estimated pose.  ``--white`` composites on the viewers' white background.  ``--cameras`` draws what the
viewers draw besides the map -- the estimated trajectory and the camera frusta, coloured along matplotlib's ``cool``, depth-tested
against the picture (csrc/viewoverlay.hip, ``RunOverlay``); ``--mode centers`` is their render mode of that name.  No window is opened;
INTEGRATION.md section 7 shows how to feed one.

``jet_lut()`` is the default colour table of depth mode: matplotlib's ``jet`` at 256 entries, rebuilt from its piecewise-linear
definition without importing matplotlib (pinned by tests/golden/jet_lut.npy).  This is the map of the reference's plots and viewers
(``plt.get_cmap('jet')``).  The reference's ``save_frames`` uses ``cv2.COLORMAP_JET`` instead, a different table of the same name; OpenCV
is installed neither where this is developed nor where it is tested, so that table cannot be obtained and is NOT pinned: saved depth
frames here carry matplotlib's jet.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

# matplotlib's _jet_data: (x, y below x, y above x) per channel
_JET = {
    'red': ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    'green': ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    'blue': ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}
FOLLOW_OFFSET_Z = 0.5       # the follow camera of the reference's online viewer: +0.5 m along the view's z


def _segment_table(data, n):
    """One channel of a linearly segmented colour map at ``n`` entries, as matplotlib tabulates it: entry i sits at x = i / (n - 1), between
    the two mapping points around it the value runs linearly from the left point's upper to the right point's lower value."""
    data = np.array(data, dtype=float)
    x, y0, y1 = data[:, 0] * (n - 1), data[:, 1], data[:, 2]
    xind = (n - 1) * np.linspace(0, 1, n)
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0)


def jet_lut():
    """[256, 3] uint8: ``matplotlib.colormaps['jet'](np.arange(256), bytes=True)[:, :3]`` (see the module's docstring for which jet this is)."""
    table = np.stack([_segment_table(_JET[c], 256) for c in ('red', 'green', 'blue')], axis=1)
    return (table * 255).astype(np.uint8)


def cool_lut():
    """[256, 3] uint8: matplotlib's ``cool`` at 256 entries from its formula, entry i = (i / 255, 1 - i / 255, 1), as bytes rounded to
    nearest like every colour of the view layer: (i, 255 - i, 255).  (``matplotlib.colormaps['cool'](i, bytes=True)`` truncates a
    table that sits an ulp below i / 255 in places and is one lower in 62 of its bytes.)  The map the reference's viewers colour frusta
    (its lower half) and trajectory (its upper half) with; the overlay kernels evaluate the same formula (csrc/viewoverlay_math.h
    vo_cool), this table is for legends and tests."""
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.rint(np.stack([v, 1.0 - v, np.ones(256)], axis=1) * 255).astype(np.uint8)


def follow_offset(dz=FOLLOW_OFFSET_Z):
    """The 4 x 4 multiplied from the left of a pose by the follow camera: a translation along the view's z."""
    m = np.eye(4)
    m[2, 3] = dz
    return m


FRUSTUM_SIZE = 0.045        # the viewers' frustum_size
GT_COLOR = (255, 255, 0)    # the ground-truth polyline (this project's addition: the reference's viewers do not draw one)


class RunOverlay:
    """The cameras of a run as line segments on the device (csrc/viewoverlay.hip splat_view_run_segments), for ``render_view(overlay=...)``:
    the estimated trajectory as a polyline through the camera centres and one frustum per frame, coloured along matplotlib's ``cool``
    as the reference's viewers colour them (viz_scripts/final_recon.py:194-223).  The frustum is a stated construction -- apex at the
    centre, the image's four corners at depth ``frustum_size`` -- after Open3D's ``create_camera_visualization`` as recalled; Open3D
    is not available to compare with and no parity is claimed.

    ``source``: a ``FusedEngine`` or a dict of parameters with ``cam_unnorm_rots`` [1, 4, n] / ``cam_trans`` [1, 3, n] on the device; the
    poses are read by the kernel at every ``refresh``, never on the host.  ``first_w2c``: float32 [4, 4] on the device (default the
    identity).  ``intrinsics`` / ``size`` = (width, height): the RUN's camera, whose image corners the frusta span.  ``gt_w2c``
    ([n, 4, 4], e.g. a ``params.npz``'s ``gt_w2c_all_frames``): a second polyline through the ground-truth centres in ``GT_COLOR`` --
    not in the reference's viewers, this project's addition.

    Arrays: ``segments`` [S, 6] float32, ``colors`` [S, 3] uint8; trajectory segments [0, n - 1), eight per frame from n - 1, then the
    ground-truth polyline's n - 1.  ``refresh(upto)`` rebuilds frames 0..upto in place (one launch, nothing allocated)."""

    def __init__(self, source, num_frames, first_w2c=None, frustum_size=FRUSTUM_SIZE, intrinsics=None, size=None, gt_w2c=None):
        import ctypes as C
        import torch
        from . import _capi
        from .fused import _intrinsics4
        if intrinsics is None or size is None:
            raise ValueError("RunOverlay needs the run's intrinsics and size = (width, height)")
        self._source = source
        rots, _ = self._poses()
        self.dev, n = rots.device, int(num_frames)
        if n < 1 or n != rots.shape[-1]:
            raise ValueError(f"num_frames {n} is not the number of poses the parameters hold ({rots.shape[-1]}): the run's length sets "
                             "the colours and the layout (draw a part of it with overlay_upto)")
        self.num_frames, self._stride = n, int(rots.shape[-1])
        self.first_w2c = torch.eye(4, dtype=torch.float32, device=self.dev) if first_w2c is None else first_w2c
        if not (self.first_w2c.dtype == torch.float32 and tuple(self.first_w2c.shape) == (4, 4) and self.first_w2c.is_contiguous()
                and self.first_w2c.device == self.dev):
            raise RuntimeError(f"first_w2c must be a contiguous float32 tensor of shape [4, 4] on {self.dev}")
        self.gt_first = 9 * n - 1
        self.num_segments = self.gt_first + (n - 1 if gt_w2c is not None else 0)
        self.segments = torch.zeros(max(self.num_segments, 1), 6, dtype=torch.float32, device=self.dev)
        self.colors = torch.zeros(max(self.num_segments, 1), 3, dtype=torch.uint8, device=self.dev)
        r = self._run = _capi.SplatViewRun()
        r.width, r.height = int(size[0]), int(size[1])
        r.fx, r.fy, r.cx, r.cy = _intrinsics4(intrinsics)
        r.scale, r.frusta = float(frustum_size), 1
        r.segments, r.colors = self.segments.data_ptr(), self.colors.data_ptr()
        self._C, self._capi, self._torch = C, _capi, torch
        self.gt_w2c = None
        if gt_w2c is not None:
            gt = torch.as_tensor(np.ascontiguousarray(np.asarray(gt_w2c.cpu() if hasattr(gt_w2c, "cpu") else gt_w2c, dtype=np.float32)))
            if tuple(gt.shape[1:]) != (4, 4) or gt.shape[0] < n:
                raise ValueError(f"gt_w2c must be [>= {n}, 4, 4] (got {tuple(gt.shape)})")
            self.gt_w2c = gt[:n].contiguous().to(self.dev)
            g = _capi.SplatViewRun()
            g.num_frames, g.first, g.count, g.w2c_all = n, 0, n, self.gt_w2c.data_ptr()
            g.frusta, g.fixed_color = 0, 1
            g.color[:3] = GT_COLOR
            g.segments, g.colors = self.segments[self.gt_first:].data_ptr(), self.colors[self.gt_first:].data_ptr()
            self._launch(g)
        self.refresh()

    def _poses(self):
        p = self._source.params if hasattr(self._source, "params") else self._source
        return p['cam_unnorm_rots'], p['cam_trans']

    def _launch(self, run):
        torch = self._torch
        with torch.cuda.device(self.dev):
            self._capi.check(self._capi.lib().splat_view_run_segments(self._C.byref(run), torch.cuda.current_stream(self.dev).cuda_stream),
                             "splat_view_run_segments")

    def refresh(self, upto=None):
        """Rebuilds the segments of frames 0..``upto`` (default: all) from the CURRENT pose parameters, on the current stream."""
        upto = self.num_frames - 1 if upto is None else int(upto)
        if not 0 <= upto < self.num_frames:
            raise ValueError(f"upto {upto} is outside the run's {self.num_frames} frames")
        rots, trans = self._poses()
        if rots.shape[-1] != self._stride or not (rots.is_contiguous() and trans.is_contiguous()) or rots.dtype != self._torch.float32:
            raise RuntimeError("the pose parameters changed their shape or layout since the overlay was made")
        r = self._run
        r.num_frames, r.first, r.count = self._stride, 0, upto + 1
        r.cam_unnorm_rots, r.cam_trans, r.first_w2c = rots.data_ptr(), trans.data_ptr(), self.first_w2c.data_ptr()
        self._launch(r)
        return self

    def ranges(self, upto=None, frusta="all"):
        """[(first, count)] of ``segments`` that show the run up to time step ``upto``: the trajectory so far, every frustum up to it
        ("all"), its own ("current") or none (None / "none"), the ground-truth polyline so far."""
        upto = self.num_frames - 1 if upto is None else int(upto)
        if not 0 <= upto < self.num_frames:
            raise ValueError(f"overlay_upto {upto} is outside the run's {self.num_frames} frames")
        if frusta not in ("all", "current", "none", None):
            raise ValueError(f"frusta must be 'all', 'current' or None (got {frusta!r})")
        base = self._stride - 1
        out = [(0, upto)]
        if frusta == "all":
            out.append((base, 8 * (upto + 1)))
        elif frusta == "current":
            out.append((base + 8 * upto, 8))
        if self.gt_w2c is not None:
            out.append((self.gt_first, upto))
        return [(first, count) for first, count in out if count > 0]


_RUN_KEYS = ("cam_unnorm_rots", "cam_trans", "intrinsics", "w2c", "org_width", "org_height")     # of a run's params.npz, besides the map


def _check_run_file(z, path, keys=_RUN_KEYS):
    """``z`` (the opened ``path``) holds every one of ``keys``: a ``params.npz`` as a run writes it."""
    missing = [k for k in keys if k not in z]
    if missing:
        raise SystemExit(f"{path}: not a params.npz of a run (missing {', '.join(missing)})")


def _scaled_intrinsics(intrinsics, size, org_size):
    """(fx, fy, cx, cy) of pictures of ``size`` = (width, height) from the intrinsics of pictures of ``org_size``: slam.scale_intrinsics."""
    from .fused import _intrinsics4
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    sx, sy = size[0] / org_size[0], size[1] / org_size[1]
    return fx * sx, fy * sy, cx * sx, cy * sy


def load_map(path, device, extras=None):
    """(params, variables, intrinsics [3, 3] numpy, first-frame w2c tensor on ``device``, (width, height)) of a ``params.npz``.  With
    ``extras`` (names of further entries, such as ``keyframe_time_indices`` or ``gt_w2c_all_frames``) a sixth element: a dict of those
    entries as numpy arrays, None for one the file does not hold."""
    import torch
    from .fused import PARAM_ORDER
    with np.load(path) as z:
        _check_run_file(z, path, PARAM_ORDER + _RUN_KEYS)
        params = {k: torch.from_numpy(np.ascontiguousarray(z[k], dtype=np.float32)).to(device)
                  for k in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        variables = {'timestep': torch.from_numpy(np.ascontiguousarray(z['timestep'], dtype=np.float32)).to(device)} if 'timestep' in z else None
        k = np.array(z['intrinsics'], dtype=np.float64)[:3, :3]
        w2c = torch.from_numpy(np.ascontiguousarray(z['w2c'], dtype=np.float32)).to(device)
        size = (int(z['org_width']), int(z['org_height']))
        more = {name: np.array(z[name]) if name in z else None for name in extras or ()}
    return (params, variables, k, w2c, size) + ((more,) if extras is not None else ())


def render_trajectory(path, out_dir, mode="color", replay=False, every=1, size=None, white=False, device="cuda:0", verbose=True,
                      cameras=False, frusta=None, gt_trajectory=False, frustum_size=FRUSTUM_SIZE, point_size=1, line_width=1, occlude=True):
    """Writes ``view_%04d.png`` for every ``every``-th estimated pose of ``path`` into ``out_dir``; returns the files' paths.
    ``cameras``: the run's cameras drawn in (``RunOverlay``) -- with ``replay`` the online viewer's picture by default (the trajectory so
    far and the current frustum), without it the final viewer's (the whole trajectory, every frustum); ``frusta`` ("all", "current",
    "none") overrides.  ``gt_trajectory``: the file's ``gt_w2c_all_frames`` as a second polyline."""
    import torch
    from PIL import Image
    from . import slam
    from .fused import FusedEngine
    from .map_pass import fit_lists
    dev = torch.device(device)
    params, variables, k0, first_w2c, (W0, H0), more = load_map(path, dev, extras=("gt_w2c_all_frames",) if gt_trajectory else ())
    if replay and variables is None:
        raise SystemExit(f"{path}: --replay needs the map's `timestep` entry")
    gt = more.get("gt_w2c_all_frames")
    if gt_trajectory and gt is None:
        raise SystemExit(f"{path}: --gt-trajectory needs the file's `gt_w2c_all_frames` entry")
    W, H = size or (W0, H0)
    os.makedirs(out_dir, exist_ok=True)
    with torch.no_grad():
        cam = slam.setup_camera(W0, H0, k0, first_w2c.cpu().numpy(), device=dev)
        k = _scaled_intrinsics(k0, (W, H), (W0, H0))
        engine = FusedEngine(params, cam, variables=variables)
        view = engine.view_camera(W, H)
        bg = (1.0, 1.0, 1.0) if white else (0.0, 0.0, 0.0)
        offset = follow_offset() if replay else None
        overlay = None
        if cameras or gt_trajectory:
            overlay = RunOverlay(engine, engine.num_frames, first_w2c=first_w2c.contiguous(), frustum_size=frustum_size, intrinsics=k0, size=(W0, H0),
                                 gt_w2c=gt)
            frusta = (("current" if replay else "all") if cameras else "none") if frusta is None else frusta
        written = []

        for t in range(0, engine.num_frames, max(int(every), 1)):
            # (the picture is read right below: the digest's two small reads ride along; the centres' picture uses no lists)
            fit_lists(lambda: engine.render_view(view, time_idx=t, first_w2c=first_w2c, intrinsics=k, mode=mode, background=bg,
                                                 max_timestep=t if replay else None, offset=offset, point_size=point_size, overlay=overlay,
                                                 overlay_upto=t if replay else None, frusta=frusta, line_width=line_width, occlude=occlude),
                      lambda: mode != "centers" and view.check_overflow(), f"frame {t}: the per-tile lists could not be sized for its view")
            name = os.path.join(out_dir, f"view_{t:04d}.png")
            Image.fromarray(view.rgb8.cpu().numpy()).save(name)       # (``rgb8`` of the ViewImage: the view's own)
            written.append(name)
            if verbose:
                print(name, flush=True)
    return written


def _size(text):
    try:
        w, h = text.lower().split("x")
        w, h = int(w), int(h)
        if w <= 0 or h <= 0:
            raise ValueError
        return w, h
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected WIDTHxHEIGHT, e.g. 640x480 (got {text!r})") from None


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.view", description=__doc__.split("\n\n")[0])
    parser.add_argument("params", help="params.npz of a run")
    parser.add_argument("--out", required=True, help="directory for view_%%04d.png")
    parser.add_argument("--mode", default="color", choices=("color", "depth", "sil", "centers"),
                        help="centers: every Gaussian's centre as a point in its colour (the viewers' render mode of that name)")
    parser.add_argument("--replay", action="store_true", help="the map as it stood at each time step, from the follow camera")
    parser.add_argument("--every", type=int, default=1, help="every N-th pose of the trajectory")
    parser.add_argument("--size", type=_size, default=None, help="WIDTHxHEIGHT of the pictures (default: the run's frame size)")
    parser.add_argument("--white", action="store_true", help="composite on a white background")
    parser.add_argument("--cameras", action="store_true",
                        help="draw the estimated trajectory and camera frusta (with --replay: the trajectory so far and the current frustum)")
    parser.add_argument("--frusta", default=None, choices=("all", "current", "none"), help="which frusta --cameras draws")
    parser.add_argument("--gt-trajectory", action="store_true", help="draw the ground-truth trajectory (gt_w2c_all_frames) as a second line")
    parser.add_argument("--frustum-size", type=float, default=FRUSTUM_SIZE, metavar="M", help="depth of a frustum's base in metres")
    parser.add_argument("--point-size", type=int, default=1, choices=range(1, 9), metavar="K", help="pixels across a centre (1..8)")
    parser.add_argument("--line-width", type=int, default=1, choices=range(1, 5), metavar="K", help="pixels across a line (1..4)")
    parser.add_argument("--no-occlude", action="store_true", help="draw cameras and trajectory over the map instead of depth-testing them")
    parser.add_argument("--device", default="cuda:0")
    args = parser.parse_args(argv)
    if args.frusta is not None and not args.cameras:
        parser.error("--frusta needs --cameras")
    written = render_trajectory(args.params, args.out, mode=args.mode, replay=args.replay, every=args.every, size=args.size,
                                white=args.white, device=args.device, cameras=args.cameras, frusta=args.frusta,
                                gt_trajectory=args.gt_trajectory, frustum_size=args.frustum_size, point_size=args.point_size,
                                line_width=args.line_width, occlude=not args.no_occlude)
    print(f"wrote {len(written)} pictures to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
