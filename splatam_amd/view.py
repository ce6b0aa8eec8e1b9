"""Look at a map: ``python -m splatam_amd.view PARAMS.npz --out DIR [--mode color|depth|sil] [--replay] [--every N] [--size WxH] [--white]``.

Loads a ``params.npz`` as ``python -m splatam_amd.run`` writes it (the reference's entries: the map, ``timestep``, ``intrinsics``,
``w2c``, ``org_width`` / ``org_height``), builds a ``FusedEngine`` around it and writes ``view_%04d.png`` along the estimated
trajectory through ``FusedEngine.render_view`` (csrc/view.hip): the headless counterpart of the reference's viewers.  Without
``--replay`` it is ``viz_scripts/final_recon.py``'s camera on the finished map at every estimated pose; with ``--replay`` it is
``viz_scripts/online_recon.py``: the map as it stood at each time step (the Gaussians with ``timestep <= t``), seen from the follow
camera half a metre behind the estimated pose.  ``--white`` composites on the viewers' white background.  No window is opened;
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


def follow_offset(dz=FOLLOW_OFFSET_Z):
    """The 4 x 4 multiplied from the left of a pose by the follow camera: a translation along the view's z."""
    m = np.eye(4)
    m[2, 3] = dz
    return m


def load_map(path, device):
    """(params, variables, intrinsics [3, 3] numpy, first-frame w2c tensor on ``device``, (width, height)) of a ``params.npz``."""
    import torch
    from .fused import PARAM_ORDER
    with np.load(path) as z:
        missing = [k for k in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans", "intrinsics", "w2c", "org_width", "org_height") if k not in z]
        if missing:
            raise SystemExit(f"{path}: not a params.npz of a run (missing {', '.join(missing)})")
        params = {k: torch.from_numpy(np.ascontiguousarray(z[k], dtype=np.float32)).to(device)
                  for k in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        variables = {'timestep': torch.from_numpy(np.ascontiguousarray(z['timestep'], dtype=np.float32)).to(device)} if 'timestep' in z else None
        k = np.array(z['intrinsics'], dtype=np.float64)[:3, :3]
        w2c = torch.from_numpy(np.ascontiguousarray(z['w2c'], dtype=np.float32)).to(device)
        size = (int(z['org_width']), int(z['org_height']))
    return params, variables, k, w2c, size


def render_trajectory(path, out_dir, mode="color", replay=False, every=1, size=None, white=False, device="cuda:0", verbose=True):
    """Writes ``view_%04d.png`` for every ``every``-th estimated pose of ``path`` into ``out_dir``; returns the files' paths."""
    import torch
    from PIL import Image
    from . import slam
    from .fused import FusedEngine
    dev = torch.device(device)
    params, variables, k, first_w2c, (W0, H0) = load_map(path, dev)
    if replay and variables is None:
        raise SystemExit(f"{path}: --replay needs the map's `timestep` entry")
    W, H = size or (W0, H0)
    os.makedirs(out_dir, exist_ok=True)
    with torch.no_grad():
        cam = slam.setup_camera(W0, H0, k, first_w2c.cpu().numpy(), device=dev)
        k = k.copy()
        k[0] *= W / W0                  # (fx, cx and fy, cy of the pictures' size: slam.scale_intrinsics)
        k[1] *= H / H0
        engine = FusedEngine(params, cam, variables=variables)
        view = engine.view_camera(W, H)
        bg = (1.0, 1.0, 1.0) if white else (0.0, 0.0, 0.0)
        offset = follow_offset() if replay else None
        written = []
        for t in range(0, engine.num_frames, max(int(every), 1)):
            for _ in range(3):
                image = engine.render_view(view, time_idx=t, first_w2c=first_w2c, intrinsics=k, mode=mode, background=bg,
                                           max_timestep=t if replay else None, offset=offset)
                if not view.check_overflow():       # (the picture is read right below: the digest's two small reads ride along)
                    break
            else:
                raise RuntimeError(f"frame {t}: the per-tile lists could not be sized for its view")
            name = os.path.join(out_dir, f"view_{t:04d}.png")
            Image.fromarray(image.rgb8.cpu().numpy()).save(name)
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
    parser.add_argument("--mode", default="color", choices=("color", "depth", "sil"))
    parser.add_argument("--replay", action="store_true", help="the map as it stood at each time step, from the follow camera")
    parser.add_argument("--every", type=int, default=1, help="every N-th pose of the trajectory")
    parser.add_argument("--size", type=_size, default=None, help="WIDTHxHEIGHT of the pictures (default: the run's frame size)")
    parser.add_argument("--white", action="store_true", help="composite on a white background")
    parser.add_argument("--device", default="cuda:0")
    args = parser.parse_args(argv)
    written = render_trajectory(args.params, args.out, mode=args.mode, replay=args.replay, every=args.every, size=args.size,
                                white=args.white, device=args.device)
    print(f"wrote {len(written)} pictures to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
