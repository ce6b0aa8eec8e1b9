"""The case behind tests/golden/nvs_reference.npz: a held-out split over the scene of tests/eval_ref.py (240 x 176), regenerated from
its seeds by the generator (tests/golden/make_golden_nvs.py, which runs the reference's ``eval_nvs`` on it) and by the tests.

Item 0 is the first training frame; items 1 .. 12 are held-out frames at poses that are NOT on the training trajectory (rotations
about all three axes, sideways and vertical shifts).  The map is the scene without the Gaussians of one region -- a hole --, and every
frame has a rectangle of invalid depth.  Where the rectangle lies decides what eval_nvs makes of the frame:
  * "cover":   it covers the hole's projection with a margin -- (almost) no pixel has depth where the map shows nothing: a VALID view;
  * "patch":   as "cover", but a 5 x 4 patch of depth is kept well inside the hole: 20 holes, below the 0.1 % limit (42.24 pixels)
               -- a valid view whose hole count is not zero;
  * "open":    it lies elsewhere: the hole is seen against valid depth, hundreds of holes -- an INVALID view.
The scored frames of every cadence used (1 and 3) hold at least two views of each kind of verdict."""
import math

import numpy as np
import torch

from tests import eval_ref

SCENE = dict(eval_ref.GOLDEN_SCENE, frames=13)
SIL_THRES = eval_ref.GOLDEN_SIL_THRES
HOLE = dict(x=(0.2, 0.7), y=(-0.1, 0.35))             # the region of eval_ref.golden_case
# held-out index k -> kind; cadence 3 scores k = 0, 2, 5, 8, 11: cover, open, patch, cover, open
KINDS = ("cover", "cover", "open", "open", "open", "patch", "patch", "open", "cover", "cover", "open", "open")
MARGIN = 8
# (map, (mapping_iters, add_new_gaussians), eval_every, general first pose)
CASES = {
    "iso/valid/every1": ("iso", eval_ref.GOLDEN_VARIANTS["valid"], 1, False),
    "iso/sil/every3": ("iso", eval_ref.GOLDEN_VARIANTS["sil"], 3, False),
    "aniso/valid/every3": ("aniso", eval_ref.GOLDEN_VARIANTS["valid"], 3, False),
    "aniso/sil/every1": ("aniso", eval_ref.GOLDEN_VARIANTS["sil"], 1, False),
    "general/valid/every3": ("iso", eval_ref.GOLDEN_VARIANTS["valid"], 3, True),
}


def held_out_w2c(k):
    """World-to-camera of held-out frame k (float64 [4, 4]): a turn of up to ~4 degrees about a seeded axis with components on all
    three axes, a shift of a few centimetres in x, y and z."""
    rng = np.random.default_rng(700 + k)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = math.radians(1.5 + 2.5 * rng.random())
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    m[:3, 3] = rng.uniform(-0.08, 0.08, size=3) * np.array([1.0, 0.6, 0.5])
    return m


def _quat(R):
    """(w, x, y, z) of a rotation matrix with a small angle (w is the largest component)."""
    w = math.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 0.0)) / 2
    return [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)]


class HeldOutSplit:
    """Items as a dataset's test split hands them over: item 0 the first training frame, then the held-out frames.  ``first_w2c``
    (None: the identity): the first frame's world-to-camera M; the poses are then ``pose_0 = inv(M)`` and ``pose_t = inv(C_t) @ M``,
    so that ``inv(pose_0) @ inv(pose_t)`` is the frame's true world-to-camera C_t."""

    def __init__(self, frames, w2cs, k, first_w2c=None):
        M = torch.eye(4) if first_w2c is None else torch.as_tensor(np.asarray(first_w2c), dtype=torch.float32)
        M = M.to(frames[0][0].device)
        self.items = []
        for t, (color, depth) in enumerate(frames):
            C = torch.as_tensor(w2cs[t], dtype=torch.float32).to(M.device)
            pose = torch.linalg.inv(M) if t == 0 else torch.linalg.inv(C) @ M
            self.items.append((color, depth, k, pose.contiguous()))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, t):
        return self.items[t]


def _anisotropic(scene):
    """The scene with ellipsoids: per-axis scales spread by seeded factors of 0.9 .. 1.2 and seeded orientations."""
    g = torch.Generator().manual_seed(4321)
    n = scene['means3D'].shape[0]
    dev = scene['means3D'].device
    out = dict(scene)
    out['log_scales'] = (scene['log_scales'].cpu() + 0.3 * (torch.rand(n, 3, generator=g) - 0.35)).to(dev).contiguous()
    out['unnorm_rotations'] = torch.randn(n, 4, generator=g).to(dev).contiguous()
    return out


_cache = {}


def scene_and_frames(kind, device="cpu"):
    """(final params, frames [(color [H, W, 3] in 0..255, depth [H, W, 1])], world-to-camera per item, intrinsics [4, 4]) of the
    isotropic (``kind="iso"``) or anisotropic (``"aniso"``) scene; rendered once per kind and device with whatever ``slam.Renderer``
    is at that moment."""
    from splatam_amd import pipeline
    key = (kind, str(device))
    if key in _cache:
        return _cache[key]
    s = SCENE
    ds = pipeline.SyntheticRGBDSequence(s['n_gaussians'], s['W'], s['H'], s['f'], s['f'], s['W'] / 2 - 0.5, s['H'] / 2 - 0.5, num_frames=s['frames'],
                                        seed=s['seed'], device=device, step_m=s['step_m'], step_deg=s['step_deg'])
    if kind == "aniso":
        ds._scene = _anisotropic(ds._scene)
    w2cs = [np.eye(4)] + [held_out_w2c(k) for k in range(s['frames'] - 1)]
    for t, m in enumerate(w2cs):
        ds._scene['cam_unnorm_rots'][0, :, t] = torch.tensor(_quat(m[:3, :3]), dtype=torch.float32)
        ds._scene['cam_trans'][0, :, t] = torch.tensor(m[:3, 3], dtype=torch.float32)
    w2cs = [ds.gt_w2c(t).cpu().numpy().astype(np.float64) for t in range(s['frames'])]        # (as rendered: from the float32 quaternion)
    scene = ds._scene
    m3 = scene['means3D']
    gone = (m3[:, 0] > HOLE['x'][0]) & (m3[:, 0] < HOLE['x'][1]) & (m3[:, 1] > HOLE['y'][0]) & (m3[:, 1] < HOLE['y'][1])
    params = {k: (v[~gone] if v.shape[0] == m3.shape[0] else v).clone().contiguous() for k, v in scene.items()
              if k not in ('cam_unnorm_rots', 'cam_trans')}
    # a reconstruction is not the scene: seeded errors of ~1 cm in the centres and ~0.04 in the colours, so that PSNR and depth L1 are
    # the finite numbers of a real run (30 dB, millimetres) and not the rounding noise of a perfect map
    g = torch.Generator().manual_seed(97)
    params['means3D'] = (params['means3D'] + 0.01 * torch.randn(params['means3D'].shape, generator=g).to(m3.device)).contiguous()
    params['rgb_colors'] = (params['rgb_colors'] + 0.04 * torch.randn(params['rgb_colors'].shape, generator=g).to(m3.device)).contiguous()
    # (eval_nvs reads no trajectory; a one-frame identity keeps the dict a complete map for FusedEngine)
    params['cam_unnorm_rots'] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=m3.device).view(1, 4, 1)
    params['cam_trans'] = torch.zeros(1, 3, 1, device=m3.device)
    f, cx, cy, W, H = s['f'], s['W'] / 2 - 0.5, s['H'] / 2 - 0.5, s['W'], s['H']
    removed = m3[gone].cpu().numpy().astype(np.float64)
    frames = []
    for t in range(s['frames']):
        color, depth, _, _ = ds[t]
        depth = depth.clone()
        kind_t = "open" if t == 0 else KINDS[t - 1]
        if kind_t == "open":
            depth[H // 6:H // 3, W // 16:W // 16 + W // 4] = 0.0
        else:
            cam = removed @ w2cs[t][:3, :3].T + w2cs[t][:3, 3]
            u, v = f * cam[:, 0] / cam[:, 2] + cx, f * cam[:, 1] / cam[:, 2] + cy
            u0, u1, v0, v1 = int(math.floor(u.min())), int(math.ceil(u.max())), int(math.floor(v.min())), int(math.ceil(v.max()))
            keep = depth[v0 + 14:v0 + 18, u0 + 14:u0 + 19].clone()
            depth[max(v0 - MARGIN, 0):v1 + MARGIN + 1, max(u0 - MARGIN, 0):u1 + MARGIN + 1] = 0.0
            if kind_t == "patch":
                assert v0 + 14 >= 0 and u0 + 14 >= 0 and bool((keep > 0).all()), "the patch lies inside the frame, on valid depth"
                depth[v0 + 14:v0 + 18, u0 + 14:u0 + 19] = keep
        frames.append((color, depth.contiguous()))
    _cache[key] = (params, frames, w2cs, ds.k)
    return _cache[key]


def case(name, device="cpu"):
    """(dataset, params, (mapping_iters, add_new_gaussians), eval_every) of golden case ``name``."""
    from tests.util import general_w2c
    kind, variant, every, general = CASES[name]
    params, frames, w2cs, k = scene_and_frames(kind, device)
    return HeldOutSplit(frames, w2cs, k, first_w2c=general_w2c() if general else None), params, variant, every
