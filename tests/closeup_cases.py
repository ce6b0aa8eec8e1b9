"""The walk-through scene (CPU side; nothing here imports the GPU package at module level): a camera 1.2 m INSIDE a map that stays
where it was made, with footprints six times the projective size -- what a SplaTAM run shows once the camera has walked into the
map: Gaussians slide past the image border at z = 0.2 .. 0.5 m and fill a quarter of the frame.

Every other scene of the suite moves its map with its camera (tests/util.py: scene), so no Gaussian of theirs that carries a
gradient has its view-space centre outside the 1.3 tan(fov) guard band: a splat centred there needs a radius of 0.15 W to touch a
pixel.  Here such rows exist by the dozen and carry the LARGEST means3D / scales gradients of the frame.  The rows are grouped, in
float64, by what the projection does to them:

  clamp_x / clamp_y / clamp_both   live rows whose centre is clamped in x / in y / in both (splat_math.h ewa_setup: the clamped
                                   tx, ty enter the Jacobian and xmul / ymul mask dL/dtx, dL/dty in the adjoint)
  near                             live rows with 0.2 < z < 0.4
  behind                           rows with z <= 0.2 (culled: no radius, no gradient)
  wide                             rows whose radius exceeds the image width (tile rectangles clamped on up to four sides)
  plain                            live rows in none of the groups above

"live": any non-zero gradient in the float64 oracle.  A gradient check PER GROUP (groupwise_excess) bounds every row by 1e-3 of its
own group's maximum, so a wrong mask cannot hide under a tolerance taken from another group's rows."""
import functools
import math

import numpy as np
import torch

from oracle import c_ref
from oracle import raster_ref as R
from tests.util import rigid_w2c

SCALE_FACTOR = 6.0
WALK_ANGLE_DEG, WALK_AXIS, WALK_T = 12.0, (0.2, 1.0, 0.1), (0.2, 0.03, -1.2)
OFF_ANGLE_DEG, OFF_T = 0.4, (0.01, -0.005, 0.005)           # the frame of the engine case is rendered this far off the pose
GROUPS = ("clamp_x", "clamp_y", "clamp_both", "near", "behind", "wide", "plain")
MIN_ROWS = dict(clamp_x=20, clamp_y=20, clamp_both=20, near=20, wide=10)
GRAD_KEYS = ("means3D", "means2D", "colors", "opacities", "scales", "rotations")       # the C oracle's names

# (n, W, H, f, seed, anisotropic): the cells the GPU tests use -- tests/test_closeup_cases_cpu.py asserts on each what the GPU
# tests rely on (group sizes, the fast-path condition, the reference's own error)
CELLS = ((3000, 160, 112, 150.0, 5, False), (3000, 160, 112, 150.0, 5, True))


def walk_w2c(extra_deg=0.0, extra_t=(0.0, 0.0, 0.0)):
    return rigid_w2c(math.radians(WALK_ANGLE_DEG + extra_deg), WALK_AXIS, tuple(a + b for a, b in zip(WALK_T, extra_t)))


def walk_quat(extra_deg=0.0):
    """(w, x, y, z) of the rotation of walk_w2c."""
    a = np.asarray(WALK_AXIS, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(WALK_ANGLE_DEG + extra_deg) / 2
    return np.concatenate([[math.cos(h)], math.sin(h) * a])


def gout_planes(W, H, seed=1):
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed))


def oracle_run(cam, rv, gout, precision):
    """One forward + backward of the C oracle: (colour, radii, depth, gradients, CRef)."""
    cr = c_ref.CRef(precision)
    col, radii, dep = cr.forward(rv['means3D'].numpy(), rv['colors_precomp'].numpy(), rv['opacities'].numpy(), rv['scales'].numpy(),
                                 rv['rotations'].numpy(), cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.tanfovx, cam.tanfovy,
                                 cam.image_width, cam.image_height, cam.bg.numpy(), scale_modifier=cam.scale_modifier)
    return col, radii, dep, cr.backward(gout.numpy()), cr


def view_centres(means3D, w2c):
    """float64 view-space centres of float32 rows under a float32 matrix (both widened exactly)."""
    M = np.asarray(w2c, dtype=np.float32).astype(np.float64)
    return np.asarray(means3D, dtype=np.float64) @ M[:3, :3].T + M[:3, 3]


def row_groups(tv, radii, grads, W, tanfovx, tanfovy):
    """The boolean row masks of this module's docstring from float64 view-space centres ``tv`` [P, 3], the float64 oracle's radii and
    an iterable of its per-row gradient arrays."""
    P = tv.shape[0]
    live = np.zeros(P, dtype=bool)
    for g in grads:
        live |= (np.asarray(g).reshape(P, -1) != 0).any(axis=1)
    z = tv[:, 2]
    zs = np.where(z > 0.2, z, 1.0)
    cx = (z > 0.2) & (np.abs(tv[:, 0] / zs) > R.FOV_GUARD * tanfovx)
    cy = (z > 0.2) & (np.abs(tv[:, 1] / zs) > R.FOV_GUARD * tanfovy)
    groups = dict(clamp_x=live & cx, clamp_y=live & cy, clamp_both=live & cx & cy, near=live & (z > 0.2) & (z < 0.4),
                  behind=z <= 0.2, wide=np.asarray(radii) > W)
    special = np.zeros(P, dtype=bool)
    for m in groups.values():
        special |= m
    groups['plain'] = live & ~special
    return groups


@functools.lru_cache(maxsize=None)
def closeup_reference(n, W, H, f, seed, anisotropic):
    """The scene and both builds of the C oracle on it, computed once per process and shared (callers must not write into it):
    dict(cam, rv, gout, groups, f32 = (colour, radii, depth, grads, CRef), f64 = the same)."""
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    p = R.synthetic_cloud(n, W, H, f, f, cx, cy, seed=seed, anisotropic=anisotropic)
    p['log_scales'] = p['log_scales'] + math.log(SCALE_FACTOR)
    w2c = walk_w2c()
    cam = R.make_camera(W, H, f, f, cx, cy, w2c=w2c)
    rv = R.cloud_to_rendervar(p)
    gout = gout_planes(W, H)
    f32, f64 = oracle_run(cam, rv, gout, "f32"), oracle_run(cam, rv, gout, "f64")
    groups = row_groups(view_centres(rv['means3D'].numpy(), w2c), f64[1], [f64[3][k] for k in GRAD_KEYS], W, cam.tanfovx, cam.tanfovy)
    return dict(cam=cam, rv=rv, gout=gout, groups=groups, f32=f32, f64=f64)


def closeup_scene(n, W, H, f, seed, anisotropic):
    """(cam, rv, groups): the cloud of R.synthetic_cloud at the identity (NOT moved with the camera), scales x 6, seen from
    walk_w2c()."""
    ref = closeup_reference(n, W, H, f, seed, anisotropic)
    return ref['cam'], {k: v.clone() for k, v in ref['rv'].items()}, ref['groups']


def groupwise_excess(got, ref64, groups, rows_ok=None, rel=1e-3):
    """The project's 1e-3 gradient bound taken PER GROUP: for every group the largest |got - ref64| over its rows (those of
    ``rows_ok``, when given: rows not lying over a float32 decision flip) as a multiple of rel * max|ref64[group]| -- at most 1 where
    the bound holds.  Groups whose reference gradient is all zero (``behind``) are left to the caller's exact check.
    Returns {group: (factor, rows compared)}."""
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64).reshape(got.shape)
    P = got.shape[0]
    err = np.abs(got - ref64).reshape(P, -1).max(axis=1)
    out = {}
    for name, m in groups.items():
        gmax = float(np.abs(ref64[m]).max()) if m.any() else 0.0
        if gmax == 0.0:
            continue
        rows = m if rows_ok is None else m & rows_ok
        out[name] = (float(err[rows].max()) / (rel * gmax) if rows.any() else 0.0, int(rows.sum()))
    return out


def assert_groupwise(got, ref64, groups, rows_ok=None, what=""):
    ex = groupwise_excess(got, ref64, groups, rows_ok)
    print(f"{what}: largest error / (1e-3 x the group's max), rows compared: " + ", ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in ex.items()))
    bad = {k: v for k, v in ex.items() if v[0] > 1.0}
    assert not bad, f"{what}: beyond 1e-3 of the group's own maximum: {bad}"


def rows_clear_of(flagged, geom, radii):
    """Rows that lie over no pixel of the boolean image ``flagged`` (tests/util.py: flip_pixels).  A flipped decision at a pixel
    changes T for the Gaussians blended there, so "over" is taken from the float64 oracle's geometry (``geom`` = CRef.geom()): the row
    reaches that pixel with alpha >= 0.5 / 255, half the blend threshold.  (The bounding box centre +- radius of a splat wider than
    the frame covers every pixel: with that definition one flip anywhere would take all of ``wide`` out of the comparison.)"""
    ys, xs = np.nonzero(flagged)
    P = len(radii)
    if ys.size == 0:
        return np.ones(P, dtype=bool)
    xy, co = np.asarray(geom['xy'], dtype=np.float64), np.asarray(geom['conic_op'], dtype=np.float64)
    dx, dy = xy[:, 0:1] - xs[None, :], xy[:, 1:2] - ys[None, :]
    power = -0.5 * (co[:, 0:1] * dx * dx + co[:, 2:3] * dy * dy) - co[:, 1:2] * dx * dy
    alpha = co[:, 3:4] * np.exp(np.minimum(power, 0.0))
    over = (np.asarray(radii)[:, None] > 0) & (power <= 1e-3) & (alpha >= 0.5 / 255.0)
    return ~over.any(axis=1)


def closeup_engine_case(n, W, H, f, seed, anisotropic, device="cuda"):
    """The same map as a fused-engine case: slam.synthetic_params (the same draws as R.synthetic_cloud) with the same scale factor,
    the walk-through pose in cam_unnorm_rots / cam_trans [..., 1], and a frame rendered 0.4 deg / 1 cm off that pose with the noise
    and the invalid-depth patch of tests/util.py: multiview_scene.  Returns (params, variables, frame, cam, k, c)."""
    from splatam_amd import slam
    from tests.util import frame_at_pose
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    params, variables = slam.synthetic_params(n, W, H, f, f, cx, cy, num_frames=3, seed=seed, device=device, anisotropic=anisotropic)
    k = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    first = np.eye(4, dtype=np.float32)
    w2c = torch.tensor(first, device=device)
    cam = slam.setup_camera(W, H, k, first, device=device)
    with torch.no_grad():
        params['log_scales'] += math.log(SCALE_FACTOR)
        params['cam_unnorm_rots'][0, :, 1] = torch.as_tensor(walk_quat(), dtype=torch.float32, device=device)
        params['cam_trans'][0, :, 1] = torch.as_tensor(WALK_T, dtype=torch.float32, device=device)
    im, depth = frame_at_pose(params, cam, w2c, walk_quat(OFF_ANGLE_DEG), np.asarray(WALK_T) + np.asarray(OFF_T))
    g = torch.Generator().manual_seed(seed + 1)
    im = (im + 0.03 * torch.randn(im.shape, generator=g).to(device)).clamp(0, 1).contiguous()
    depth = (depth * (1 + 0.01 * torch.randn(depth.shape, generator=g).to(device))).contiguous()
    depth[:, : H // 8, : W // 8] = 0.0
    frame = {'cam': cam, 'im': im, 'depth': depth, 'id': 1, 'w2c': w2c}
    return params, variables, frame, cam, k, dict(n=n, W=W, H=H, fx=f, fy=f, cx=cx, cy=cy)


def engine_view_centres(params, time_idx=1):
    """float64 view-space centres of the engine case's rows at pose ``time_idx`` (first-frame matrix: the identity)."""
    q = params['cam_unnorm_rots'][0, :, time_idx].detach().double().cpu().numpy()
    t = params['cam_trans'][0, :, time_idx].detach().double().cpu().numpy()
    w, x, y, z = q / np.linalg.norm(q)
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return params['means3D'].detach().double().cpu().numpy() @ Rq.T + t
