"""Float64 numpy restatement of the view layer (splatam_amd/csrc/view_math.h, csrc/view.hip), shared by tests/test_view_math_cpu.py and
tests/test_gpu_view.py.  Inputs are what the kernels read (float32 planes and matrices), widened; every step is then float64.

V1: ``camera64`` is ``slam.setup_camera`` in float64 (P from the host numbers, (P w2c)^T, campos = -R^T t), ``rel_w2c64`` the relative
pose of a frame of the map as ``slam.transform_to_frame`` forms it.
V2: ``bytes64`` gives, per element, the byte (or table row) the definitions in include/splat_hip.h ask for AND the float64 value before
the rounding or truncation, so that ``check_bytes`` can apply the rule of the tests: equal wherever that value is farther than
``NEAR`` from a rounding / truncation boundary, off by at most one nearer than that, and at most ``MAX_NEAR_SHARE`` of the elements
that near.  ``cloud64`` is rgbd2pcd with the rigid inverse of the view's w2c."""
import numpy as np

NEAR = 1e-4
MAX_NEAR_SHARE = 1e-3
MODES = {"color": 0, "depth": 1, "sil": 2}


def camera_bound(t_norm):
    """Allowed |entry - float64| of V1's outputs: 4 * 2^-24 * (1 + |t|) (a dot product of three terms plus the sign)."""
    return 4.0 * 2.0 ** -24 * (1.0 + float(t_norm))


def rigid(axis, degrees, t):
    """Row-major float32 4 x 4 of a rotation about ``axis`` followed by the translation ``t`` (rounded to float32: what the kernel reads)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    m[:3, 3] = t
    return m.astype(np.float32)


def rel_w2c64(q_raw, t):
    """normalize(q_raw) -> build_rotation (which normalises once more) -> [R | t]."""
    q = np.asarray(q_raw, dtype=np.float64)
    q = q / max(np.linalg.norm(q), 1e-12)
    q = q / np.linalg.norm(q)
    r, x, y, z = q
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                 [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                 [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = np.asarray(t, dtype=np.float64)
    return m


def camera64(w2c, w, h, fx, fy, cx, cy, near=0.01, far=100.0, offset=None):
    """The four outputs of splat_view_camera in float64, in the library's layouts (viewmatrix / projmatrix: element (r, c) at [c*4+r])."""
    M = np.asarray(w2c, dtype=np.float64).reshape(4, 4)
    if offset is not None:
        M = np.asarray(offset, dtype=np.float64).reshape(4, 4) @ M
    P = np.array([[2 * fx / w, 0.0, -(w - 2 * cx) / w, 0.0],
                  [0.0, 2 * fy / h, -(h - 2 * cy) / h, 0.0],
                  [0.0, 0.0, far / (far - near), -(far * near) / (far - near)],
                  [0.0, 0.0, 1.0, 0.0]])
    return {'w2c': M.reshape(-1), 'viewmatrix': M.T.reshape(-1), 'projmatrix': (P @ M).T.reshape(-1), 'campos': -(M[:3, :3].T @ M[:3, 3])}


def seeded_planes(W, H, seed, lo=-0.1, hi=1.1, depth_lo=-0.5, depth_hi=7.0):
    """out6 [6, H, W] float32: r, g, b, silhouette uniform in lo..hi, depth in depth_lo..depth_hi, depth^2."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, size=(6, H, W))
    o[3] = rng.uniform(depth_lo, depth_hi, size=(H, W))
    o[5] = o[3] ** 2
    return o.astype(np.float32)


def _clip01(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0.0, np.clip(x, 0.0, 1.0))


def colour64(out6, bg):
    """[H, W, 3] float64: clip(rgb + (1 - silhouette) bg, 0, 1), NaN -> 0."""
    o = np.asarray(out6, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = o[0:3] + (1.0 - o[4])[None] * np.asarray(bg, dtype=np.float64)[:, None, None]
    return _clip01(c).transpose(1, 2, 0)


def bytes64(out6, mode, bg=(0.0, 0.0, 0.0), vmin=0.0, vmax=6.0):
    """(want, distance): ``want`` the bytes [H, W, 3] (colour, silhouette) or the table rows [H, W] (depth); ``distance`` how far the
    float64 value lies from the nearest boundary of its rounding (x.5) or truncation (integers; none for a value the clip made exact)."""
    o = np.asarray(out6, dtype=np.float64)
    if mode == "depth":
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            raw = (o[3] - np.float64(np.float32(vmin))) / (np.float64(np.float32(vmax)) - np.float64(np.float32(vmin)))
        v = _clip01(raw) * 255.0
        frac = v - np.floor(v)
        clipped = np.isnan(raw) | (raw <= 0.0) | (raw >= 1.0)
        return np.floor(v).astype(np.int64), np.where(clipped, np.inf, np.minimum(frac, 1.0 - frac))
    if mode == "sil":
        with np.errstate(invalid="ignore"):
            v = np.repeat(_clip01(1.0 - o[4])[:, :, None], 3, axis=2) * 255.0
    else:
        v = colour64(out6, bg) * 255.0
    return np.rint(v).astype(np.int64), np.abs(v - np.floor(v) - 0.5)


def check_bytes(got, out6, mode, bg=(0.0, 0.0, 0.0), vmin=0.0, vmax=6.0, lut=None, what=""):
    """The rule of the issue on ``got`` [H, W, 3] uint8; returns the share of elements within NEAR of a boundary."""
    want, dist = bytes64(out6, mode, bg, vmin, vmax)
    got = np.asarray(got).astype(np.int64)
    near = dist <= NEAR
    if mode == "depth":
        lut = np.asarray(lut).astype(np.int64)
        exact = (got == lut[want]).all(axis=2)
        one_off = exact | (got == lut[np.clip(want - 1, 0, 255)]).all(axis=2) | (got == lut[np.clip(want + 1, 0, 255)]).all(axis=2)
    else:
        exact, one_off = got == want, np.abs(got - want) <= 1
    share = float(near.mean())
    print(f"{what} {mode}: {int(near.sum())} of {near.size} elements within {NEAR} of a boundary, {int((~exact).sum())} differ")
    assert exact[~near].all(), (what, mode, np.argwhere(~exact & ~near)[:5])
    assert one_off[near].all(), (what, mode)
    assert share <= MAX_NEAR_SHARE, (what, mode, share)
    return share


def cloud64(out6, w2c, fx, fy, cx, cy, bg=(0.0, 0.0, 0.0)):
    """(points, colors) [H W, 3] float64: rgbd2pcd with the rigid inverse [R^T | -R^T t] of ``w2c``; colours as colour mode shows them."""
    o = np.asarray(out6, dtype=np.float64)
    H, W = o.shape[1:]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = o[3]
    cam = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z, np.ones_like(z)], axis=-1).reshape(-1, 4)
    M = np.asarray(w2c, dtype=np.float64).reshape(4, 4)
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = M[:3, :3].T, -(M[:3, :3].T @ M[:3, 3])          # the RIGID inverse: what the definition names
    return (cam @ c2w.T)[:, :3], colour64(out6, bg).reshape(-1, 3)


def cloud_torch32(out6, w2c, fx, fy, cx, cy):
    """The torch float32 form of the reference's rgbd2pcd on the same planes (tensors on any device): points [H W, 3]."""
    import torch
    H, W = out6.shape[1:]
    dev = out6.device
    xx = torch.tile(torch.arange(W, device=dev), (H,))
    yy = torch.repeat_interleave(torch.arange(H, device=dev), W)
    xx = (xx - cx) / fx
    yy = (yy - cy) / fy
    z = out6[3].reshape(-1)
    pts4 = torch.cat((torch.stack((xx * z, yy * z, z), dim=-1), torch.ones(H * W, 1, device=dev)), dim=1)
    c2w = torch.inverse(w2c.float())
    return (c2w @ pts4.T).T[:, :3]
