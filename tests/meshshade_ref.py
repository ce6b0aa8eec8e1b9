"""numpy float64 restatement of the mesh shade layer (splatam_amd/csrc/meshshade_math.h), the yardstick of tests/test_meshshade_cpu.py:

  * area-weighted vertex normals by the header's definition WITHOUT its quantisation;
  * a ray caster that also names the nearest face and its barycentrics.  It is ``meshrender_ref.raycast``'s arithmetic -- every ray
    against every triangle that can matter -- made affordable at the supersampled sizes by testing, per tile of pixels, only the faces
    whose projected box (grown by two pixels) meets the tile; faces with a vertex at z <= near are tested everywhere, faces wholly
    behind the near plane nowhere.  Its depth and its fragile flags are asserted equal to ``meshrender_ref.oracle``'s at samples == 1;
  * the shading of one sub-sample and of a picture, with the flags of the pixels where the restatement itself sits on a decision
    (a depth-table index within 1e-4 of the next row, a camera-frame normal within 1e-4 of edge-on).

The cases are ``meshrender_ref.render_cases()`` as they stand, with seeded vertex colours, and ``meshrender_ref.grid_cube()``."""
import functools

import numpy as np

import meshrender_ref as R

MODES = ("color", "shaded", "shaded-color", "normal", "depth")
MODE_ID = {name: k for k, name in enumerate(MODES)}
TOL_DECISION = 1e-4
# the angle (radians) between the header's normals and the restatement's over the sphere, the box and the grid cube: 4 x the largest
# value observed on the host (tests/test_meshshade_cpu.py prints it; profiles/mesh_view.md 1).  The float32 rounding of a component.
ANGLE_OBSERVED = 3.9281e-08     # the sphere
ANGLE_BOUND = 4 * ANGLE_OBSERVED
# bytes: the largest |header - restatement| observed on the host over every case, mode, smooth and samples off the fragile pixels,
# plus 1 (printed by the test; profiles/mesh_view.md 1)
BYTES_OBSERVED = 1              # a value within rounding of a half-integer byte (every case has one)
B = BYTES_OBSERVED + 1

BG = (1.0, 0.5, 0.25)
ALBEDO = (0.8, 0.7, 0.6)
AMBIENT = 0.25
DEPTH_RANGE = (0.2, 3.1)


def supersampled(intr, size, s):
    """(intrinsics, size) of the key plane of ``s`` x ``s`` sub-pixels per pixel: fx s, fy s, (cx + 0.5) s - 0.5, cy alike (float64)."""
    fx, fy, cx, cy = (float(x) for x in intr)
    return (fx * s, fy * s, (cx + 0.5) * s - 0.5, (cy + 0.5) * s - 0.5), (int(size[0]) * s, int(size[1]) * s)


def vertex_colors(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_colors(name):
    v = R.render_cases()[name][0]
    return vertex_colors(len(v), 7 if name.startswith("box") else 11)


def vertex_normals(vertices, faces):
    """float64 [V, 3]: sum over the accepted faces of (b - a) x (c - a), normalised; zeros where the sum is zero."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    f = f[ok]
    f = f[np.isfinite(v[f]).all(axis=(1, 2))] if len(f) else f
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]) if len(f) else np.zeros((0, 3))
    keep = (np.abs(n) < 2.0 ** 22).all(axis=1)
    f, n = f[keep], n[keep]
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], n)
    length = np.linalg.norm(acc, axis=1)
    return np.where(length[:, None] > 0, acc / np.where(length > 0, length, 1.0)[:, None], 0.0)


def angles(a, b):
    """The angle between corresponding unit vectors (rows that are zero in both: 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    cross, dot = np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1)
    return np.where((np.abs(a).sum(axis=1) == 0) & (np.abs(b).sum(axis=1) == 0), 0.0, np.arctan2(cross, dot))


# ---------------------------------------------------------------------------------------------------------------- the ray caster
def _camera(vertices, faces, w2c):
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    M = np.asarray(w2c, dtype=np.float64).reshape(4, 4)
    return v @ M[:3, :3].T + M[:3, 3], f


def _face_terms(pc, f):
    A, B, C = pc[f[:, 0]], pc[f[:, 1]], pc[f[:, 2]]
    n = np.cross(B - A, C - A)
    return (np.cross(B, C), np.cross(C, A), np.cross(A, B)), n, (n * A).sum(axis=1)


def _against(r, planes, n, na, near):
    """(z [P, F], lo [P, F], lam [3, P, F], alive) of rays r [P, 3] against faces: meshrender_ref.raycast's expressions."""
    den = r @ n.T
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.stack([(r @ p.T) / den for p in planes])
        z = na[None, :] / den
    lo = np.nan_to_num(lam.min(axis=0), nan=-np.inf)
    return z, lo, lam, np.isfinite(z) & (z >= near)


def raycast_faces(vertices, faces, w2c, intr, size, near=R.NEAR, tile=8):
    """(depth [H, W] float64 with 0 for none, face [H, W] int64 with -1, lam [H, W, 3], fragile [H, W]): the nearest hit of every pixel's
    ray in float64; ties go to the lowest face index (they occur on fragile pixels only)."""
    pc, f = _camera(vertices, faces, w2c)
    W, H = size
    fx, fy, cx, cy = intr
    d = R.rays(intr, size).reshape(H, W, 3)
    depth, face, lam3 = np.zeros((H, W)), np.full((H, W), -1, dtype=np.int64), np.zeros((H, W, 3))
    fragile = np.zeros((H, W), dtype=bool)
    zs = pc[f][:, :, 2]                                                  # [F, 3]
    front = (zs > near).all(axis=1)
    behind = (zs < near - 1e-9).all(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * pc[f][:, :, 0] / zs + cx
        w = fy * pc[f][:, :, 1] / zs + cy
    ulo, uhi, wlo, whi = u.min(axis=1) - 2, u.max(axis=1) + 2, w.min(axis=1) - 2, w.max(axis=1) + 2
    everywhere = ~front & ~behind
    for j0 in range(0, H, tile):
        for i0 in range(0, W, tile):
            j1, i1 = min(j0 + tile, H), min(i0 + tile, W)
            pick = np.nonzero(everywhere | (front & (uhi >= i0) & (ulo <= i1 - 1) & (whi >= j0) & (wlo <= j1 - 1)))[0]
            if len(pick) == 0:
                continue
            r = d[j0:j1, i0:i1].reshape(-1, 3)
            planes, n, na = _face_terms(pc, f[pick])
            z, lo, lam, alive = _against(r, planes, n, na, near)
            hit = alive & (lo >= 0)
            zz = np.where(hit, z, np.inf)
            best = zz.argmin(axis=1)                                     # (the first minimum: the lowest index, `pick` is ascending)
            zmin = zz[np.arange(len(r)), best]
            found = np.isfinite(zmin)
            close = (lo >= -R.TOL_BARY) & (lo < R.TOL_BARY) & alive & (z <= zmin[:, None] * (1 + 1e-9))
            shape = (j1 - j0, i1 - i0)
            depth[j0:j1, i0:i1] = np.where(found, zmin, 0.0).reshape(shape)
            face[j0:j1, i0:i1] = np.where(found, pick[best], -1).reshape(shape)
            lam3[j0:j1, i0:i1] = np.where(found[:, None], lam[:, np.arange(len(r)), best].T, 0.0).reshape(*shape, 3)
            fragile[j0:j1, i0:i1] = close.any(axis=1).reshape(shape)
    return depth, face, lam3, fragile


def face_at(vertices, faces, w2c, intr, size, ids, near=R.NEAR):
    """(z [H, W], lo [H, W]) of the faces ``ids`` [H, W] (>= 0) at their own pixels: what the oracle makes of a named face."""
    pc, f = _camera(vertices, faces, w2c)
    W, H = size
    d = R.rays(intr, size)
    g = f[np.asarray(ids).reshape(-1)]
    A, B, C = pc[g[:, 0]], pc[g[:, 1]], pc[g[:, 2]]
    n = np.cross(B - A, C - A)
    den = (d * n).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.stack([(d * p).sum(axis=1) / den for p in (np.cross(B, C), np.cross(C, A), np.cross(A, B))])
        z = (n * A).sum(axis=1) / den
    return z.reshape(H, W), np.nan_to_num(lam.min(axis=0), nan=-np.inf).reshape(H, W)


@functools.lru_cache(maxsize=None)
def oracle(name, samples=1):
    """(depth, face, lam, fragile) of a case on its key plane of ``samples`` x ``samples`` sub-pixels per pixel: computed once, shared,
    read-only."""
    v, f, w2c, intr, size = R.render_cases()[name]
    intr_s, size_s = supersampled(intr, size, samples)
    out = raycast_faces(v, f, w2c, intr_s, size_s)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- shading
def shade(vertices, faces, colors, normals, w2c, intr, size, samples, face, lam, z_given, mode, smooth=True, normal_frame=0, bg=BG, albedo=ALBEDO,
          ambient=AMBIENT, depth_range=DEPTH_RANGE, lut=None):
    """(values [H, W, 3] float64 in 0..1 -- a byte is rint(255 value) --, decision [H, W] bool): the picture of ``size`` from the key plane's
    ``face`` / ``lam`` (of ``raycast_faces`` at the supersampled camera) and ``z_given`` (the depths AS GIVEN, for depth mode).  ``colors``
    / ``normals`` may be None (albedo / the faces' own normals)."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    intr_s, size_s = supersampled(intr, size, samples)
    Ws, Hs = size_s
    M = np.asarray(w2c, dtype=np.float64).reshape(4, 4)
    Rm = M[:3, :3]
    d = R.rays(intr_s, size_s)                                           # camera frame
    ids = face.reshape(-1)
    hit = ids >= 0
    g = f[np.where(hit, ids, 0)]
    lam = lam.reshape(-1, 3)                                             # of a, b, c

    def mix(x):
        return lam[:, 0:1] * x[g[:, 0]] + lam[:, 1:2] * x[g[:, 1]] + lam[:, 2:3] * x[g[:, 2]]

    colour = mix(np.asarray(colors, dtype=np.float64)) if colors is not None else np.broadcast_to(np.asarray(albedo, dtype=np.float64), (len(ids), 3))
    fn = np.cross(v[g[:, 1]] - v[g[:, 0]], v[g[:, 2]] - v[g[:, 0]])
    length = np.linalg.norm(fn, axis=1)
    n = np.where(length[:, None] > 0, fn / np.where(length > 0, length, 1.0)[:, None], 0.0)
    if smooth and normals is not None:
        s = mix(np.asarray(normals, dtype=np.float64))
        length = np.linalg.norm(s, axis=1)
        n = np.where(length[:, None] > 0, s / np.where(length > 0, length, 1.0)[:, None], n)
    decision = np.zeros(len(ids), dtype=bool)
    if mode == "color":
        val = colour
    elif mode in ("shaded", "shaded-color"):
        wr = d @ Rm                                                      # R^T d
        L = ambient + (1 - ambient) * np.abs((n * wr).sum(axis=1)) / np.linalg.norm(wr, axis=1)
        val = (np.asarray(albedo, dtype=np.float64)[None, :] if mode == "shaded" else colour) * L[:, None]
    elif mode == "normal":
        if normal_frame:
            nc = n @ Rm.T
            along = (nc * d).sum(axis=1)
            decision = hit & (np.abs(along) / np.linalg.norm(d, axis=1) < TOL_DECISION)
            n = np.where((along > 0)[:, None], -nc, nc)
        val = (n + 1) / 2
    else:
        raw = (np.asarray(z_given, dtype=np.float64).reshape(-1) - depth_range[0]) / (depth_range[1] - depth_range[0]) * 255
        x = np.clip(raw, 0, 255)
        decision = hit & (np.abs(raw - np.round(raw)) < TOL_DECISION) & (raw > -TOL_DECISION) & (raw < 255 + TOL_DECISION)
        val = np.asarray(lut, dtype=np.float64)[np.trunc(x).astype(int)] / 255.0
    val = np.where(hit[:, None], val, np.asarray(bg, dtype=np.float64)[None, :])
    W, H = size
    val = val.reshape(H, samples, W, samples, 3).mean(axis=(1, 3))
    decision = decision.reshape(H, samples, W, samples).any(axis=(1, 3))
    return np.clip(val, 0.0, 1.0), decision


def reduce_any(flags, samples):
    H, W = flags.shape[0] // samples, flags.shape[1] // samples
    return flags.reshape(H, samples, W, samples).any(axis=(1, 3))
