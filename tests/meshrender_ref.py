"""numpy float64 restatement of the mesh render layer (splatam_amd/csrc/meshrender_math.h), the yardstick of
tests/test_meshrender_cpu.py and tests/test_gpu_meshrender.py:

  * a brute-force ray caster: every pixel's ray against every triangle, with the flags of the pixels the oracle itself finds FRAGILE
    (a triangle that would set or change the pixel's depth has a barycentric coordinate within 1e-4 of zero there);
  * brute-force seen counts, with the flags of the vertices whose decision lies within rounding of a boundary;
  * closed forms (a box and a sphere seen from inside) and the cases both test files run."""
import functools

import numpy as np

import meshscore_ref as S

TOL_BARY = 1e-4         # a barycentric coordinate this close to zero: a silhouette edge passes within rounding of the pixel centre
TOL_PIXEL = 1e-4        # a projected coordinate this close to a rounding boundary (pixels)
TOL_DEPTH = 1e-6        # z this close (relative) to d + eps
MAX_EXCUSED = 0.01      # at most this share of a case's pixels / vertices may be excused
# |z32 - z64| / z64 of the header against the ray caster: 4 x the largest value observed over `render_cases` on the host
# (profiles/mesh_render.md 1: the observed value and where it occurs)
Z_OBSERVED = 5.5421e-07    # box-inside-96x64, at a grazing wall
Z_BOUND = 4 * Z_OBSERVED


def look_at(origin, target, up=(0.0, 0.0, 1.0), roll=0.0):
    """float32 w2c [4, 4] of a camera at ``origin`` looking at ``target`` (x right, y down, z forward), rolled about its axis."""
    o, t, u = (np.asarray(a, dtype=np.float64) for a in (origin, target, up))
    z = (t - o) / np.linalg.norm(t - o)
    x = np.cross(z, u)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross(z, np.array([1.0, 0.0, 0.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    x, y = c * x + s * y, -s * x + c * y
    M = np.eye(4)
    M[:3, :3] = np.stack((x, y, z))
    M[:3, 3] = -M[:3, :3] @ o
    return M.astype(np.float32)


def rotated(origin, angle, axis):
    """float32 w2c of a camera at ``origin`` whose orientation is the rotation by ``angle`` about ``axis`` (Rodrigues)."""
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = -R @ np.asarray(origin, dtype=np.float64)
    return M.astype(np.float32)


def pinhole(W, H, f):
    """(fx, fy, cx, cy) as float32 values: a principal point that puts no symmetric vertex on a pixel centre."""
    return tuple(float(np.float32(v)) for v in (f, f * 1.013, W / 2 - 0.37, H / 2 - 0.41))


def _valid_faces(vertices, faces):
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    ok[ok] = np.isfinite(v[f[ok]]).all(axis=(1, 2))
    return v, f[ok]


def rays(intr, size):
    fx, fy, cx, cy = intr
    W, H = size
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.stack(((i - cx) / fx, (j - cy) / fy, np.ones_like(i)), axis=-1).reshape(-1, 3)


def raycast(vertices, faces, w2c, intr, size, near=0.01, chunk=256):
    """(depth float64 [H, W] with 0 where no triangle is met, fragile bool [H, W]): every ray against every triangle in float64."""
    v, f = _valid_faces(vertices, faces)
    M = np.asarray(w2c, dtype=np.float64).reshape(4, 4)
    pc = v @ M[:3, :3].T + M[:3, 3] if len(v) else v
    W, H = size
    d = rays(intr, size)
    depth, fragile = np.zeros(W * H), np.zeros(W * H, dtype=bool)
    if len(f) == 0:
        return depth.reshape(H, W), fragile.reshape(H, W)
    A, B, C = pc[f[:, 0]], pc[f[:, 1]], pc[f[:, 2]]
    planes = (np.cross(B, C), np.cross(C, A), np.cross(A, B))             # barycentrics of A, B, C: d . plane / d . n
    n = np.cross(B - A, C - A)
    na = (n * A).sum(axis=1)
    for s in range(0, len(d), chunk):
        r = d[s:s + chunk]
        den = r @ n.T
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = np.stack([(r @ p.T) / den for p in planes])             # [3, P, F]
            z = na[None, :] / den
        lo = np.nan_to_num(lam.min(axis=0), nan=-np.inf)
        alive = np.isfinite(z) & (z >= near)
        hit = alive & (lo >= 0)
        zz = np.where(hit, z, np.inf).min(axis=1)
        depth[s:s + chunk] = np.where(np.isfinite(zz), zz, 0.0)
        close = (lo >= -TOL_BARY) & (lo < TOL_BARY) & alive & (z <= zz[:, None] * (1 + 1e-9))
        fragile[s:s + chunk] = close.any(axis=1)
    return depth.reshape(H, W), fragile.reshape(H, W)


def seen_counts(vertices, w2c, intr, size, edge=0, depth=None, eps=0.0):
    """(counts int64 [V], excused bool [V]): the seen predicate in float64 over all views; ``depth`` [n, H, W] are the planes AS GIVEN
    (float32 values).  A vertex is excused when, in some view, a projected coordinate lies within TOL_PIXEL of a rounding boundary (the
    image's margin is one) or z within TOL_DEPTH (relative) of d + eps."""
    v = np.asarray(vertices, dtype=np.float64)
    Ms = np.asarray(w2c, dtype=np.float64).reshape(-1, 4, 4)
    fx, fy, cx, cy = intr
    W, H = size
    counts, excused = np.zeros(len(v), dtype=np.int64), np.zeros(len(v), dtype=bool)
    for k, M in enumerate(Ms):
        pc = v @ M[:3, :3].T + M[:3, 3]
        z = pc[:, 2]
        front = z > 0
        zs = np.where(front, z, 1.0)
        u, w = fx * pc[:, 0] / zs + cx + 0.5, fy * pc[:, 1] / zs + cy + 0.5
        i, j = np.floor(u), np.floor(w)
        inside = front & (i >= edge) & (i <= W - 1 - edge) & (j >= edge) & (j <= H - 1 - edge)
        near_edge = front & ((np.abs(u - np.round(u)) < TOL_PIXEL) | (np.abs(w - np.round(w)) < TOL_PIXEL))
        fragile = near_edge & (i >= edge - 1) & (i <= W - edge) & (j >= edge - 1) & (j <= H - edge)
        ok = inside
        if depth is not None:
            plane = np.asarray(depth[k], dtype=np.float64)
            dd = plane[np.clip(j, 0, H - 1).astype(int), np.clip(i, 0, W - 1).astype(int)]
            ok = inside & (dd > 0) & (z <= dd + eps)
            fragile |= inside & (dd > 0) & (np.abs(z - (dd + eps)) <= TOL_DEPTH * np.abs(dd + eps))
        counts += ok
        excused |= fragile
    return counts, excused


# ---------------------------------------------------------------------------------------------------------------- closed forms
def world_rays(w2c, intr, size):
    """(origin [3], directions [H W, 3]) in the world: a point at camera depth z along ray k is origin + z directions[k]."""
    M = np.asarray(w2c, dtype=np.float64).reshape(4, 4)
    R, t = M[:3, :3], M[:3, 3]
    return -R.T @ t, rays(intr, size) @ R


def box_depth(lo, hi, w2c, intr, size):
    """Depth [H, W] of the inside of the box lo .. hi from a camera inside it: the smallest positive ray-plane hit over the six planes."""
    o, d = world_rays(w2c, intr, size)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.concatenate(((np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d), axis=1)
    return np.where(t > 0, t, np.inf).min(axis=1).reshape(size[1], size[0])


def sphere_depth(r, w2c, intr, size, centre=(0.0, 0.0, 0.0), first=False):
    """Depth [H, W] at which each ray meets the sphere: the far root (a camera inside) or, ``first``, the near one (inf: a miss)."""
    o, d = world_rays(w2c, intr, size)
    o = o - np.asarray(centre, dtype=np.float64)
    a, b, c = (d * d).sum(axis=1), (d * o).sum(axis=1), o @ o - r * r
    disc = b * b - a * c
    root = np.sqrt(np.where(disc >= 0, disc, np.nan))
    t = (-b - root) / a if first else (-b + root) / a
    return np.where(np.isfinite(t) & (t > 0), t, np.inf).reshape(size[1], size[0])


def inscribed_radius(vertices, faces, centre=(0.0, 0.0, 0.0)):
    """The least distance from ``centre`` to a face's plane: the sphere about it that the (convex) mesh contains."""
    v, f = np.asarray(vertices, dtype=np.float64) - np.asarray(centre), np.asarray(faces, dtype=np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return float(np.abs((n * v[f[:, 0]]).sum(axis=1) / np.linalg.norm(n, axis=1)).min())


def grid_cube(nx=6, ny=4, nz=4, cell=0.1, origin=(-0.3, -0.2, -0.2)):
    """(vertices float32, faces int32, colors float32): the surface of a box of nx x ny x nz grid squares, two triangles each."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    dims = (nx, ny, nz)
    for axis in range(3):
        a, b = [k for k in range(3) if k != axis]
        for side in (0, dims[axis]):
            for i in range(dims[a]):
                for j in range(dims[b]):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[a], p[b] = side, i + di, j + dj
                        q.append(vid(tuple(p)))
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    v = (np.array(verts, dtype=np.float64) * cell + np.asarray(origin)).astype(np.float32)
    colors = (np.array(verts, dtype=np.float32) / np.array(dims, dtype=np.float32)).astype(np.float32)
    return v, np.array(faces, dtype=np.int32), colors


def ring_views(n, radius, centre=(0.0, 0.0, 0.0), height=0.13, phase=0.21):
    """[n, 4, 4] float32: cameras on a ring about ``centre``, looking inward, each rolled a little differently."""
    c = np.asarray(centre, dtype=np.float64)
    out = []
    for k in range(n):
        a = phase + 2 * np.pi * k / n
        o = c + np.array([radius * np.cos(a), radius * np.sin(a), height])
        out.append(look_at(o, c, roll=0.1 + 0.37 * k))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------- the cases
BOX_SIDES, BOX_ORIGIN = S.BOX, (-0.3, 0.2, 0.1)
SPHERE_R = 0.45
NEAR = 0.01


@functools.lru_cache(maxsize=None)
def sphere():
    return S.sphere_mesh(5, SPHERE_R)


@functools.lru_cache(maxsize=None)
def box():
    return S.box_mesh(BOX_SIDES, BOX_ORIGIN, zero_area=False)


def box_inside_view():
    return rotated((0.27, 0.5, 0.33), 0.7331, (1.0, 2.0, 3.0))


def sphere_inside_view():
    return rotated((0.11, -0.07, 0.05), 1.1173, (3.0, -1.0, 2.0))


def sphere_outside_view():
    d = np.array([0.48, -0.61, 0.63])
    return look_at(-2.0 * d / np.linalg.norm(d), (0.0, 0.0, 0.0), roll=0.2931)


SIZES = {(96, 64): 80.0, (67, 45): 57.0}                               # size -> focal length: multiples of neither 16 nor 64


def render_cases():
    """name -> (vertices, faces, w2c, intrinsics, size): what both test files render."""
    cases = {}
    for size, f in SIZES.items():
        tag = f"{size[0]}x{size[1]}"
        cases[f"box-inside-{tag}"] = (*box(), box_inside_view(), pinhole(*size, f * 0.6), size)
        cases[f"sphere-inside-{tag}"] = (*sphere(), sphere_inside_view(), pinhole(*size, f * 0.6), size)
        cases[f"sphere-outside-{tag}"] = (*sphere(), sphere_outside_view(), pinhole(*size, f), size)
    return cases


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The ray caster's (depth, fragile) of a case: computed once, shared, never changed (read-only arrays)."""
    v, f, w2c, intr, size = render_cases()[name]
    depth, fragile = raycast(v, f, w2c, intr, size, NEAR)
    depth.setflags(write=False)
    fragile.setflags(write=False)
    return depth, fragile
