"""float64 numpy restatement of the mesh layer (splatam_amd/csrc/tsdf_math.h), and the float32 numpy form of the same formulas.

Written from the definitions, not from the header: the update rule is vectorised over the whole grid, and the marching-tetrahedra
triangles are built geometrically -- each of Kuhn's six tetrahedra is walked edge by edge for a sign pattern and every triangle is
oriented by the cross product of its (midpoint) corners against the direction from the inside to the outside vertices -- so the
header's 16-row case table has something independent to agree with.

    VOLUME   p(i, j, k) = origin + voxel (i, j, k), x fastest; arrays [nz, ny, nx]
    UPDATE   ``integrate``: returns the new volume and, in float64, ``near``: the grid points whose decisions sit within rounding of a
             threshold (u + 0.5 or v + 0.5 within 1e-3 of an integer; pc.z, s - sil_thres, d - depth_max, sdf + trunc or sdf - trunc
             within 1e-5 of zero -- each only where the decisions before it let the point get that far).  A float32 evaluation may
             decide those differently; every other point must be decided alike.
    SURFACE  ``triangles``: [F, 3] vertex keys; ``vertices``: positions and colours of keys.
"""
import itertools

import numpy as np

PIXEL_MARGIN, VALUE_MARGIN = 1e-3, 1e-5
VOLUME_ARRAYS = ("tsdf", "weight", "r", "g", "b")


def rigid(axis, degrees, t):
    """4 x 4 float64 world-to-camera matrix: a rotation by ``degrees`` about ``axis`` (Rodrigues) and a translation."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = t
    return M


def new_volume(dims, dtype=np.float32):
    nx, ny, nz = dims
    vol = {k: np.zeros((nz, ny, nx), dtype=dtype) for k in VOLUME_ARRAYS}
    vol["tsdf"][:] = 1
    return vol


def grid_points(dims, origin, voxel, dtype):
    """x, y, z of every grid point, each [nz, ny, nx], evaluated in ``dtype`` as origin + voxel * index."""
    nx, ny, nz = dims
    o, vx = np.asarray(origin, dtype=dtype), dtype(voxel)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return o[0] + vx * i.astype(dtype), o[1] + vx * j.astype(dtype), o[2] + vx * k.astype(dtype)


def integrate(vol, dims, origin, voxel, trunc, out6, w2c, intr, sil_thres=0.99, depth_max=0.0, weight_max=0.0, dtype=np.float64):
    """One view into ``vol`` (a dict of [nz, ny, nx] arrays, not modified).  Every input is first rounded to float32 -- what the device
    holds -- and then every step is taken in ``dtype``.  Returns ``(new volume in dtype, updated mask, near mask)``."""
    f = dtype
    with np.errstate(all="ignore"):
        x, y, z = grid_points(dims, np.asarray(origin, np.float32), np.float32(voxel), f)
        m = np.asarray(w2c, dtype=np.float32).astype(f).reshape(4, 4)
        fx, fy, cx, cy = (f(np.float32(v)) for v in intr)
        trunc, sil_thres, depth_max, weight_max = (f(np.float32(v)) for v in (trunc, sil_thres, depth_max, weight_max))
        planes = np.asarray(out6, dtype=np.float32).astype(f)
        H, W = planes.shape[1:]
        pcx = m[0, 0] * x + m[0, 1] * y + m[0, 2] * z + m[0, 3]
        pcy = m[1, 0] * x + m[1, 1] * y + m[1, 2] * z + m[1, 3]
        pcz = m[2, 0] * x + m[2, 1] * y + m[2, 2] * z + m[2, 3]
        near = np.abs(pcz) < VALUE_MARGIN
        ok = pcz > 0
        u = fx * pcx / pcz + cx
        v = fy * pcy / pcz + cy
        uh, vh = u + f(0.5), v + f(0.5)
        uf, vf = np.floor(uh), np.floor(vh)
        near |= ok & ((np.abs(uh - np.round(uh)) < PIXEL_MARGIN) | (np.abs(vh - np.round(vh)) < PIXEL_MARGIN))
        ok &= (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
        ui = np.where(ok, uf, 0).astype(np.int64)
        vi = np.where(ok, vf, 0).astype(np.int64)
        s = planes[4][vi, ui]
        near |= ok & (np.abs(s - sil_thres) < VALUE_MARGIN)
        ok &= s > sil_thres
        d = planes[3][vi, ui] / s
        ok &= d > 0
        if depth_max > 0:
            near |= ok & (np.abs(d - depth_max) < VALUE_MARGIN)
            ok &= d <= depth_max
        sdf = d - pcz
        near |= ok & ((np.abs(sdf + trunc) < VALUE_MARGIN) | (np.abs(sdf - trunc) < VALUE_MARGIN))
        ok &= ~(sdf < -trunc)
        val = np.minimum(f(1), sdf / trunc)
        w0 = vol["weight"].astype(f)
        w1 = w0 + f(1)
        new = {"tsdf": np.where(ok, (vol["tsdf"].astype(f) * w0 + val) / w1, vol["tsdf"].astype(f))}
        for c, name in enumerate(("r", "g", "b")):
            colour = np.clip(planes[c][vi, ui] / s, 0, 1)
            new[name] = np.where(ok, (vol[name].astype(f) * w0 + colour) / w1, vol[name].astype(f))
        new["weight"] = np.where(ok, np.minimum(w1, weight_max) if weight_max > 0 else w1, w0)
    return new, ok, near


# ---------------------------------------------------------------------------------------------------------------- surface
def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def kuhn_tetrahedra():
    """The six tetrahedra of a cell as tuples of four corner numbers (dx + 2 dy + 4 dz) along c -> c + e_a -> c + e_a + e_b -> c + (1,1,1)."""
    return [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in itertools.permutations(range(3))]


def _tetrahedron_triangles(corners, inside):
    """Triangles of one tetrahedron (four corner numbers along its path; ``inside``: four booleans): each a list of three edges
    (corner, corner), oriented towards the outside vertices by geometry at the edges' midpoints."""
    ins = [v for v in range(4) if inside[v]]
    out = [v for v in range(4) if not inside[v]]
    if not ins or not out:
        return []
    if len(ins) == 1 or len(out) == 1:
        apex = ins[0] if len(ins) == 1 else out[0]
        tris = [[(min(apex, v), max(apex, v)) for v in range(4) if v != apex]]
    else:
        (a, b), (c, d) = ins, out                       # the quadrilateral ac, ad, bd, bc, split along ac - bd
        e = [tuple(sorted(p)) for p in ((a, c), (a, d), (b, d), (b, c))]
        tris = [[e[0], e[1], e[2]], [e[0], e[2], e[3]]]
    pos = [corner_offset(c).astype(float) for c in corners]
    towards = np.mean([pos[v] for v in out], axis=0) - np.mean([pos[v] for v in ins], axis=0)
    result = []
    for tri in tris:
        p = [(pos[i] + pos[j]) / 2 for i, j in tri]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert abs(n @ towards) > 1e-9
        if n @ towards < 0:
            tri = [tri[0], tri[2], tri[1]]
        result.append([(corners[i], corners[j]) for i, j in tri])
    return result


_PATTERNS = {}


def cell_pattern(mask):
    """Triangles of a cell whose corner c is inside when bit c of ``mask`` is set: a list of triangles, each three (corner a, corner b)
    edges with a below b along the tetrahedron's path (so a's offsets are a subset of b's)."""
    if mask not in _PATTERNS:
        tris = []
        for corners in kuhn_tetrahedra():
            tris += _tetrahedron_triangles(corners, [bool((mask >> c) & 1) for c in corners])
        _PATTERNS[mask] = tris
    return _PATTERNS[mask]


def linear(dims, i, j, k):
    return (k * dims[1] + j) * dims[0] + i


def edge_key(dims, cell, ca, cb):
    a = np.asarray(cell) + corner_offset(ca)
    return int(linear(dims, *a)) * 8 + (cb & ~ca)


def decode_key(dims, key):
    """(grid point a, grid point b) of a key."""
    l, d = key >> 3, key & 7
    a = np.array([l % dims[0], (l // dims[0]) % dims[1], l // (dims[0] * dims[1])])
    return a, a + corner_offset(d)


def triangles(tsdf, weight, min_weight=1.0):
    """[F, 3] int64 keys of the volume's surface (arrays [nz, ny, nx]; a corner is inside when tsdf < 0), in cell order."""
    nz, ny, nx = tsdf.shape
    dims = (nx, ny, nz)
    inside, seen = tsdf < 0, weight >= min_weight
    mask = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int64)
    ok = np.ones(mask.shape, dtype=bool)
    for c in range(8):
        dx, dy, dz = corner_offset(c)
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        mask |= inside[sl].astype(np.int64) << c
        ok &= seen[sl]
    mask[~ok] = 0
    out = []
    for k, j, i in zip(*np.nonzero((mask != 0) & (mask != 255))):
        for tri in cell_pattern(int(mask[k, j, i])):
            out.append([edge_key(dims, (i, j, k), ca, cb) for ca, cb in tri])
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def vertices(keys, vol, origin, voxel, dtype=np.float64):
    """Positions [n, 3] and colours [n, 3] of ``keys`` in ``dtype`` (inputs rounded to float32 first, as the device holds them)."""
    f = dtype
    nz, ny, nx = vol["tsdf"].shape
    dims = (nx, ny, nz)
    o, vx = np.asarray(origin, np.float32).astype(f), f(np.float32(voxel))
    keys = np.asarray(keys, dtype=np.int64)
    pos, col = np.zeros((len(keys), 3), dtype=f), np.zeros((len(keys), 3), dtype=f)
    for n, key in enumerate(keys):
        a, b = decode_key(dims, int(key))
        ia, ib = (a[2], a[1], a[0]), (b[2], b[1], b[0])
        fa, fb = f(vol["tsdf"][ia]), f(vol["tsdf"][ib])
        t = fa / (fa - fb)
        pa, pb = o + vx * a.astype(f), o + vx * b.astype(f)
        pos[n] = pa + t * (pb - pa)
        for c, name in enumerate(("r", "g", "b")):
            ca, cb = f(vol[name][ia]), f(vol[name][ib])
            col[n, c] = ca + t * (cb - ca)
    return pos, col


def canonical_triangles(keys):
    """A triangle list as a sorted list of key triples, each rotated to start with its smallest key (orientation kept)."""
    out = []
    for t in np.asarray(keys).reshape(-1, 3).tolist():
        r = t.index(min(t))
        out.append(tuple(t[r:] + t[:r]))
    return sorted(out)


def topology(faces):
    """(V, E, F, closed) of a triangle list: ``closed`` when every undirected edge is in exactly two triangles, once in each
    direction.  Degenerate triangles count like any other."""
    faces = np.asarray(faces).reshape(-1, 3)
    directed = {}
    for a, b, c in faces.tolist():
        for e in ((a, b), (b, c), (c, a)):
            directed[e] = directed.get(e, 0) + 1
    closed = all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
    undirected = {tuple(sorted(e)) for e in directed}
    return len(np.unique(faces)), len(undirected), len(faces), closed


def boundary_edges(faces):
    """Directed edges of a triangle list without their opposite."""
    directed = set()
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        directed.update(((a, b), (b, c), (c, a)))
    return [e for e in directed if (e[1], e[0]) not in directed]


def signed_volume(pos, faces):
    p = np.asarray(pos, dtype=np.float64)[np.asarray(faces).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- test scenes
def plane_view(W=72, H=40, intr=(60.0, 58.0, 35.5, 19.25)):
    """out6 [6, H, W] float32 of the tilted plane d = 1.3 / (1 - 0.2 x + 0.1 y) (x, y: normalised pixel coordinates) in smooth
    colours; silhouette 1 except for a band below the threshold, with a zero-depth hole and a NaN pixel.  The depth plane holds
    depth x silhouette, as the composite leaves it."""
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xn, yn = (u - cx) / fx, (v - cy) / fy
    depth = 1.3 / (1 - 0.2 * xn + 0.1 * yn)
    sil = np.ones((H, W))
    sil[:, 50:56] = 0.97                    # below 0.99
    sil[5:9, 10:14] = 0.995                 # above it, and not 1: the division matters
    rgb = np.stack([0.5 + 0.4 * np.sin(0.2 * u), 0.5 + 0.4 * np.cos(0.15 * v), 0.3 + 0.01 * (u + v) / 2])
    out6 = np.zeros((6, H, W), dtype=np.float64)
    out6[:3] = rgb * sil
    out6[3] = depth * sil
    out6[4] = sil
    out6[5] = depth * depth * sil
    out6[3, 20:24, 30:35] = 0.0             # a hole: d = 0
    out6[3, 12, 40] = np.nan
    out6[0, 30, 5] = 1.7                    # a colour beyond 1: clamped
    return out6.astype(np.float32)


def sphere_field(dims, origin, voxel, centre=(0.013, 0.021, -0.017), radius=0.45):
    nx, ny, nz = dims
    x, y, z = grid_points(dims, np.asarray(origin, np.float64), np.float64(voxel), np.float64)
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def torus_field(dims, origin, voxel, centre=(0.013, 0.021, -0.017), R=0.4, r=0.15):
    x, y, z = grid_points(dims, np.asarray(origin, np.float64), np.float64(voxel), np.float64)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - R
    return np.sqrt(q * q + (z - centre[2]) ** 2) - r


def field_volume(field, colour=True):
    """A float32 volume dict around a distance field: weight 1 everywhere, colours a smooth function of position."""
    f = np.asarray(field)
    vol = {"tsdf": f.astype(np.float32), "weight": np.ones(f.shape, np.float32)}
    nz, ny, nx = f.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for name, a in (("r", i / nx), ("g", j / ny), ("b", k / nz)):
        vol[name] = (a if colour else np.zeros(f.shape)).astype(np.float32)
    return vol


# ---------------------------------------------------------------------------------------------------------------- the update check
UPDATE_DIMS, UPDATE_VOXEL, UPDATE_ORIGIN, UPDATE_TRUNC = (37, 21, 13), 0.05, (-0.913, -0.507, 0.811), 0.2
UPDATE_SIZE, UPDATE_INTR = (72, 40), (60.0, 58.0, 35.5, 19.25)
UPDATE_POSES = {
    "identity": rigid((0, 1, 0), 0.0, (0.0, 0.0, 0.0)),
    "tilted": rigid((0.3, 1.0, -0.2), 17.0, (0.1, -0.05, 0.15)),
    "oblique": rigid((1.0, 0.2, 0.5), -38.0, (0.3, 0.2, 0.1)),           # only ~6 % of the grid points fall in the image
    "behind": rigid((0, 1, 0), 180.0, (0.0, 0.0, 0.0)),                  # nothing is updated
}
MAX_LEFT_OUT = 0.02


UPDATE_GRID = dict(origin=UPDATE_ORIGIN, voxel=UPDATE_VOXEL, trunc=UPDATE_TRUNC, intr=UPDATE_INTR)


def run_views(dims, poses, out6, dtype, grid=None, **kw):
    """``poses`` one after the other into a fresh volume with ``integrate`` in ``dtype``: (volume, union of the near masks).  ``out6``:
    one set of planes for every pose, or a list with one per pose; ``grid``: origin, voxel, trunc, intr (default the update check's)."""
    g = grid or UPDATE_GRID
    vol = new_volume(dims, dtype)
    near = np.zeros(vol["tsdf"].shape, dtype=bool)
    for n, w2c in enumerate(poses):
        planes = out6[n] if isinstance(out6, (list, tuple)) else out6
        vol, _, m = integrate(vol, dims, g["origin"], g["voxel"], g["trunc"], planes, w2c, g["intr"], dtype=dtype, **kw)
        near |= m
    return vol, near


def check_update(got, dims, poses, out6, what, grid=None, max_left_out=MAX_LEFT_OUT, **kw):
    """``got`` (a dict of float32 [nz, ny, nx] arrays: some float32 evaluation of ``poses`` into a fresh volume) against the float64
    restatement: at most ``max_left_out`` of the grid points sit within rounding of a threshold and are left out; on every other point
    the weight is EQUAL (the same decisions) and tsdf / r / g / b are within 4 x the float32 numpy form's own largest error on those
    points.  Returns the figures."""
    ref64, near = run_views(dims, poses, out6, np.float64, grid, **kw)
    ref32, _ = run_views(dims, poses, out6, np.float32, grid, **kw)
    keep = ~near
    figures = {"left_out": float(near.mean()), "updated": float((ref64["weight"] > 0).mean())}
    assert figures["left_out"] <= max_left_out, (what, figures)
    for name in VOLUME_ARRAYS:
        own = float(np.abs(ref32[name].astype(np.float64) - ref64[name])[keep].max())
        err = float(np.abs(np.asarray(got[name], dtype=np.float64) - ref64[name])[keep].max())
        figures[name] = (err, own)
    print(f"\n{what}: " + ", ".join(f"{k} {v}" for k, v in figures.items()))
    assert np.array_equal(np.asarray(got["weight"], dtype=np.float64)[keep], ref64["weight"][keep]), (what, "decisions differ")
    for name in VOLUME_ARRAYS:
        err, own = figures[name]
        assert err <= 4 * own, (what, name, err, own)
    return figures


# ---------------------------------------------------------------------------------------------------------------- a PLY reader
def read_mesh_ply(path):
    """(vertices [V, 3] float32, colours [V, 3] uint8 or None, faces [F, 3] int32) of a binary little-endian PLY with float x, y, z,
    optional uchar red, green, blue and ``list uchar int vertex_indices`` faces: parsed from the header it finds, byte by byte."""
    import struct
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    elements, current = [], None
    for line in lines[2:]:
        words = line.split()
        if words[:1] == ["element"]:
            current = (words[1], int(words[2]), [])
            elements.append(current)
        elif words[:1] == ["property"]:
            current[2].append(tuple(words[1:]))
    assert [e[0] for e in elements] == ["vertex", "face"], elements
    (_, nv, vprops), (_, nf, fprops) = elements
    sizes = {"float": ("f", 4), "uchar": ("B", 1)}
    fmt = "<" + "".join(sizes[p[0]][0] for p in vprops)
    names = [p[1] for p in vprops]
    assert names[:3] == ["x", "y", "z"] and fprops == [("list", "uchar", "int", "vertex_indices")], (vprops, fprops)
    stride = struct.calcsize(fmt)
    table = np.frombuffer(raw, dtype=np.dtype([(n, "<f4" if p[0] == "float" else "u1") for n, p in zip(names, vprops)]), count=nv, offset=end)
    assert table.dtype.itemsize == stride
    pos = np.stack([table["x"], table["y"], table["z"]], axis=1).astype(np.float32).reshape(-1, 3)
    col = np.stack([table["red"], table["green"], table["blue"]], axis=1).reshape(-1, 3) if names[3:] == ["red", "green", "blue"] else None
    faces = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=nf, offset=end + nv * stride)
    assert end + nv * stride + nf * 13 == len(raw), "trailing bytes"
    assert (faces["n"] == 3).all()
    return pos, col, faces["v"].astype(np.int32).reshape(-1, 3)
