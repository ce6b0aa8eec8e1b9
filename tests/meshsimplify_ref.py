"""numpy restatement of the mesh simplification layer (splatam_amd/csrc/meshsimplify_math.h, splatam_amd/mesh_simplify.py): cell keys,
cluster ids, the per-cluster integer sums, the placement, the renamed faces and the compaction, plus the meshes the tests use.

KEYS    ``keys``: i = floor(x / cell) in double per axis, |i| < 2^20; (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20); -1 otherwise.
IDS     ``cluster_ids``: the rank of a key among the distinct keys >= 0, -1 for -1.
SUMS    ``sums``: the header's double products IN THE HEADER'S ORDER, so the int64 words must agree EXACTLY: per vertex rint(p 2^32) and
        rint(colour 2^32); per face and distinct cluster the ten rint(area {n n^T, d n, d^2} 2^40).
PLACE   ``place``: the same formula solved with ``numpy.linalg.eigh`` -- another eigensolver on the same integers, so positions agree to
        rounding, not to the bit.  It also flags a cluster as FRAGILE when some l_i / lmax lies in [tau / 2, 2 tau] or max |p_k| is within
        1e-6 of 1/2: rounding decides a branch there.
FACES   ``triples`` and ``compact``: the rotation, the optional removal of repeated triples (lowest input index stays) and the dense
        renumbering in ascending cluster id.
``simplify(..., shim=lib)`` drives the HOST BUILD OF THE HEADER (tests/meshsimplify_math_shim.cpp) through the same glue instead: what
the device must equal byte for byte.
"""
import ctypes as C

import numpy as np

LIMIT = 1 << 20
TAU = 1e-3
UNIT = 2.0 ** 32
AREA = 2.0 ** 40
SUMS = 16
F32P, I32P, I64P, F64P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def cell_index(x, cell):
    """(i float64, ok) per coordinate."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.floor(np.asarray(x, dtype=np.float32).astype(np.float64) / cell)
        ok = (q > -LIMIT) & (q < LIMIT)
    return np.where(ok, q, 0.0), ok


def keys(vertices, cell):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    i, ok = cell_index(v, cell)
    i = i.astype(np.int64) + LIMIT
    return np.where(ok.all(axis=1), (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0], -1).astype(np.int64)


def cluster_ids(k):
    k = np.asarray(k, dtype=np.int64)
    out = np.full(len(k), -1, dtype=np.int32)
    live = k >= 0
    if live.any():
        out[live] = np.unique(k[live], return_inverse=True)[1].astype(np.int32)
    return out


def cluster_keys(k, cluster):
    out = np.full(len(k), -1, dtype=np.int64)
    live = cluster >= 0
    out[cluster[live]] = k[live]
    return out


def local(v, cell):
    """p [n, 3] float64 of float32 vertices that have a key."""
    i, _ = cell_index(v, cell)
    x = v.astype(np.float64)
    return (x - (i + 0.5) * cell) / cell


def quanta(x, scale):
    return np.rint(x * scale).astype(np.int64)


def sums(vertices, faces, colors, cell, cluster, quadrics=True):
    """(count int32 [V], sums int64 [V, 16], refused, the |d| of every contribution)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    count, acc = np.zeros(V, dtype=np.int32), np.zeros((V, SUMS), dtype=np.int64)
    live = (cluster >= 0) & (cluster < V)
    g = cluster[live].astype(np.int64)
    np.add.at(count, g, 1)
    p = local(v[live], cell)
    for k in range(3):
        np.add.at(acc[:, k], g, quanta(p[:, k], UNIT))
    if colors is not None:
        c = np.asarray(colors, dtype=np.float32).reshape(-1, 3)[live]
        with np.errstate(invalid="ignore"):
            fine = (c > -2.0 ** 20) & (c < 2.0 ** 20)
        q = quanta(np.where(fine, c, 0).astype(np.float64), UNIT)
        for k in range(3):
            np.add.at(acc[:, 3 + k], g, q[:, k])
    ds, refused = np.zeros(0), 0
    if quadrics and len(f) and V:
        ok = ((f >= 0) & (f < V)).all(axis=1)
        fc = f[ok]
        cs = cluster[fc].astype(np.int64)
        ok2 = ((cs >= 0) & (cs < V)).all(axis=1)
        fc, cs = fc[ok2], cs[ok2]
        a, b, c = (v[fc[:, k]].astype(np.float64) for k in range(3))
        with np.errstate(over="ignore", invalid="ignore"):
            e1, e2 = b - a, c - a
            n = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), axis=1)
            length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            has = length > 0
            area = 0.5 * length
            within = area < 2.0 ** 22
        refused = int((has & ~within).any())
        use = has & within
        fc, cs, n, length, area = fc[use], cs[use], n[use], length[use], area[use]
        nh = n / length[:, None]
        w = area[:, None] * nh
        slot_live = (np.ones(len(fc), dtype=bool), cs[:, 1] != cs[:, 0], (cs[:, 2] != cs[:, 0]) & (cs[:, 2] != cs[:, 1]))
        all_d = []
        for k in range(3):
            s = slot_live[k]
            p = local(v[fc[s, k]], cell)
            nk, wk, ak = nh[s], w[s], area[s]
            d = (nk[:, 0] * p[:, 0] + nk[:, 1] * p[:, 1]) + nk[:, 2] * p[:, 2]
            terms = (wk[:, 0] * nk[:, 0], wk[:, 0] * nk[:, 1], wk[:, 0] * nk[:, 2], wk[:, 1] * nk[:, 1], wk[:, 1] * nk[:, 2], wk[:, 2] * nk[:, 2],
                     wk[:, 0] * d, wk[:, 1] * d, wk[:, 2] * d, (ak * d) * d)
            for j, t in enumerate(terms):
                np.add.at(acc[:, 6 + j], cs[s, k], quanta(t, AREA))
            all_d.append(np.abs(d))
        ds = np.concatenate(all_d)
    return count, acc, refused, ds


def place(count, acc, ckeys, cell, placement="quadric", colors=False):
    """dict by cluster: positions, colors (or None), rank, fallback, value, fragile, p (float64, local)."""
    V = len(count)
    live = (count > 0) & (ckeys >= 0)
    n = np.where(live, count, 1).astype(np.float64)
    m = acc[:, 0:3].astype(np.float64) * 2.0 ** -32 / n[:, None]
    col = (acc[:, 3:6].astype(np.float64) * 2.0 ** -32 / n[:, None]).astype(np.float32) if colors else None
    p = m.copy()
    rank, fallback = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
    value, fragile = np.zeros(V), np.zeros(V, dtype=bool)
    if placement == "quadric":
        s = acc.astype(np.float64) * 2.0 ** -40
        A = np.stack((s[:, [6, 7, 8]], s[:, [7, 9, 10]], s[:, [8, 10, 11]]), axis=1)
        b, c = s[:, 12:15], s[:, 15]
        lam, E = np.linalg.eigh(A)
        lmax = np.abs(lam).max(axis=1)
        some = lmax > 0
        ratio = lam / np.where(some, lmax, 1.0)[:, None]
        use = (ratio > TAU) & some[:, None]
        r = b - np.einsum("nij,nj->ni", A, m)
        coef = np.where(use, np.einsum("nji,nj->ni", E, r) / np.where(use, lam, 1.0), 0.0)
        q = m + np.einsum("nij,nj->ni", E, coef)
        inside = (np.abs(q) <= 0.5).all(axis=1)
        ok = some & inside
        p = np.where(ok[:, None], q, m)
        rank = np.where(ok, use.sum(axis=1), 0).astype(np.int32)
        fallback = (~ok).astype(np.int32)
        fragile = (((ratio >= TAU / 2) & (ratio <= 2 * TAU)).any(axis=1) | (np.abs(np.abs(q).max(axis=1) - 0.5) < 1e-6)) & some
        value = np.einsum("ni,nij,nj->n", p, A, p) - 2 * (b * p).sum(axis=1) + c
    idx = np.stack([((np.where(live, ckeys, 0) >> (21 * k)) & 0x1fffff) - LIMIT for k in range(3)], axis=1).astype(np.float64)
    pos = ((idx + 0.5) * cell + p * cell).astype(np.float32)
    pos[~live] = 0
    if col is not None:
        col[~live] = 0
    for a in (rank, fallback, value, fragile):
        a[~live] = 0
    return dict(positions=pos, colors=col, rank=rank, fallback=fallback, value=value, fragile=fragile, p=p, live=live)


def triples(faces, V, cluster):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    out = np.full((len(f), 3), -1, dtype=np.int32)
    if V == 0 or len(f) == 0:
        return out
    ok = ((f >= 0) & (f < V)).all(axis=1)
    g = cluster[np.clip(f, 0, V - 1)].astype(np.int64)
    ok &= (g >= 0).all(axis=1) & (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    shift = g.argmin(axis=1)
    rot = np.stack([g[np.arange(len(g)), (shift + k) % 3] for k in range(3)], axis=1)
    out[ok] = rot[ok]
    return out


def first_of_each(tri, keep):
    """keep without the faces whose triple a kept face of lower index has too."""
    t = np.asarray(tri, dtype=np.int64)
    idx = np.flatnonzero(keep)
    order = idx[np.lexsort((t[idx, 2], t[idx, 1], t[idx, 0]))]          # (stable: equal triples stay in input order)
    s = t[order]
    first = np.ones(len(order), dtype=bool)
    first[1:] = (s[1:] != s[:-1]).any(axis=1)
    out = np.zeros(len(t), dtype=bool)
    out[order[first]] = True
    return out


def compact(positions, colors, tri, keep):
    kept = tri[keep].astype(np.int64)
    used = np.zeros(len(positions), dtype=bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    return positions[used], renumber[kept].astype(np.int32).reshape(-1, 3), None if colors is None else colors[used]


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def load_shim():
    from tests.util import host_shim
    lib = host_shim("meshsimplify_math_shim", "meshsimplify_math.h", "meshclean_math.h", "meshscore_math.h", "icp_math.h")
    lib.sqs_keys.restype = None
    lib.sqs_keys.argtypes = [F32P, C.c_int32, C.c_double, I64P]
    lib.sqs_vertices.restype = None
    lib.sqs_vertices.argtypes = [F32P, F32P, C.c_int32, I32P, C.c_double, I32P, I64P]
    lib.sqs_quadrics.restype = C.c_double
    lib.sqs_quadrics.argtypes = [F32P, C.c_int32, I32P, C.c_int32, I32P, C.c_double, I64P, I32P, I64P]
    lib.sqs_place.restype = None
    lib.sqs_place.argtypes = [I32P, I64P, I64P, C.c_int32, C.c_double, C.c_int, F32P, F32P, I32P, I32P, F64P]
    lib.sqs_solve.restype = None
    lib.sqs_solve.argtypes = [I32P, I64P, C.c_int32, C.c_int, F64P]
    lib.sqs_faces.restype = None
    lib.sqs_faces.argtypes = [I32P, C.c_int32, C.c_int32, I32P, I32P]
    lib.sqs_num_sums.restype = C.c_int
    return lib


def shim_keys(shim, v, cell):
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    k = np.empty(len(v), dtype=np.int64)
    shim.sqs_keys(_p(v, F32P), len(v), cell, _p(k, I64P))
    return k


def shim_sums(shim, v, f, c, cell, cluster, quadrics=True):
    """(count, sums, refused, the largest |d|, contributions) through the header."""
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)
    c = None if c is None else np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3)
    cluster = np.ascontiguousarray(cluster, dtype=np.int32)
    V = len(v)
    count, acc = np.zeros(V, dtype=np.int32), np.zeros((V, SUMS), dtype=np.int64)
    refused, contributions = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    shim.sqs_vertices(_p(v, F32P), _p(c, F32P), V, _p(cluster, I32P), cell, _p(count, I32P), _p(acc, I64P))
    worst = 0.0
    if quadrics:
        worst = shim.sqs_quadrics(_p(v, F32P), V, _p(f, I32P), len(f), _p(cluster, I32P), cell, _p(acc, I64P), _p(refused, I32P),
                                  _p(contributions, I64P))
    return count, acc, int(refused[0]), worst, int(contributions[0])


def shim_place(shim, count, acc, ckeys, cell, placement="quadric", colors=False):
    V = len(count)
    pos, col = np.empty((V, 3), dtype=np.float32), np.empty((V, 3), dtype=np.float32) if colors else None
    rank, fallback, value = np.empty(V, dtype=np.int32), np.empty(V, dtype=np.int32), np.empty(V, dtype=np.float64)
    shim.sqs_place(_p(count, I32P), _p(np.ascontiguousarray(acc), I64P), _p(np.ascontiguousarray(ckeys), I64P), V, cell,
                   int(placement == "quadric"), _p(pos, F32P), _p(col, F32P), _p(rank, I32P), _p(fallback, I32P), _p(value, F64P))
    p = np.empty((V, 3), dtype=np.float64)
    shim.sqs_solve(_p(count, I32P), _p(np.ascontiguousarray(acc), I64P), V, int(placement == "quadric"), _p(p, F64P))
    return dict(positions=pos, colors=col, rank=rank, fallback=fallback, value=value, live=(count > 0) & (ckeys >= 0), p=p)


def shim_triples(shim, f, V, cluster):
    f = np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)
    cluster = np.ascontiguousarray(cluster, dtype=np.int32)
    out = np.empty((len(f), 3), dtype=np.int32)
    shim.sqs_faces(_p(f, I32P), len(f), V, _p(cluster, I32P), _p(out, I32P))
    return out


def simplify(vertices, faces, colors=None, cell=0.1, placement="quadric", dedupe=True, shim=None, details=False):
    """(vertices, faces int32, colors or None, report) of the simplified mesh: the restatement, or with ``shim`` the header itself.
    Raises ValueError as ``simplify_mesh`` does.  ``details=True`` adds a dict of the intermediate arrays."""
    if not (cell > 0 and np.isfinite(cell)):
        raise ValueError("cell must be positive and finite")
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 3)
    V, F = len(v), len(f)
    names = ("vertices", "faces", "vertices_kept", "faces_kept", "cells", "fallbacks", "rank1", "rank2", "rank3", "rms_plane_distance_m")
    if V == 0 or F == 0:
        out = (v[:0], f[:0], None if c is None else c[:0], dict(zip(names, (V, F, 0, 0, 0, 0, 0, 0, 0, 0.0))))
        return out + ({},) if details else out
    quadric = placement == "quadric"
    k = shim_keys(shim, v, cell) if shim else keys(v, cell)
    if (np.isfinite(v).all(axis=1) & (k < 0)).any():
        raise ValueError("a vertex lies beyond 2^20 cells from the origin")
    cluster = cluster_ids(k)
    ckeys = cluster_keys(k, cluster)
    if shim:
        count, acc, refused = shim_sums(shim, v, f, c, cell, cluster, quadric)[:3]
        placed = shim_place(shim, count, acc, ckeys, cell, placement, c is not None)
        tri = shim_triples(shim, f, V, cluster)
    else:
        count, acc, refused = sums(v, f, c, cell, cluster, quadric)[:3]
        placed = place(count, acc, ckeys, cell, placement, c is not None)
        tri = triples(f, V, cluster)
    if refused:
        raise ValueError("a face's area is beyond 2^22 m^2")
    keep = tri[:, 0] >= 0
    if dedupe:
        keep = first_of_each(tri, keep)
    nv, nf, nc = compact(placed["positions"], placed["colors"], tri, keep)
    live, rank = placed["live"], placed["rank"]
    area_q = int((acc[:, 6] + acc[:, 9] + acc[:, 11]).sum())
    value = float(placed["value"].sum())
    rms = cell * np.sqrt(max(value, 0.0) / (area_q * 2.0 ** -40)) if area_q > 0 else 0.0
    report = dict(zip(names, (V, F, len(nv), len(nf), int(live.sum()), int((placed["fallback"] > 0).sum()), int((rank == 1).sum()),
                              int((rank == 2).sum()), int((rank == 3).sum()), float(rms))))
    out = (nv, nf, nc, report)
    return out + (dict(keys=k, cluster=cluster, cell_keys=ckeys, count=count, sums=acc, placed=placed, triples=tri, keep=keep),) if details else out


# ---------------------------------------------------------------------------------------------------------------- meshes
def welded_cube(n=24, lo=(0.0, 0.0, 0.0), size=1.0):
    """A closed cube of n x n quads per side, two triangles each, welded: 6 n^2 + 2 vertices, 12 n^2 faces, outward winding."""
    index, verts, faces = {}, [], []

    def vid(i, j, k):
        if (i, j, k) not in index:
            index[(i, j, k)] = len(verts)
            verts.append((i, j, k))
        return index[(i, j, k)]

    for axis in range(3):
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    def at(u, w):
                        q = [0, 0, 0]
                        q[axis], q[(axis + 1) % 3], q[(axis + 2) % 3] = side, u, w
                        return vid(*q)
                    q00, q10, q11, q01 = at(a, b), at(a + 1, b), at(a + 1, b + 1), at(a, b + 1)
                    if side == n:
                        faces += [(q00, q10, q11), (q00, q11, q01)]
                    else:
                        faces += [(q00, q11, q10), (q00, q01, q11)]
    v = np.asarray(verts, dtype=np.float64) / n * size + np.asarray(lo, dtype=np.float64)
    return v.astype(np.float32), np.asarray(faces, dtype=np.int32)


def uv_sphere(rings=48, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A closed sphere of ``rings`` latitude bands and 2 ``rings`` segments."""
    seg = 2 * rings
    v = [(0.0, 0.0, 1.0)]
    for r in range(1, rings):
        th = np.pi * r / rings
        for s in range(seg):
            ph = 2 * np.pi * s / seg
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda r, s: 1 + (r - 1) * seg + s % seg       # noqa: E731
    f = [(0, ring(1, s), ring(1, s + 1)) for s in range(seg)]
    for r in range(1, rings - 1):
        for s in range(seg):
            f += [(ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)), (ring(r, s), ring(r + 1, s + 1), ring(r, s + 1))]
    last = len(v) - 1
    f += [(last, ring(rings - 1, s + 1), ring(rings - 1, s)) for s in range(seg)]
    return (np.asarray(v) * radius + np.asarray(centre)).astype(np.float32), np.asarray(f, dtype=np.int32)


def torus(nu=40, nv=20, R=0.7, r=0.25):
    u, w = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    v = np.stack(((R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)), axis=-1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + j % nv       # noqa: E731
    f = []
    for i in range(nu):
        for j in range(nv):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v.astype(np.float32), np.asarray(f, dtype=np.int32)


PLANE_NORMAL = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
PLANE_POINT = np.array([0.11, -0.23, 0.37])


def tilted_plane(n=40, spacing=0.021, jitter=0.3, seed=3):
    """An n x n grid with a boundary on a tilted plane, its vertices jittered WITHIN the plane."""
    rng = np.random.default_rng(seed)
    e1 = np.cross(PLANE_NORMAL, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_NORMAL, e1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i + jitter * rng.uniform(-1, 1, i.shape) - n / 2) * spacing
    b = (j + jitter * rng.uniform(-1, 1, j.shape) - n / 2) * spacing
    v = PLANE_POINT + a[..., None] * e1 + b[..., None] * e2
    q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate((np.stack((q, q + n, q + 1), axis=1), np.stack((q + 1, q + n, q + n + 1), axis=1)))
    return v.reshape(-1, 3).astype(np.float32), f.astype(np.int32)


def renumbered(vertices, faces, perm, colors=None):
    """The same mesh with vertex i renamed perm[i]."""
    perm = np.asarray(perm, dtype=np.int64)
    v = np.empty_like(vertices)
    v[perm] = vertices
    f = np.asarray(faces)
    ok = ((f >= 0) & (f < len(perm))).all(axis=1)
    out = f.copy()
    out[ok] = perm[f[ok]]
    if colors is None:
        return v, out.astype(np.int32)
    c = np.empty_like(colors)
    c[perm] = colors
    return v, out.astype(np.int32), c


def directed_edges_balanced(faces):
    """True when every directed edge of ``faces`` occurs as often as its reverse."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    n = int(f.max()) + 1 if len(f) else 1
    fwd, cnt = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    rev, rcnt = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
    return np.array_equal(fwd, rev) and np.array_equal(cnt, rcnt)


def check_invariants(v, f, c, cell, out, dedupe, closed=False, shim=None):
    """CPU item 4 on a result ``out`` = (vertices, faces, colors) of the input (v, f, c)."""
    nv, nf = np.asarray(out[0]), np.asarray(out[1])
    k = keys(v, cell)
    cluster = cluster_ids(k)
    # every output vertex lies within cell / 2 plus one float32 ulp of its cell's centre, in the infinity norm
    ok_key = keys(nv, cell) >= 0
    assert ok_key.all()
    idx = np.floor(nv.astype(np.float64) / cell)
    tri = triples(f, len(v), cluster)
    keep = tri[:, 0] >= 0
    if dedupe:
        keep = first_of_each(tri, keep)
    used = np.zeros(len(v), dtype=bool)
    used[tri[keep].reshape(-1)] = True
    ckeys = cluster_keys(k, cluster)[used]
    assert len(ckeys) == len(nv)
    centre = (np.stack([((ckeys >> (21 * a)) & 0x1fffff) - LIMIT for a in range(3)], axis=1) + 0.5) * cell
    ulp = np.spacing(np.abs(nv).astype(np.float32)).astype(np.float64)
    assert (np.abs(nv.astype(np.float64) - centre) <= cell / 2 + ulp).all()
    del idx
    # every input vertex is within sqrt(3) cell of its cluster's vertex
    renumber = np.cumsum(used) - 1
    has = (cluster >= 0) & used[np.clip(cluster, 0, None)]
    d = np.linalg.norm(v[has].astype(np.float64) - nv[renumber[cluster[has]]].astype(np.float64), axis=1)
    assert (d <= np.sqrt(3) * cell * (1 + 1e-6)).all()
    # no degenerate face, no index out of range
    assert nf.dtype == np.int32 and (len(nf) == 0 or (nf.min() >= 0 and nf.max() < len(nv)))
    assert ((nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 0] != nf[:, 2])).all()
    assert (nf[:, 0] < nf[:, 1]).all() and (nf[:, 0] < nf[:, 2]).all()
    assert len(np.unique(nf.reshape(-1))) == len(nv)                    # (every vertex is named)
    if dedupe:
        assert len(np.unique(nf, axis=0)) == len(nf)
        assert np.array_equal(nf, renumber[tri[keep]].astype(np.int32))  # (the survivor is the one of lowest input index, in input order)
    elif closed:
        assert directed_edges_balanced(nf)
