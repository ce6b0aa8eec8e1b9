"""numpy restatement of the mesh cleaning layer (splatam_amd/csrc/meshclean_math.h, splatam_amd/mesh_clean.py): connected components of a
mesh by vertex INDEX, per-component statistics, the filter and the compaction, plus the meshes the tests use.

LABELS  ``labels``: rounds of the min over each face followed by ``lab = lab[lab]``, until nothing changes -- every vertex ends with the
        smallest vertex index of its component.  A face with an index outside 0..V-1 links nothing.
STATS   by root label: vertices, faces (a face counts for the label of its first vertex), the area as an int64 sum of
        rint(area 2^40) of ``meshscore_ref.areas``' doubles, the box by float32 min / max.
FILTER  ``clean``: a component with a face survives the thresholds; ``keep_largest`` keeps the k survivors with the most faces, ties to
        the lower label; surviving faces keep their order, vertices are renumbered densely in their order, colours travel.
"""
import numpy as np

import meshscore_ref as R

AREA_SCALE = 2.0 ** 40
AREA_BAD = 1 << 62


def valid_faces(V, faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def labels(V, faces):
    """int32 [V]: the smallest vertex index of every vertex's component.  Returns (labels, rounds)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(V, f)]
    lab = np.arange(V, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        new = lab.copy()
        if len(f):
            m = lab[f].min(axis=1)
            for k in range(3):
                np.minimum.at(new, f[:, k], m)                          # the face's vertices ...
                np.minimum.at(new, lab[f[:, k]], m)                     # ... and what they point at
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            return lab.astype(np.int32), rounds
        lab = new


def labels_any(V, faces):
    """The same labels through scipy's connected components where scipy is installed (a million vertices in a second), else ``labels``."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return labels(V, faces)[0]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(V, f)]
    rows, cols = np.concatenate((f[:, 0], f[:, 1])), np.concatenate((f[:, 1], f[:, 2]))
    _, comp = connected_components(coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(V, V)), directed=False)
    smallest = np.full(comp.max() + 1 if V else 0, V, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    return smallest[comp].astype(np.int32)


def area_quanta(vertices, faces):
    """int64 [F]: rint(area 2^40), AREA_BAD for a face whose area is not below 2^22 m^2."""
    a = R.areas(vertices, faces)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(a < 2.0 ** 22, np.rint(np.where(a < 2.0 ** 22, a, 0.0) * AREA_SCALE), float(AREA_BAD)).astype(np.int64)


def stats(vertices, faces, lab=None):
    """dict by root label of arrays of length V: num_vertices, num_faces (int32), area_quanta (int64), area (float64), lo, hi
    (float32 [V, 3]; NaN where the index is no root), is_root."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    if lab is None:
        lab = labels(V, f)[0]
    lab = np.asarray(lab, dtype=np.int64)
    ok = valid_faces(V, f)
    root = lab[f[ok, 0]]
    nv = np.bincount(lab, minlength=V).astype(np.int32)
    nf = np.bincount(root, minlength=V).astype(np.int32)
    q = np.zeros(V, dtype=np.int64)
    np.add.at(q, root, area_quanta(v, f)[ok])
    lo, hi = np.full((V, 3), np.inf, dtype=np.float32), np.full((V, 3), -np.inf, dtype=np.float32)
    np.minimum.at(lo, lab, v)
    np.maximum.at(hi, lab, v)
    is_root = lab == np.arange(V)
    lo[~is_root], hi[~is_root] = np.nan, np.nan
    return {"num_vertices": nv, "num_faces": nf, "area_quanta": q, "area": q.astype(np.float64) * 2.0 ** -40, "lo": lo, "hi": hi, "is_root": is_root}


def survivors(st, min_vertices=200, min_faces=0, min_area=0.0, min_extent=0.0, keep_largest=None):
    with np.errstate(invalid="ignore"):
        d = st["hi"].astype(np.float64) - st["lo"].astype(np.float64)
        extent = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        keep = (st["is_root"] & (st["num_faces"] > 0) & (st["num_vertices"] >= min_vertices) & (st["num_faces"] >= min_faces)
                & (st["area"] >= min_area) & (extent >= min_extent))
    if keep_largest is not None:
        cand = np.flatnonzero(keep)
        order = cand[np.lexsort((cand, -st["num_faces"][cand].astype(np.int64)))][:keep_largest]        # most faces first, then the lower label
        keep = np.zeros_like(keep)
        keep[order] = True
    return keep


def clean(vertices, faces, colors=None, **thresholds):
    """(vertices, faces int32, colors or None, report) of the cleaned mesh."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    if V == 0 or len(f) == 0:
        return v[:0], f[:0].astype(np.int32), None if colors is None else colors[:0], dict(components=0, components_kept=0, faces=len(f),
                                                                                          faces_removed=len(f), area_m2=0.0, area_removed_m2=0.0)
    lab = labels(V, f)[0].astype(np.int64)
    st = stats(v, f, lab)
    keep_c = survivors(st, **thresholds)
    ok = valid_faces(V, f)
    keep_f = ok.copy()
    keep_f[ok] = keep_c[lab[f[ok, 0]]]
    kept = f[keep_f]
    used = np.zeros(V, dtype=bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    total, kept_q = int(st["area_quanta"].sum()), int(st["area_quanta"][keep_c].sum())
    report = dict(components=int((st["is_root"] & (st["num_faces"] > 0)).sum()), components_kept=int(keep_c.sum()), faces=len(f),
                  faces_removed=len(f) - len(kept), area_m2=total * 2.0 ** -40, area_removed_m2=(total - kept_q) * 2.0 ** -40)
    return v[used], renumber[kept].astype(np.int32), None if colors is None else np.asarray(colors)[used], report


# ---------------------------------------------------------------------------------------------------------------- meshes
def strip(n):
    """A strip of ``n`` triangles over n + 2 vertices: triangle i is (i, i + 1, i + 2); vertices on two rows."""
    i = np.arange(n + 2)
    v = np.stack((0.01 * (i // 2), 0.01 * (i % 2), np.zeros(n + 2)), axis=1).astype(np.float32)
    t = np.arange(n)
    return v, np.stack((t, t + 1, t + 2), axis=1).astype(np.int32)


def grid(nx, ny, spacing=0.01, origin=(0.0, 0.0, 0.0)):
    """An nx x ny grid of vertices, two triangles per cell."""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    v = (np.stack((x, y, np.zeros_like(x)), axis=-1).reshape(-1, 3) * spacing + np.asarray(origin)).astype(np.float32)
    a = (x[:-1, :-1] * ny + y[:-1, :-1]).reshape(-1)
    f = np.concatenate((np.stack((a, a + ny, a + 1), axis=1), np.stack((a + 1, a + ny, a + ny + 1), axis=1)))
    return v, f.astype(np.int32)


def cube(lo=(0.0, 0.0, 0.0), size=1.0):
    """8 vertices, 12 triangles."""
    c = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64) * size + np.asarray(lo)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, cc, d in q for t in ((a, b, cc), (a, cc, d))]
    return c.astype(np.float32), np.array(f, dtype=np.int32)


def tetrahedron(at, size=0.02):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64) * size + np.asarray(at)
    return v.astype(np.float32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)


def join(parts):
    """One mesh of several (vertices, faces): indices offset, nothing welded."""
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def renumbered(vertices, faces, perm):
    """The same mesh with vertex i renamed perm[i]."""
    perm = np.asarray(perm, dtype=np.int64)
    v = np.empty_like(vertices)
    v[perm] = vertices
    return v, perm[faces].astype(np.int32)


def mix(seed=5):
    """3 000 loose triangles, 50 tetrahedra and one 40 x 40 grid, vertex ids permuted and faces shuffled: (vertices, faces)."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(3000):
        at = rng.uniform(-2, 2, size=3)
        parts.append(((at + rng.uniform(0.005, 0.03, size=(3, 3))).astype(np.float32), np.array([[0, 1, 2]], dtype=np.int32)))
    parts += [tetrahedron(rng.uniform(-2, 2, size=3)) for _ in range(50)]
    parts.append(grid(40, 40, origin=(-0.2, 0.3, 0.1)))
    v, f = join(parts)
    v, f = renumbered(v, f, rng.permutation(len(v)))
    return v, f[rng.permutation(len(f))]
