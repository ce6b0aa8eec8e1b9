"""Python restatement of the marching-cubes rule of splatam_amd/csrc/tsdf_math.h ("SURFACE, cubes"), written from the rule and not from
the header's table, so that the 256-row literal has something independent to agree with.

    CORNERS   dx + 2 dy + 4 dz; inside when bit c of the mask is set (tsdf < 0).
    EDGES     e = 0..11: the axis edges (c, c | 1 << a), axis-major (a = 0, 1, 2), c ascending within an axis.
    FACES     the four corners of each cube face counter-clockwise seen from outside the cube.  Walking that cycle, every maximal run of
              inside corners gives one directed SEGMENT from the crossing where the walk enters the run to the crossing where it leaves:
              two diagonal inside corners are cut off one by one (the outside connects through the face).
    LOOPS     every crossed edge has one outgoing and one incoming segment; the loops they chain into start at their lowest edge, are
              visited by ascending start and fan-triangulated from it: (l0, li, li+1).
"""
import numpy as np

import tsdf_ref as R

EDGES = [(c, c | (1 << a)) for a in range(3) for c in range(8) if not c & (1 << a)]
EDGE_OF = {e: n for n, e in enumerate(EDGES)}


def face_cycles():
    """[(axis, side, (c0, c1, c2, c3))]: each face's corners counter-clockwise seen from outside.  With (a, b, c) a cyclic permutation of
    the axes e_b x e_c = e_a, so base -> +b -> +b+c -> +c turns about +e_a: the outside view of the face on the +a side; the -a side
    is walked the other way round."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            base = side << a
            cyc = (base, base | (1 << b), base | (1 << b) | (1 << c), base | (1 << c))
            out.append((a, side, cyc if side else (cyc[0], cyc[3], cyc[2], cyc[1])))
    return out


FACES = face_cycles()


def crossing(ca, cb):
    return EDGE_OF[(min(ca, cb), max(ca, cb))]


def cycle_segments(inside4, cyc):
    """Directed segments (edge from, edge to) of one face: ``inside4`` the four booleans along ``cyc``."""
    segs = []
    if all(inside4) or not any(inside4):
        return segs
    for n in range(4):
        if inside4[n] and not inside4[n - 1]:                # the walk enters a run at corner n
            m = n
            while inside4[(m + 1) % 4]:
                m += 1
            segs.append((crossing(cyc[n - 1], cyc[n]), crossing(cyc[m % 4], cyc[(m + 1) % 4])))
    return segs


def face_segments(mask, face):
    cyc = FACES[face][2]
    return cycle_segments([bool((mask >> c) & 1) for c in cyc], cyc)


def segments(mask):
    return [s for f in range(6) for s in face_segments(mask, f)]


def loops(mask):
    nxt = {}
    for a, b in segments(mask):
        assert a not in nxt
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    out, done = [], set()
    for start in sorted(nxt):
        if start in done:
            continue
        loop, e = [], start
        while e not in done:
            done.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        out.append(loop)
    return out


def cell_triangles(mask):
    """[(e0, e1, e2)] of a mask, in table order."""
    return [(l[0], l[n], l[n + 1]) for l in loops(mask) for n in range(1, len(l) - 1)]


def table():
    """[256, 16] int8: the count, then three edge numbers per triangle, zeros behind."""
    t = np.zeros((256, 16), dtype=np.int8)
    for mask in range(256):
        tris = cell_triangles(mask)
        assert len(tris) <= 5
        t[mask, 0] = len(tris)
        t[mask, 1:1 + 3 * len(tris)] = np.array(tris, dtype=np.int8).reshape(-1)
    return t


_TABLE = None


def triangles(tsdf, weight, min_weight=1.0):
    """[F, 3] int64 keys of the volume's cubes surface (arrays [nz, ny, nx]), in cell order: ``tsdf_ref.triangles`` with this rule."""
    global _TABLE
    if _TABLE is None:
        _TABLE = [cell_triangles(m) for m in range(256)]
    nz, ny, nx = tsdf.shape
    dims = (nx, ny, nz)
    inside, seen = tsdf < 0, weight >= min_weight
    mask = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int64)
    ok = np.ones(mask.shape, dtype=bool)
    for c in range(8):
        dx, dy, dz = R.corner_offset(c)
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        mask |= inside[sl].astype(np.int64) << c
        ok &= seen[sl]
    mask[~ok] = 0
    out = []
    for k, j, i in zip(*np.nonzero((mask != 0) & (mask != 255))):
        for tri in _TABLE[int(mask[k, j, i])]:
            out.append([R.edge_key(dims, (i, j, k), *EDGES[e]) for e in tri])
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def directed_edges(faces):
    """{(a, b): count} over the triangles' directed edges."""
    d = {}
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for e in ((a, b), (b, c), (c, a)):
            d[e] = d.get(e, 0) + 1
    return d


def balanced(faces):
    """Every directed edge occurs as often as its reverse (a closed oriented cycle); also the number of directed edges used more than once."""
    d = directed_edges(faces)
    return all(d.get((b, a), 0) == n for (a, b), n in d.items()), sum(1 for n in d.values() if n > 1)


def noise_volume(dims=(14, 13, 12), seed=0):
    """Gaussian noise with an outside shell: a float32 volume dict, weight 1."""
    nx, ny, nz = dims
    f = np.random.default_rng(seed).standard_normal((nz, ny, nx))
    f[0] = f[-1] = f[:, 0] = f[:, -1] = 1.0
    f[:, :, 0] = f[:, :, -1] = 1.0
    return R.field_volume(f)
