"""numpy restatement of the mesh score layer (splatam_amd/csrc/meshscore_math.h), the yardstick of tests/test_meshscore_cpu.py and
tests/test_gpu_meshscore.py:

  * Philox4x32-10 and the surface sampler, BIT FOR BIT in float32 (numpy rounds every float32 operation on its own, as the header's
    one-operation steps do) and the same sampler in float64;
  * the float32 brute-force nearest neighbour with the header's expression order, (dx dx + dy dy) + dz dz, and the lowest index among
    equal distances; the float64 brute force;
  * an octahedron subdivided k times and pushed onto a sphere, with its longest edge;
  * the nearest-neighbour cases both test files run."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(seed, i):
    """[n, 4] uint32: ten rounds over the counters (i low, i high, 0, 0) under the key (seed low, seed high)."""
    i = np.asarray(i, dtype=np.uint64).reshape(-1)
    seed = int(seed) & (2 ** 64 - 1)
    c = [i & MASK, i >> np.uint64(32), np.zeros_like(i), np.zeros_like(i)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]             # (32 x 32 bits: no overflow of uint64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def uniform3(seed, i):
    """[n, 3] float32 in [0, 1): words 0..2 as (word >> 8) 2^-24 (exact)."""
    w = philox4x32_10(seed, i)[:, :3]
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def areas(vertices, faces):
    """float64 areas from the float32 vertices in the header's order; 0 for a face out of range or without area."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    g = np.where(ok[:, None], f, 0)
    e1, e2 = v[g[:, 1]] - v[g[:, 0]], v[g[:, 2]] - v[g[:, 0]]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    a = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    return np.where(ok & (a > 0), a, 0.0)


def sample(vertices, faces, n, seed, prefix=None, dtype=np.float32, first=0):
    """(points [n, 3] of ``dtype``, face [n] int32, (u1, u2) after the fold as float32): samples first .. first + n - 1.  float32: the
    header's result bit for bit.  float64: the same triangle and the same folded (u1, u2), the point formed in float64."""
    v32 = np.asarray(vertices, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64)
    if prefix is None:
        prefix = np.cumsum(areas(v32, f))
    u = uniform3(seed, np.arange(first, first + n, dtype=np.uint64))
    t = u[:, 0].astype(np.float64) * prefix[-1]
    face = np.searchsorted(prefix, t, side="right")                      # the first prefix that EXCEEDS t
    assert (face < len(f)).all()
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    fold = (u1 + u2) > np.float32(1.0)                                   # (a float32 sum, as in the header)
    u1[fold], u2[fold] = np.float32(1.0) - u1[fold], np.float32(1.0) - u2[fold]
    v = v32.astype(dtype)
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    w1, w2 = u1.astype(dtype)[:, None], u2.astype(dtype)[:, None]
    p = (a + w1 * (b - a)) + w2 * (c - a)
    assert p.dtype == dtype
    return p, face.astype(np.int32), (u1, u2)


def brute32(queries, targets, chunk=512):
    """(dist2 float32 [n], index int32 [n]): every target compared in float32, (dx dx + dy dy) + dz dz; np.argmin returns the FIRST
    minimum, i.e. the lowest index among equals."""
    q, t = np.asarray(queries, dtype=np.float32), np.asarray(targets, dtype=np.float32)
    d2, idx = np.empty(len(q), dtype=np.float32), np.empty(len(q), dtype=np.int32)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - t[None, :, :]
        m = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert m.dtype == np.float32
        k = np.argmin(m, axis=1)
        idx[s:s + chunk], d2[s:s + chunk] = k, m[np.arange(len(k)), k]
    return d2, idx


def brute64(queries, targets, chunk=512):
    """float64 distance [n] of every query to its nearest target."""
    q, t = np.asarray(queries, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    out = np.empty(len(q))
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - t[None, :, :]
        out[s:s + chunk] = np.sqrt((d * d).sum(axis=2).min(axis=1))
    return out


# ---------------------------------------------------------------------------------------------------------------- closed-form geometry
def sphere_mesh(k, r, centre=(0.0, 0.0, 0.0)):
    """(vertices float32 [V, 3], faces int32 [F, 3]): an octahedron subdivided ``k`` times (every triangle into four, midpoints shared),
    every vertex pushed onto the sphere of radius ``r`` (in float64, rounded once); outward winding."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)
    for _ in range(k):
        e = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        n, F = len(v), len(f)
        m01, m12, m20 = n + inv[:F], n + inv[F:2 * F], n + inv[2 * F:]
        v = np.concatenate((v, mid))
        f = np.concatenate((np.stack((f[:, 0], m01, m20), 1), np.stack((m01, f[:, 1], m12), 1), np.stack((m20, m12, f[:, 2]), 1),
                            np.stack((m01, m12, m20), 1)))
    return (v * r + np.asarray(centre, dtype=np.float64)).astype(np.float32), f.astype(np.int32)


def longest_edge(vertices, faces):
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    return float(max(np.linalg.norm(v[f[:, a]] - v[f[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0))))


def box_mesh(sides=(1.0, 0.7, 0.4), origin=(-0.3, 0.2, 0.1), zero_area=True):
    """The 12 triangles of a box of unequal sides, and (``zero_area``) a 13th triangle of no area (two corners the same)."""
    s, o = np.asarray(sides), np.asarray(origin)
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], dtype=np.float64) * s + o
    f = [[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]]
    if zero_area:
        f.append([0, 7, 7])
    return v.astype(np.float32), np.array(f, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- the cases
BOX = (1.0, 0.7, 0.4)


def _uniform(rng, n, lo=(0.0, 0.0, 0.0), size=BOX):
    return (np.asarray(lo) + rng.random((n, 3)) * np.asarray(size)).astype(np.float32)


def nn_cases():
    """name -> (targets float32 [M, 3], queries float32 [n, 3], cell or None): the cases both test files run the grid search on."""
    rng = np.random.default_rng(20)
    cases = {}
    t, q = _uniform(rng, 2500, (-0.2, 0.1, 0.3)), _uniform(rng, 3001, (-0.25, 0.05, 0.25), (1.1, 0.8, 0.5))
    cases["uniform-box"] = (t, q, None)
    cases["cell-cap"] = (t, q, 1e-4)                                     # 10 000 x 7 000 x 4 000 cells asked for: the 2^21 cap applies
    cases["one-cell"] = (t, q, 10.0)
    cluster = _uniform(rng, 2000, (0.0, 0.0, 0.0), (0.04, 0.04, 0.04))
    far = np.array([[2.0, 2.0, 1.0]], dtype=np.float32)                  # 3 m from the cluster
    inside = _uniform(rng, 200, (0.0, 0.0, 0.0), (0.04, 0.04, 0.04))
    between = _uniform(rng, 200, (0.0, 0.0, 0.0), (2.0, 2.0, 1.0))
    outside = np.concatenate((_uniform(rng, 50, (7.0, 0.0, 0.0), (0.5, 2.0, 1.0)), _uniform(rng, 50, (-3.0, -5.0, -4.0), (1.0, 1.0, 1.0))))
    cases["cluster-and-stray"] = (np.concatenate((cluster, far)), np.concatenate((inside, between, outside)), 0.05)
    cases["one-target"] = (np.array([[0.3, -0.2, 0.7]], dtype=np.float32), _uniform(rng, 130, (-1.0, -1.0, -1.0), (2.0, 2.0, 2.0)), None)
    plane = _uniform(rng, 1500)
    plane[:, 2] = np.float32(0.3)
    cases["coplanar"] = (plane, _uniform(rng, 700, (0.0, 0.0, 0.0), (1.0, 0.7, 0.6)), None)
    cases["coincident"] = (t, np.concatenate((t[rng.permutation(2500)[:600]], q[:101])), None)
    for name, cell in (("cell-faces-0.1", 0.1), ("cell-faces-0.125", 0.125)):
        lo, c = np.array([0.3, -0.2, 0.1], dtype=np.float32), np.float32(cell)
        k = np.stack(np.meshgrid(np.arange(9), np.arange(8), np.arange(7), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
        lattice = lo + k * c                                             # lo + k cell in float32
        assert lattice.dtype == np.float32
        pick = rng.permutation(len(lattice))
        cases[name] = (lattice[pick[:300]].copy(), np.concatenate((lattice, lattice[pick[:40]] + np.float32(0.05) * c)), float(c))
        cases[name][0][0] = lattice[0]                                   # (the grid's lo is the lattice's origin)
    d = _uniform(rng, 300)
    both = np.concatenate((d, d))[rng.permutation(600)]
    cases["duplicates"] = (both, np.concatenate((d[:150], _uniform(rng, 250))), None)
    cases["64-queries"] = (t, q[:64], None)
    cases["65-queries"] = (t, q[:65], None)
    return cases
