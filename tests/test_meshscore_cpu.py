"""The mesh score layer without a GPU: splatam_amd/csrc/meshscore_math.h compiled for the host (tests/meshscore_math_shim.cpp: the loop
bodies of the kernels of csrc/meshscore.hip) against the numpy restatement tests/meshscore_ref.py, and the PLY reader.

1. PLY: binary and ASCII round trips through ``save_mesh_ply`` / ``load_mesh_ply``; a quad file (fan-triangulated), mixed polygons, extra
   vertex properties, a ``uint`` index type with a ``ushort`` count; big-endian files and files without faces refused by name.
2. SAMPLER: Philox4x32-10 against the published known answer for the zero counter and key, and against the restatement; the header's points and faces equal the restatement's bit for
   bit on a 12-triangle box of unequal sides plus one zero-area triangle, n = 60 000, two seeds; every sample within 8 2^-24 x (largest
   coordinate magnitude) of its triangle's plane and of the triangle; each triangle's share within 5 sqrt(n p (1 - p)) of n p; the
   zero-area triangle gets none; sample i does not depend on n.
3. GRID SEARCH: the host loop over the header's functions gives dist2 and index EQUAL to the float32 brute force on every case of
   ``meshscore_ref.nn_cases`` (the list of tests/test_gpu_meshscore.py), and |d32 - d64| <= 4 2^-24 d64 against the float64 brute force
   (one rounding per difference, per square and per add, halved by the root).  The ring bound never exceeds the float32 d2 of an
   unsearched target, on the lattice cases and on the first.
4. PLUMBING: ``plan_grid`` (the cell from the box's area, the 2^21 cap, degenerate boxes, refusals) and ``load_transform``."""
import ctypes as C

import numpy as np
import pytest

import meshscore_ref as R
from tests.util import host_shim

F32P, F64P, I32P, U32P = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def load_shim():
    lib = host_shim("meshscore_math_shim", "meshscore_math.h")
    lib.mm_uniform3.restype = None
    lib.mm_uniform3.argtypes = [C.c_uint64, C.c_uint64, C.c_longlong, F32P]
    lib.mm_philox.restype = None
    lib.mm_philox.argtypes = [C.c_uint64, C.c_uint64, U32P]
    lib.mm_areas.restype = None
    lib.mm_areas.argtypes = [F32P, C.c_int32, I32P, C.c_int32, F64P]
    lib.mm_sample.restype = None
    lib.mm_sample.argtypes = [F32P, C.c_int32, I32P, C.c_int32, F64P, C.c_uint64, C.c_longlong, F32P, I32P]
    lib.mm_cell_keys.restype = C.c_int
    lib.mm_cell_keys.argtypes = [F32P, C.c_float, I32P, F32P, C.c_longlong, I32P]
    lib.mm_nearest.restype = C.c_int
    lib.mm_nearest.argtypes = [F32P, C.c_float, I32P, F32P, C.c_int32, F32P, C.c_longlong, F32P, I32P, I32P]
    lib.mm_ring_bound2.restype = C.c_double
    lib.mm_ring_bound2.argtypes = [F32P, C.c_float, I32P, F32P, C.c_int]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def shim_areas(shim, vertices, faces):
    v, f = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(faces, np.int32)
    area = np.empty(len(f), dtype=np.float64)
    shim.mm_areas(_p(v, F32P), len(v), _p(f, I32P), len(f), _p(area, F64P))
    return area


def shim_sample(shim, vertices, faces, prefix, seed, n):
    v, f, pre = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(faces, np.int32), np.ascontiguousarray(prefix, np.float64)
    points, face = np.empty((n, 3), dtype=np.float32), np.empty(n, dtype=np.int32)
    shim.mm_sample(_p(v, F32P), len(v), _p(f, I32P), len(f), _p(pre, F64P), seed, n, _p(points, F32P), _p(face, I32P))
    return points, face


def shim_nearest(shim, targets, queries, cell, account=False):
    """The header's search on the grid ``plan_grid`` gives for the targets' box: (dist2, index[, account]) and the grid."""
    from splatam_amd.mesh_score import plan_grid
    t, q = np.ascontiguousarray(targets, np.float32), np.ascontiguousarray(queries, np.float32)
    lo, cell, dims = plan_grid(t.min(axis=0), t.max(axis=0), len(t), cell)
    lo32, dims32 = np.array(lo, dtype=np.float32), np.array(dims, dtype=np.int32)
    d2, idx, acc = np.empty(len(q), dtype=np.float32), np.empty(len(q), dtype=np.int32), np.zeros((len(q), 2), dtype=np.int32)
    assert shim.mm_nearest(_p(lo32, F32P), cell, _p(dims32, I32P), _p(t, F32P), len(t), _p(q, F32P), len(q), _p(d2, F32P), _p(idx, I32P),
                           _p(acc, I32P)) == 0
    return (d2, idx, acc, (lo, cell, dims)) if account else (d2, idx)


# ---------------------------------------------------------------------------------------------------------------- 1. PLY
def _write(path, header, body):
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(body)


def test_ply_round_trips_binary_and_ascii(tmp_path):
    from splatam_amd.export import load_mesh_ply, save_mesh_ply
    v, f = R.sphere_mesh(2, 0.45, (0.1, -0.2, 0.3))
    col = np.random.default_rng(0).integers(0, 256, (len(v), 3)).astype(np.float32) / np.float32(255.0)
    path = str(tmp_path / "binary.ply")
    save_mesh_ply(path, v, f, col)
    v2, f2, c2 = load_mesh_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32 and c2.dtype == np.float32
    assert v2.tobytes() == v.tobytes() and np.array_equal(f2, f) and np.array_equal(np.rint(c2 * 255), np.rint(col * 255))
    save_mesh_ply(path, v, f)
    v3, f3, c3 = load_mesh_ply(path)
    assert v3.tobytes() == v.tobytes() and np.array_equal(f3, f) and c3 is None
    save_mesh_ply(str(tmp_path / "again.ply"), v2, f2, c2)                # what was read writes the same bytes
    save_mesh_ply(path, v, f, col)
    assert open(path, "rb").read() == open(tmp_path / "again.ply", "rb").read()
    # ASCII: %.9g reads back to the same float32
    header = f"ply\nformat ascii 1.0\ncomment made by a test\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
    header += f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n"
    rows = "".join("%.9g %.9g %.9g %d %d %d\n" % (*p, *np.rint(c * 255)) for p, c in zip(v, col))
    rows += "".join("3 %d %d %d\n" % tuple(t) for t in f)
    _write(tmp_path / "ascii.ply", header, rows.encode("ascii"))
    v4, f4, c4 = load_mesh_ply(str(tmp_path / "ascii.ply"))
    assert v4.tobytes() == v.tobytes() and np.array_equal(f4, f) and np.array_equal(np.rint(c4 * 255), np.rint(col * 255))


def test_ply_quads_polygons_extra_properties_and_uint_indices(tmp_path):
    from splatam_amd.export import load_mesh_ply
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [2, 1, 0], [3, 0.5, 0]], dtype=np.float32)
    # quads, binary, with normals and a double "quality" among the vertex properties, uint indices under a ushort count
    vt = np.zeros(len(v), dtype=[('nx', '<f4'), ('x', '<f4'), ('quality', '<f8'), ('y', '<f4'), ('z', '<f4'), ('ny', '<f4'), ('nz', '<f4')])
    vt['x'], vt['y'], vt['z'], vt['quality'], vt['nx'] = v[:, 0], v[:, 1], v[:, 2], 7.5, 1.0
    quads = np.array([[0, 1, 2, 3], [1, 4, 5, 2]])
    ft = np.zeros(2, dtype=[('n', '<u2'), ('v', '<u4', (4,))])
    ft['n'], ft['v'] = 4, quads
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float nx\nproperty float x\nproperty double quality\n"
              "property float y\nproperty float z\nproperty float ny\nproperty float nz\nelement face 2\n"
              "property list ushort uint vertex_index\nend_header\n")
    _write(tmp_path / "quads.ply", header, vt.tobytes() + ft.tobytes())
    v2, f2, c2 = load_mesh_ply(str(tmp_path / "quads.ply"))
    assert v2.tobytes() == v.tobytes() and c2 is None
    assert f2.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 5], [1, 5, 2]]
    # a triangle, a quad and a pentagon in one binary file, and the same in ASCII
    polys = [[0, 1, 2], [1, 4, 5, 2], [0, 1, 4, 6, 5]]
    body = b"".join(np.array([len(p)], '<u1').tobytes() + np.array(p, '<i4').tobytes() for p in polys)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\nelement face 3\n"
    header += "property list uchar int vertex_indices\nend_header\n"
    _write(tmp_path / "mixed.ply", header, v.astype('<f4').tobytes() + body)
    want = [[0, 1, 2], [1, 4, 5], [1, 5, 2], [0, 1, 4], [0, 4, 6], [0, 6, 5]]
    assert load_mesh_ply(str(tmp_path / "mixed.ply"))[1].tolist() == want
    text = "".join("%g %g %g\n" % tuple(p) for p in v) + "".join("%d %s\n" % (len(p), " ".join(map(str, p))) for p in polys)
    _write(tmp_path / "mixed_ascii.ply", header.replace("binary_little_endian", "ascii"), text.encode("ascii"))
    v3, f3, _ = load_mesh_ply(str(tmp_path / "mixed_ascii.ply"))
    assert f3.tolist() == want and v3.tobytes() == v.tobytes()


def test_ply_refusals_name_the_file(tmp_path):
    from splatam_amd.export import load_mesh_ply, save_ply
    big = tmp_path / "big_endian.ply"
    _write(big, "ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nelement face 0\n"
                "property list uchar int vertex_indices\nend_header\n", b"")
    with pytest.raises(ValueError, match="big_endian.ply.*big-endian"):
        load_mesh_ply(str(big))
    cloud = tmp_path / "cloud.ply"
    _write(cloud, "ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
           np.zeros(6, '<f4').tobytes())
    with pytest.raises(ValueError, match="cloud.ply.*no faces"):
        load_mesh_ply(str(cloud))
    empty = tmp_path / "no_faces.ply"
    _write(empty, "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nelement face 0\n"
                  "property list uchar int vertex_indices\nend_header\n", b"0 0 0\n")
    with pytest.raises(ValueError, match="no_faces.ply.*no faces"):
        load_mesh_ply(str(empty))
    splat = str(tmp_path / "splat.ply")                                   # the Gaussian export is a point cloud too
    save_ply(splat, np.zeros((3, 3)), np.zeros((3, 1)), np.zeros((3, 4)), np.zeros((3, 3)), np.zeros((3, 1)))
    with pytest.raises(ValueError, match="splat.ply.*no faces"):
        load_mesh_ply(splat)
    bad = tmp_path / "bad_index.ply"
    _write(bad, "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                "property list uchar int vertex_indices\nend_header\n", b"0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n")
    with pytest.raises(ValueError, match="bad_index.ply.*do not exist"):
        load_mesh_ply(str(bad))


# ---------------------------------------------------------------------------------------------------------------- 2. sampler
def test_philox_known_answers(shim):
    """The known answer of the Random123 distribution (kat_vectors, philox4x32 with 10 rounds) for the all-zero counter and key: the
    header and the restatement both give it.  (The header's counter is (i low, i high, 0, 0), so the all-ones vector cannot be asked.)"""
    out = (C.c_uint32 * 4)()
    shim.mm_philox(0, 0, out)
    assert [hex(v) for v in out] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    assert [hex(v) for v in R.philox4x32_10(0, [0])[0]] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    # counter (ff.., ff.., 0, 0) is not a published vector: the two implementations against each other on large counters and keys
    seed, i = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF
    shim.mm_philox(seed, i, out)
    assert list(out) == R.philox4x32_10(seed, np.array([i], dtype=np.uint64))[0].tolist()
    u = np.empty((1000, 3), dtype=np.float32)
    shim.mm_uniform3(12345678901234567, 2 ** 40, 1000, _p(u, F32P))
    ref = R.uniform3(12345678901234567, np.arange(2 ** 40, 2 ** 40 + 1000, dtype=np.uint64))
    assert u.tobytes() == ref.tobytes() and u.min() >= 0 and u.max() < 1


@pytest.mark.parametrize("seed", (0, 0x123456789ABCDEF))
def test_sampler_equals_the_restatement_and_lies_on_the_surface(shim, seed):
    n = 60_000
    v, f = R.box_mesh()
    area = shim_areas(shim, v, f)
    assert area.tobytes() == R.areas(v, f).tobytes() and area[12] == 0 and (area[:12] > 0).all()
    assert np.allclose(area[:12].sum(), 2 * (1.0 * 0.7 + 0.7 * 0.4 + 0.4 * 1.0), rtol=1e-6)
    prefix = np.cumsum(area)
    pts, face = shim_sample(shim, v, f, prefix, seed, n)
    ref_pts, ref_face, (u1, u2) = R.sample(v, f, n, seed, prefix)
    assert face.tobytes() == ref_face.tobytes() and pts.tobytes() == ref_pts.tobytes()
    # on the surface: the float64 point of the same (u1, u2) is a convex combination of the triangle's corners up to the fold's own
    # rounding (u1 + u2 <= 1 + 2^-24), and the float32 point is within the bound of it and of the triangle's plane
    bound = 8 * EPS * float(np.abs(v).max())
    p64 = R.sample(v, f, n, seed, prefix, dtype=np.float64)[0]
    assert (u1 >= 0).all() and (u2 >= 0).all() and (u1.astype(np.float64) + u2.astype(np.float64) <= 1 + EPS).all()
    err = np.linalg.norm(pts.astype(np.float64) - p64, axis=1)
    v64, f64 = v.astype(np.float64), f.astype(np.int64)
    a, b, c = (v64[f64[face, k]] for k in range(3))
    normal = np.cross(b - a, c - a)
    plane = np.abs(((pts.astype(np.float64) - a) * normal).sum(axis=1)) / np.linalg.norm(normal, axis=1)
    print(f"seed {seed:#x}: largest distance to the float64 point {err.max():.3e}, to the plane {plane.max():.3e}, bound {bound:.3e}")
    assert err.max() <= bound and plane.max() <= bound
    # shares
    counts = np.bincount(face, minlength=13)
    p = area / area.sum()
    dev = np.abs(counts - n * p) / np.maximum(np.sqrt(n * p * (1 - p)), 1e-30)
    print(f"seed {seed:#x}: counts {counts.tolist()}, largest deviation {dev[:12].max():.2f} sigma")
    assert counts[12] == 0 and (dev[:12] <= 5).all()
    # sample i does not depend on n
    few_pts, few_face = shim_sample(shim, v, f, prefix, seed, 1000)
    assert few_pts.tobytes() == pts[:1000].tobytes() and few_face.tobytes() == face[:1000].tobytes()
    one_pts, _ = shim_sample(shim, v, f, prefix, seed, 1)
    assert one_pts.tobytes() == pts[:1].tobytes()
    assert R.sample(v, f, 10, seed, prefix, first=500)[0].tobytes() == pts[500:510].tobytes()


def test_a_face_that_names_no_vertex_has_no_area_and_no_sample(shim):
    v, f = R.box_mesh(zero_area=False)
    f = np.concatenate((f, np.array([[0, 1, 8], [-1, 2, 3]], dtype=np.int32)))
    area = shim_areas(shim, v, f)
    assert area[12] == 0 and area[13] == 0 and area.tobytes() == R.areas(v, f).tobytes()
    _, face = shim_sample(shim, v, f, np.cumsum(area), 3, 5000)
    assert face.min() >= 0 and face.max() < 12
    pts, face = shim_sample(shim, v, f, np.zeros(len(f)), 3, 10)            # a mesh without area
    assert (face == -1).all() and not pts.any()


# ---------------------------------------------------------------------------------------------------------------- 3. grid search
CASES = R.nn_cases()


@pytest.fixture(scope="module")
def brute():
    """The float32 and float64 brute force of every case, computed once."""
    return {name: (R.brute32(q, t), R.brute64(q, t)) for name, (t, q, _) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_grid_search_equals_the_float32_brute_force(shim, brute, name):
    targets, queries, cell = CASES[name]
    d2, idx, acc, (lo, c, dims) = shim_nearest(shim, targets, queries, cell, account=True)
    (ref_d2, ref_idx), d64 = brute[name]
    cells = dims[0] * dims[1] * dims[2]
    print(f"{name}: grid {dims} of cell {c:.6g} ({cells} cells), {len(targets)} targets, {len(queries)} queries; candidates per query "
          f"mean {acc[:, 0].mean():.1f} max {acc[:, 0].max()}, shells mean {acc[:, 1].mean():.2f} max {acc[:, 1].max()}")
    assert cells <= 2 ** 21
    assert d2.tobytes() == ref_d2.tobytes() and idx.tobytes() == ref_idx.tobytes()
    d32 = np.sqrt(d2.astype(np.float64))
    print(f"{name}: largest |d32 - d64| / (2^-24 d64) = {(np.abs(d32 - d64) / np.maximum(EPS * d64, 1e-300)).max():.3f} (bound 4)")
    assert (np.abs(d32 - d64) <= 4 * EPS * d64).all()
    if name == "cell-cap":
        assert cells > 2 ** 20 and c > 1e-3                              # the cell grew until the grid fitted
    if name == "one-cell":
        assert dims == (1, 1, 1) and (acc[:, 0] == len(targets)).all()
    if name == "coplanar":
        assert dims[2] == 1
    if name == "coincident":
        assert (d2[:600] == 0).all()
    if name == "duplicates":
        assert (d2[:150] == 0).all() and (idx[:150] == ref_idx[:150]).all()
    if name == "uniform-box":
        assert acc[:, 0].mean() < 0.1 * len(targets)                     # (the grid does prune)
    if name == "cluster-and-stray":
        assert (idx == 2000).any() and (idx != 2000).any()


def test_the_ring_bound_is_conservative(shim):
    """For the lattice cases -- targets exactly on cell faces -- and every shell count r: no target outside the searched box has a
    float32 d2 below the bound; a query outside the grid's box on an axis has the grid's open side there, never a negative distance."""
    from splatam_amd.mesh_score import plan_grid
    for name in ("cell-faces-0.1", "cell-faces-0.125", "uniform-box"):
        targets, queries, cell = CASES[name]
        lo, c, dims = plan_grid(targets.min(axis=0), targets.max(axis=0), len(targets), cell)
        lo32, dims32 = np.array(lo, dtype=np.float32), np.array(dims, dtype=np.int32)
        keys_t, keys_q = np.empty(len(targets), dtype=np.int32), np.empty(len(queries), dtype=np.int32)
        assert shim.mm_cell_keys(_p(lo32, F32P), c, _p(dims32, I32P), _p(targets, F32P), len(targets), _p(keys_t, I32P)) == 0
        assert shim.mm_cell_keys(_p(lo32, F32P), c, _p(dims32, I32P), _p(queries, F32P), len(queries), _p(keys_q, I32P)) == 0
        cell_of = lambda k: np.stack((k % dims[0], (k // dims[0]) % dims[1], k // (dims[0] * dims[1])), axis=1)      # noqa: E731
        ct, cq = cell_of(keys_t), cell_of(keys_q)
        checked = 0
        for n in range(0, len(queries), 7):
            q = np.ascontiguousarray(queries[n])
            d = q[None, :] - targets
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            ring = np.abs(ct - cq[n]).max(axis=1)
            for r in range(0, int(ring.max())):
                b2 = shim.mm_ring_bound2(_p(lo32, F32P), c, _p(dims32, I32P), _p(q, F32P), r)
                outside = ring > r
                assert outside.any() and b2 >= 0 and float(d2[outside].min()) >= b2, (name, n, r)
                checked += 1
        assert checked > 100


# ---------------------------------------------------------------------------------------------------------------- 4. plumbing
def test_plan_grid_caps_the_cells_and_takes_degenerate_boxes():
    from splatam_amd.mesh_score import MAX_CELLS, plan_grid
    lo, cell, dims = plan_grid((0, 0, 0), (8.0, 6.0, 3.0), 200_000)
    assert dims == tuple(int(np.floor(e / cell)) + 1 for e in (8.0, 6.0, 3.0)) and dims[0] * dims[1] * dims[2] <= MAX_CELLS
    assert cell == float(np.float32(cell)) and lo == (0.0, 0.0, 0.0)
    assert abs(cell - np.sqrt(2.0 * 2 * (48 + 18 + 24) / 200_000)) < 1e-6          # 2 targets per cell of the box's own area: no cap here
    _, capped, dims = plan_grid((0, 0, 0), (8.0, 6.0, 3.0), 200_000, cell=1e-3)
    assert capped > 1e-3 and MAX_CELLS / 2 < dims[0] * dims[1] * dims[2] <= MAX_CELLS
    assert plan_grid((1, 2, 3), (1, 2, 3), 1)[1:] == (1.0, (1, 1, 1))               # one point
    _, cell, dims = plan_grid((0, 0, 0), (2.0, 0, 0), 10)                            # a line: extent / count as float32, 0.2 rounded up
    assert cell == float(np.float32(0.2)) and dims == (int(np.floor(2.0 / cell)) + 1, 1, 1) and dims[0] == 10
    assert plan_grid((0, 0, 0), (1.0, 1.0, 0), 100)[2][2] == 1                       # a plane
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf"))):
        with pytest.raises(ValueError):
            plan_grid((0, 0, 0), (1, 1, 1), 10, **bad)
    with pytest.raises(ValueError):
        plan_grid((0, 0, 0), (float("inf"), 1, 1), 10)
    with pytest.raises(ValueError):
        plan_grid((0, 0, 0), (-1, 1, 1), 10)


def test_load_transform_reads_the_first_sixteen_numbers(tmp_path):
    from splatam_amd.mesh_score import load_transform
    M = np.arange(16, dtype=np.float64).reshape(4, 4) / 7
    traj = tmp_path / "traj.txt"                                         # Replica's layout: one row-major pose per line
    traj.write_text("\n".join(" ".join(repr(float(v)) for v in (M + k).reshape(-1)) for k in range(3)) + "\n")
    assert np.array_equal(load_transform(str(traj)), M)
    square = tmp_path / "pose.txt"
    np.savetxt(str(square), M)
    assert np.allclose(load_transform(str(square)), M, rtol=0, atol=1e-15)
    short = tmp_path / "short.txt"
    short.write_text("1 0 0\n0 1 0\n")
    with pytest.raises(ValueError, match="short.txt.*16"):
        load_transform(str(short))
    words = tmp_path / "words.txt"
    words.write_text("a b c d " * 4)
    with pytest.raises(ValueError, match="words.txt"):
        load_transform(str(words))
