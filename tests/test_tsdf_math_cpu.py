"""The mesh layer without a GPU: splatam_amd/csrc/tsdf_math.h compiled for the host (tests/tsdf_math_shim.cpp: the loop bodies of the
kernels of csrc/tsdf.hip over every grid point, cell and vertex) against the float64 numpy restatement tests/tsdf_ref.py.

1. UPDATE RULE on a 37 x 21 x 13 volume (voxel 0.05, an origin off the grid's own lattice, trunc 0.2) under 72 x 40 planes of a tilted
   plane with a band below the silhouette threshold, a zero-depth hole and a NaN pixel, from four poses, once and three views into one
   volume: the same decisions as float64 on every grid point that is not within rounding of a threshold (at most 2 % are), values
   within 4 x the float32 numpy form's own largest error (``tsdf_ref.check_update``).
2. TABLE: all 256 corner sign patterns of one cell give the restatement's triangles, as sets of oriented key triples up to rotation.
3. TOPOLOGY on exact distance fields of a sphere and a torus in a 29 x 25 x 27 grid: closed (every edge twice, once per direction),
   Euler characteristic 2 and 0, positive signed volume, every sphere vertex within the interpolation error of a distance field along
   the longest edge; the same with 156 corners set to exactly zero (zero-area triangles kept); nothing next to unseen grid points."""
import ctypes as C

import numpy as np
import pytest

import tsdf_ref as R
from tests.util import host_shim

F32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int64)
TOPO_DIMS, TOPO_VOXEL, TOPO_ORIGIN = (29, 25, 27), 0.05, (-0.7, -0.6, -0.65)
SPHERE_C, SPHERE_R = (0.013, 0.021, -0.017), 0.45


@pytest.fixture(scope="module")
def shim():
    lib = host_shim("tsdf_math_shim", "tsdf_math.h")
    lib.tm_integrate.restype = C.c_longlong
    lib.tm_integrate.argtypes = [C.c_int] * 3 + [F32P, C.c_float, C.c_float] + [F32P] * 5 + [C.c_int, C.c_int, F32P, F32P] + [C.c_float] * 3 + [F32P]
    lib.tm_cell_pattern.restype = C.c_int
    lib.tm_cell_pattern.argtypes = [C.c_int, I64P]
    lib.tm_triangles.restype = C.c_longlong
    lib.tm_triangles.argtypes = [C.c_int] * 3 + [F32P, C.c_float, F32P, F32P, C.c_float, I64P, C.c_longlong]
    lib.tm_vertices.restype = None
    lib.tm_vertices.argtypes = [C.c_int] * 3 + [F32P, C.c_float] + [F32P] * 4 + [I64P, C.c_longlong, F32P, F32P]
    return lib


def _f(a):
    return a.ctypes.data_as(F32P)


def shim_integrate(shim, vol, dims, out6, w2c, sil_thres=0.99, depth_max=0.0, weight_max=0.0):
    """One view into ``vol`` (float32 arrays, updated in place) through the header; returns the number of points updated."""
    origin, intr = np.array(R.UPDATE_ORIGIN, np.float32), np.array(R.UPDATE_INTR, np.float32)
    planes, m = np.ascontiguousarray(out6, np.float32), np.ascontiguousarray(w2c, np.float32)
    return shim.tm_integrate(*dims, _f(origin), R.UPDATE_VOXEL, R.UPDATE_TRUNC, *(_f(vol[k]) for k in R.VOLUME_ARRAYS),
                             planes.shape[2], planes.shape[1], _f(planes), _f(intr), sil_thres, depth_max, weight_max, _f(m))


def shim_triangles(shim, vol, origin, voxel, min_weight=1.0, capacity=None):
    nz, ny, nx = vol["tsdf"].shape
    o = np.array(origin, np.float32)
    args = (nx, ny, nz, _f(o), voxel, _f(vol["tsdf"]), _f(vol["weight"]), min_weight)
    if capacity is None:
        capacity = shim.tm_triangles(*args, None, 0)
    keys = np.full((max(capacity, 1), 3), -1, dtype=np.int64)
    n = shim.tm_triangles(*args, keys.ctypes.data_as(I64P), capacity)
    return keys[:min(n, capacity)], n


def shim_vertices(shim, vol, origin, voxel, keys):
    nz, ny, nx = vol["tsdf"].shape
    o, keys = np.array(origin, np.float32), np.ascontiguousarray(keys, np.int64)
    pos, col = np.zeros((len(keys), 3), np.float32), np.zeros((len(keys), 3), np.float32)
    shim.tm_vertices(nx, ny, nz, _f(o), voxel, _f(vol["tsdf"]), _f(vol["r"]), _f(vol["g"]), _f(vol["b"]), keys.ctypes.data_as(I64P), len(keys),
                     _f(pos), _f(col))
    return pos, col


# ---------------------------------------------------------------------------------------------------------------- 1. update rule
@pytest.fixture(scope="module")
def planes():
    return R.plane_view(*R.UPDATE_SIZE, R.UPDATE_INTR)


@pytest.mark.parametrize("pose", list(R.UPDATE_POSES))
def test_update_rule_one_view(shim, planes, pose):
    vol = R.new_volume(R.UPDATE_DIMS)
    updated = shim_integrate(shim, vol, R.UPDATE_DIMS, planes, R.UPDATE_POSES[pose])
    fig = R.check_update(vol, R.UPDATE_DIMS, [R.UPDATE_POSES[pose]], planes, pose)
    assert updated == int((vol["weight"] > 0).sum())
    if pose == "behind":
        fresh = R.new_volume(R.UPDATE_DIMS)
        assert updated == 0 and all(vol[k].tobytes() == fresh[k].tobytes() for k in R.VOLUME_ARRAYS)
    else:
        assert fig["updated"] > 0.03                        # (the check is not empty: grid points were updated)
        assert (vol["tsdf"] < 0).any() and (vol["tsdf"] == 1).any()
    if pose == "oblique":
        assert fig["updated"] < 0.10


def test_update_rule_three_views_into_one_volume(shim, planes):
    poses = [R.UPDATE_POSES[k] for k in ("identity", "tilted", "oblique")]
    vol = R.new_volume(R.UPDATE_DIMS)
    for w2c in poses:
        shim_integrate(shim, vol, R.UPDATE_DIMS, planes, w2c)
    R.check_update(vol, R.UPDATE_DIMS, poses, planes, "three views")
    assert vol["weight"].max() >= 2                         # (views overlap: the running mean is exercised)


def test_update_rule_depth_and_weight_limits(shim, planes):
    """depth_max cuts the far part of the plane off; weight_max caps the running mean's memory."""
    poses = [R.UPDATE_POSES["identity"]] * 3
    kw = dict(depth_max=1.3, weight_max=2.0)
    vol = R.new_volume(R.UPDATE_DIMS)
    for w2c in poses:
        shim_integrate(shim, vol, R.UPDATE_DIMS, planes, w2c, **kw)
    R.check_update(vol, R.UPDATE_DIMS, poses, planes, "limits", **kw)
    free = R.new_volume(R.UPDATE_DIMS)
    shim_integrate(shim, free, R.UPDATE_DIMS, planes, poses[0])
    assert vol["weight"].max() == 2 and 0 < (vol["weight"] > 0).sum() < (free["weight"] > 0).sum()


# ---------------------------------------------------------------------------------------------------------------- 2. table
def test_all_256_sign_patterns_match_the_geometric_construction(shim):
    keys = np.zeros((12, 3), dtype=np.int64)
    total = 0
    for mask in range(256):
        n = shim.tm_cell_pattern(mask, keys.ctypes.data_as(I64P))
        want = [[R.edge_key((2, 2, 2), (0, 0, 0), ca, cb) for ca, cb in tri] for tri in R.cell_pattern(mask)]
        assert 0 <= n <= 12 and n == len(want), mask
        assert R.canonical_triangles(keys[:n]) == R.canonical_triangles(want), mask
        total += n
    assert total > 0 and shim.tm_cell_pattern(0, keys.ctypes.data_as(I64P)) == 0 == shim.tm_cell_pattern(255, keys.ctypes.data_as(I64P))


# ---------------------------------------------------------------------------------------------------------------- 3. topology
def _mesh(shim, vol, min_weight=1.0):
    keys, n = shim_triangles(shim, vol, TOPO_ORIGIN, TOPO_VOXEL, min_weight)
    assert n == len(keys)
    assert R.canonical_triangles(keys) == R.canonical_triangles(R.triangles(vol["tsdf"], vol["weight"], min_weight))
    uniq, faces = np.unique(keys.reshape(-1), return_inverse=True)
    pos, col = shim_vertices(shim, vol, TOPO_ORIGIN, TOPO_VOXEL, uniq)
    return uniq, faces.reshape(-1, 3), pos, col


def _areas(pos, faces):
    p = pos.astype(np.float64)[faces]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def test_sphere_is_closed_with_euler_characteristic_2(shim):
    vol = R.field_volume(R.sphere_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, SPHERE_R))
    uniq, faces, pos, col = _mesh(shim, vol)
    V, E, F, closed = R.topology(faces)
    assert closed and V - E + F == 2 and F > 1000
    assert R.signed_volume(pos, faces) > 0
    assert abs(R.signed_volume(pos, faces) - 4 / 3 * np.pi * SPHERE_R ** 3) < 0.02 * 4 / 3 * np.pi * SPHERE_R ** 3
    L = np.sqrt(3) * TOPO_VOXEL
    off = np.abs(np.linalg.norm(pos.astype(np.float64) - np.array(SPHERE_C), axis=1) - SPHERE_R)
    print(f"sphere: {V} vertices, {F} faces, largest |distance - r| {off.max():.3e} (bound {L * L / (8 * (SPHERE_R - L)):.3e})")
    assert off.max() <= L * L / (8 * (SPHERE_R - L))
    # the vertices against the float64 restatement, within 4 x the float32 numpy form's own error
    p64, c64 = R.vertices(uniq, vol, TOPO_ORIGIN, TOPO_VOXEL, np.float64)
    p32, c32 = R.vertices(uniq, vol, TOPO_ORIGIN, TOPO_VOXEL, np.float32)
    assert np.abs(pos - p64).max() <= 4 * np.abs(p32 - p64).max() and np.abs(col - c64).max() <= 4 * np.abs(c32 - c64).max()
    assert col.min() >= 0 and col.max() <= 1 and np.ptp(col, axis=0).min() > 0.3


def test_torus_is_closed_with_euler_characteristic_0(shim):
    vol = R.field_volume(R.torus_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, 0.4, 0.15))
    _, faces, pos, _ = _mesh(shim, vol)
    V, E, F, closed = R.topology(faces)
    assert closed and V - E + F == 0 and F > 1000
    assert R.signed_volume(pos, faces) > 0


def test_corners_that_are_exactly_zero_keep_the_mesh_closed(shim):
    field = R.sphere_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, SPHERE_R).astype(np.float32)
    zero = np.abs(field) < 0.004
    assert zero.sum() == 156
    field[zero] = 0.0
    vol = R.field_volume(field)
    _, faces, pos, _ = _mesh(shim, vol)
    V, E, F, closed = R.topology(faces)
    assert closed and V - E + F == 2
    assert R.signed_volume(pos, faces) > 0
    assert (_areas(pos, faces) == 0).sum() > 0              # kept: dropping them would open the mesh


def test_cells_next_to_unseen_grid_points_emit_nothing(shim):
    vol = R.field_volume(R.sphere_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, SPHERE_R))
    slab = 14                                               # the plane x = origin + 14 voxel cuts the sphere
    vol["weight"][:, :, slab] = 0.0
    uniq, faces, pos, _ = _mesh(shim, vol)
    # no vertex lies on a grid edge that touches the slab ...
    for key in uniq.tolist():
        a, b = R.decode_key(TOPO_DIMS, key)
        assert a[0] != slab and b[0] != slab
    # ... and the mesh is open only there: every boundary edge runs in a grid plane next to the slab
    boundary = R.boundary_edges(faces)
    assert len(boundary) > 20
    planes = (np.float32(TOPO_ORIGIN[0]) + np.float32(TOPO_VOXEL) * np.float32(slab - 1), np.float32(TOPO_ORIGIN[0]) + np.float32(TOPO_VOXEL) * np.float32(slab + 1))
    for a, b in boundary:
        assert pos[a, 0] == pos[b, 0] and pos[a, 0] in planes, (pos[a], pos[b])
    V, E, F, closed = R.topology(faces)
    assert not closed
    # a capacity below the need: the count still reports the need and nothing beyond the capacity is written
    full, n = shim_triangles(shim, vol, TOPO_ORIGIN, TOPO_VOXEL)
    part, n2 = shim_triangles(shim, vol, TOPO_ORIGIN, TOPO_VOXEL, capacity=n // 2)
    assert n2 == n and len(part) == n // 2 and np.array_equal(part, full[:n // 2])
