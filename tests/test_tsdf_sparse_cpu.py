"""The sparse volume without a GPU: the sparse part of splatam_amd/csrc/tsdf_math.h compiled for the host (tests/tsdf_sparse_shim.cpp:
the loop bodies of the kernels of csrc/tsdf_sparse.hip) against the DENSE host model of the same header (tests/tsdf_math_shim.cpp).
Both sides are the same float32 functions, so every comparison is exact; both brick shapes the library accepts are run.

1. COVER: on the update check's planes and poses (identity, tilted, oblique, behind; also with a depth_max that cuts through the
   surface) and grids (37, 21, 13), (40, 21, 13), (68, 9, 10), the bricks ``tsdf_mark_box`` marks over all pixels contain every brick
   that meets the 3 x 3 x 3 neighbourhood of a grid point the dense model updates with f < 0.
2. BITS: mark all views, allocate, integrate the allocated bricks with all views: every allocated point equals the dense model bitwise.
3. MESH: the triangle key set and the vertices of the sparse model equal the dense model's exactly; also on a grid smaller than one
   brick and on one of exactly one brick plus one point per axis.
4. TIGHT: fronto-parallel planes along each axis, the first layer behind the surface the last layer of a brick or the first of the
   next: every marked brick's range along the view axis meets [layer(d) - 2, layer(d + trunc) + 2]."""
import ctypes as C

import numpy as np
import pytest

import tsdf_ref as R
import tsdf_sparse_cases as S
from tests.util import host_shim

F32P, I32P, I64P, U8P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
INTP = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def sparse():
    lib = host_shim("tsdf_sparse_shim", "tsdf_math.h")
    head = [INTP, F32P, C.c_float]                          # dims, origin, voxel
    view = [F32P, F32P, F32P]                               # cam, w2c, out6
    lib.ts_geometry.restype = None
    lib.ts_geometry.argtypes = [INTP, INTP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), INTP]
    lib.ts_mark.restype = C.c_longlong
    lib.ts_mark.argtypes = head + [INTP] + view + [I32P]
    lib.ts_negative.restype = C.c_longlong
    lib.ts_negative.argtypes = head + view + [U8P]
    lib.ts_integrate.restype = C.c_longlong
    lib.ts_integrate.argtypes = head + [INTP] + view + [C.c_int, I32P] + [F32P] * 5
    lib.ts_triangles.restype = C.c_longlong
    lib.ts_triangles.argtypes = head + [INTP, C.c_int, I32P, I32P, F32P, F32P, C.c_float, I64P, C.c_longlong]
    lib.ts_vertices.restype = C.c_longlong
    lib.ts_vertices.argtypes = head + [INTP, I32P] + [F32P] * 5 + [I64P, C.c_longlong, F32P, F32P]
    return lib


@pytest.fixture(scope="module")
def dense():
    lib = host_shim("tsdf_math_shim", "tsdf_math.h")
    lib.tm_integrate.restype = C.c_longlong
    lib.tm_integrate.argtypes = [C.c_int] * 3 + [F32P, C.c_float, C.c_float] + [F32P] * 5 + [C.c_int, C.c_int, F32P, F32P] + [C.c_float] * 3 + [F32P]
    lib.tm_triangles.restype = C.c_longlong
    lib.tm_triangles.argtypes = [C.c_int] * 3 + [F32P, C.c_float, F32P, F32P, C.c_float, I64P, C.c_longlong]
    lib.tm_vertices.restype = None
    lib.tm_vertices.argtypes = [C.c_int] * 3 + [F32P, C.c_float] + [F32P] * 4 + [I64P, C.c_longlong, F32P, F32P]
    return lib


@pytest.fixture(scope="module")
def planes():
    return R.plane_view(*R.UPDATE_SIZE, R.UPDATE_INTR)


def _f(a):
    return a.ctypes.data_as(F32P)


def _ints(v):
    return (C.c_int * len(v))(*v)


class Scene:
    """A grid, a brick shape and the settings every view of it shares; views are (out6, w2c) pairs."""

    def __init__(self, dims, lg, origin=R.UPDATE_ORIGIN, voxel=R.UPDATE_VOXEL, trunc=R.UPDATE_TRUNC, intr=R.UPDATE_INTR, size=R.UPDATE_SIZE,
                 sil_thres=0.99, depth_max=0.0, weight_max=0.0):
        self.dims, self.lg, self.voxel, self.trunc, self.intr = tuple(dims), tuple(lg), voxel, trunc, intr
        self.origin = np.array(origin, np.float32)
        self.limits = (sil_thres, depth_max, weight_max)
        self.cam = np.array([size[0], size[1], *intr, trunc, sil_thres, depth_max, weight_max], np.float32)
        self.bricks = int(np.prod(S.bricks_per_axis(dims, lg)))

    def head(self):
        return _ints(self.dims), _f(self.origin), self.voxel

    @staticmethod
    def view(out6, w2c):
        return np.ascontiguousarray(out6, np.float32), np.ascontiguousarray(w2c, np.float32)

    def mark(self, lib, views):
        flags = np.zeros(self.bricks, np.int32)
        for out6, w2c in views:
            p, m = self.view(out6, w2c)
            lib.ts_mark(*self.head(), _ints(self.lg), _f(self.cam), _f(m), _f(p), flags.ctypes.data_as(I32P))
        return flags

    def negative(self, lib, views):
        nx, ny, nz = self.dims
        neg = np.zeros((nz, ny, nx), np.uint8)
        for out6, w2c in views:
            p, m = self.view(out6, w2c)
            lib.ts_negative(*self.head(), _f(self.cam), _f(m), _f(p), neg.ctypes.data_as(U8P))
        return neg.astype(bool)

    def dense_volume(self, lib, views):
        vol = R.new_volume(self.dims)
        intr = np.array(self.intr, np.float32)
        for out6, w2c in views:
            p, m = self.view(out6, w2c)
            lib.tm_integrate(*self.dims, _f(self.origin), self.voxel, self.trunc, *(_f(vol[k]) for k in R.VOLUME_ARRAYS), p.shape[2], p.shape[1],
                             _f(p), _f(intr), *self.limits, _f(m))
        return vol

    def sparse_volume(self, lib, views, flags):
        """Two phases: (directory, brick_of_slot, pool dict of [slots * 2048] arrays) after every view into every flagged brick."""
        directory, brick_of_slot = S.allocate(flags)
        slots = len(brick_of_slot)
        pool = {k: np.zeros(max(slots, 1) * S.BRICK_POINTS, np.float32) for k in R.VOLUME_ARRAYS}
        pool["tsdf"][:] = 1
        for out6, w2c in views:
            p, m = self.view(out6, w2c)
            lib.ts_integrate(*self.head(), _ints(self.lg), _f(self.cam), _f(m), _f(p), slots, brick_of_slot.ctypes.data_as(I32P),
                             *(_f(pool[k]) for k in R.VOLUME_ARRAYS))
        return directory, brick_of_slot, pool


def _update_views(planes, names):
    return [(planes, R.UPDATE_POSES[n]) for n in names]


def assert_covered(scene, sparse, views, what):
    flags = scene.mark(sparse, views)
    negative = scene.negative(sparse, views)
    needed = S.needed_bricks(negative, scene.lg)
    missing = needed & (flags == 0)
    print(f"\n{what}: {int(negative.sum())} grid points with f < 0, {int(needed.sum())} bricks needed, {int((flags != 0).sum())} marked of {scene.bricks}")
    assert not missing.any(), (what, np.nonzero(missing)[0].tolist())
    return flags, negative


# ---------------------------------------------------------------------------------------------------------------- brick geometry
@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_brick_index_and_local_offset_round_trip(sparse, shape):
    lg = S.SHAPES[shape]
    dims = (70, 19, 21)
    per = S.bricks_per_axis(dims, lg)
    out, got_per = (C.c_longlong * 5)(), (C.c_int * 3)()
    seen = set()
    rng = np.random.default_rng(0)
    points = [(0, 0, 0), (69, 18, 20), (63, 3, 7), (64, 4, 8), (15, 15, 7), (16, 16, 8)] + [tuple(int(rng.integers(d)) for d in dims) for _ in range(200)]
    for i, j, k in points:
        sparse.ts_geometry(_ints(dims), _ints(lg), i, j, k, out, got_per)
        assert tuple(got_per) == per and tuple(out[2:5]) == (i, j, k)
        assert out[0] == ((k >> lg[2]) * per[1] + (j >> lg[1])) * per[0] + (i >> lg[0]) and 0 <= out[1] < S.BRICK_POINTS
        seen.add((out[0], out[1]))
    assert len(seen) == len(set(points))                    # (brick, local) names a grid point
    assert S.point_offsets(dims, lg, np.arange(int(np.prod(per))))[20, 18, 69] == out_for(sparse, dims, lg, (69, 18, 20))


def out_for(sparse, dims, lg, p):
    out, per = (C.c_longlong * 5)(), (C.c_int * 3)()
    sparse.ts_geometry(_ints(dims), _ints(lg), *p, out, per)
    return out[0] * S.BRICK_POINTS + out[1]


# ---------------------------------------------------------------------------------------------------------------- 1. cover
@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("dims", S.UPDATE_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_marked_bricks_cover_every_negative_update(sparse, planes, dims, shape):
    lg = S.SHAPES[shape]
    totals = []
    for limits in (dict(), dict(depth_max=1.3)):            # (1.3: the plane's depth at the image centre -- the limit cuts through it)
        scene = Scene(dims, lg, **limits)
        for pose in R.UPDATE_POSES:
            flags, negative = assert_covered(scene, sparse, _update_views(planes, [pose]), f"{dims} {shape} {pose} {limits}")
            if pose == "behind":
                assert not flags.any() and not negative.any()
        flags, negative = assert_covered(scene, sparse, _update_views(planes, list(R.UPDATE_POSES)), f"{dims} {shape} all views {limits}")
        assert negative.sum() > 100 and 0 < (flags != 0).sum()
        totals.append(int(negative.sum()))
    assert totals[1] < totals[0]                            # (the limit took negative updates away: it cut through the surface)


# ---------------------------------------------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("dims", S.UPDATE_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_allocated_points_equal_the_dense_model_bitwise(sparse, dense, planes, dims, shape):
    lg = S.SHAPES[shape]
    for limits in (dict(), dict(depth_max=1.3, weight_max=2.0)):
        scene = Scene(dims, lg, **limits)
        views = _update_views(planes, list(R.UPDATE_POSES) + ["identity"])
        flags = scene.mark(sparse, views)
        directory, brick_of_slot, pool = scene.sparse_volume(sparse, views, flags)
        want = scene.dense_volume(dense, views)
        at = S.point_offsets(dims, lg, directory)
        have = at >= 0
        assert have.sum() > 1000 and len(brick_of_slot) == (flags != 0).sum()
        for k in R.VOLUME_ARRAYS:
            assert pool[k][at[have]].tobytes() == want[k][have].tobytes(), (k, limits)
        assert (want["tsdf"][have] < 0).any() and (want["weight"][have] >= 2).any()
        assert not (want["tsdf"][~have] < 0).any()           # every negative point is allocated
        # the pool's points outside the grid (edge bricks) keep the reset values
        used = np.zeros(len(pool["tsdf"]), bool)
        used[at[have]] = True
        assert (pool["tsdf"][~used] == 1).all() and all((pool[k][~used] == 0).all() for k in ("weight", "r", "g", "b"))


# ---------------------------------------------------------------------------------------------------------------- 3. mesh
MESH_GRIDS = {
    "37x21x13": ((37, 21, 13), R.UPDATE_ORIGIN), "40x21x13": ((40, 21, 13), R.UPDATE_ORIGIN), "68x9x10": ((68, 9, 10), R.UPDATE_ORIGIN),
    "below-one-brick": ((9, 4, 5), (-0.213, -0.107, 1.211)),                       # smaller than either brick shape
    "one-brick-plus-one-16x16x8": ((17, 17, 9), (-0.413, -0.407, 1.111)),
    "one-brick-plus-one-64x4x8": ((65, 5, 9), (-1.613, -0.107, 1.111)),
}


@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("name", list(MESH_GRIDS))
def test_sparse_mesh_equals_the_dense_mesh(sparse, dense, planes, name, shape):
    lg = S.SHAPES[shape]
    dims, origin = MESH_GRIDS[name]
    scene = Scene(dims, lg, origin=origin)
    views = _update_views(planes, S.THREE_POSES)
    flags = scene.mark(sparse, views)
    directory, brick_of_slot, pool = scene.sparse_volume(sparse, views, flags)
    want = scene.dense_volume(dense, views)
    o = np.array(origin, np.float32)
    n_dense = dense.tm_triangles(*dims, _f(o), scene.voxel, _f(want["tsdf"]), _f(want["weight"]), 1.0, None, 0)
    keys_dense = np.zeros((max(n_dense, 1), 3), np.int64)
    dense.tm_triangles(*dims, _f(o), scene.voxel, _f(want["tsdf"]), _f(want["weight"]), 1.0, keys_dense.ctypes.data_as(I64P), n_dense)
    args = (*scene.head(), _ints(lg), len(brick_of_slot), brick_of_slot.ctypes.data_as(I32P), directory.ctypes.data_as(I32P), _f(pool["tsdf"]),
            _f(pool["weight"]), 1.0)
    n_sparse = sparse.ts_triangles(*args, None, 0)
    keys_sparse = np.zeros((max(n_sparse, 1), 3), np.int64)
    sparse.ts_triangles(*args, keys_sparse.ctypes.data_as(I64P), n_sparse)
    print(f"\n{name} {shape}: {n_dense} triangles, {len(brick_of_slot)} of {scene.bricks} bricks")
    assert n_sparse == n_dense > 20
    assert R.canonical_triangles(keys_sparse[:n_sparse]) == R.canonical_triangles(keys_dense[:n_dense])
    uniq = np.unique(keys_dense[:n_dense])
    pos_d, col_d = np.zeros((len(uniq), 3), np.float32), np.zeros((len(uniq), 3), np.float32)
    dense.tm_vertices(*dims, _f(o), scene.voxel, *(_f(want[k]) for k in ("tsdf", "r", "g", "b")), uniq.ctypes.data_as(I64P), len(uniq), _f(pos_d), _f(col_d))
    pos_s, col_s = np.full((len(uniq), 3), 7, np.float32), np.full((len(uniq), 3), 7, np.float32)
    missing = sparse.ts_vertices(*scene.head(), _ints(lg), directory.ctypes.data_as(I32P), *(_f(pool[k]) for k in R.VOLUME_ARRAYS),
                                 uniq.ctypes.data_as(I64P), len(uniq), _f(pos_s), _f(col_s))
    assert missing == 0 and pos_s.tobytes() == pos_d.tobytes() and col_s.tobytes() == col_d.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 4. tight
@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("axis,first_of_next", S.AXIS_CASES, ids=S.AXIS_IDS)
def test_the_mark_is_tight_on_planes_at_brick_boundaries(sparse, axis, first_of_next, shape):
    lg = S.SHAPES[shape]
    case = S.axis_case(axis, lg, first_of_next)
    scene = Scene(case["dims"], lg, origin=case["origin"], voxel=case["voxel"], trunc=case["trunc"], intr=case["intr"])
    views = [(case["out6"], case["w2c"])]
    flags, negative = assert_covered(scene, sparse, views, f"axis {axis} L {case['L']} {shape}")
    layers = np.nonzero(negative.any(axis=tuple(a for a in range(3) if a != 2 - axis)))[0]
    assert layers.tolist() == list(range(case["L"], case["L"] + 4))              # the band is layers L .. L + 3, as the case says
    S.assert_mark_is_tight(case, lg, flags)
