"""Marching cubes on the device (``splat_tsdf_cubes`` / ``splat_tsdf_sparse_cubes`` through ``extract(method="cubes")``) against the host
model of the same header (tests/tsdf_cubes_shim.cpp, itself held to the rule by tests/test_tsdf_cubes_cpu.py).

1. UPLOADED VOLUMES (sphere, torus, exact zeros, an unseen plane, sign noise) at 29 x 25 x 27, 68 x 7 x 5 (two 64-cell blocks along x,
   ragged in y) and 66 x 6 x 3: the key triples as a set and the canonical ``Mesh`` bytes equal the host model's; capacity 0, n - 1
   and the default give the same mesh and the same count, and nothing is stored at or beyond a capacity.
2. The library's copy of the table equals the restatement.
3. SPARSE: the sparse cubes mesh equals the dense cubes mesh byte for byte, for both brick shapes, on the fused volumes and an uploaded
   field of tests/tsdf_sparse_cases.py's kind.
4. END TO END on the small engine of tests/test_gpu_mesh.py: ``extract_mesh(..., method="cubes")`` is the host model applied to the
   volume read back, has fewer faces and vertices than the tetrahedra mesh, which is byte for byte what it was with ``method`` omitted;
   two runs give the same bytes; ``clean_mesh`` and ``score_with_views`` take the mesh, which scores exactly 0 against itself.
5. ``SlamSession.extract_mesh(method="cubes", path=...)`` and ``python -m splatam_amd.mesh --method cubes`` write a PLY that
   ``load_mesh_ply`` reads back to the same arrays."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tsdf_cubes_ref as Q
import tsdf_ref as R
import tsdf_sparse_cases as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = -7
VOXEL = 0.05
DIMS = {"29x25x27": (29, 25, 27), "68x7x5": (68, 7, 5), "66x6x3": (66, 6, 3)}
KINDS = ("sphere", "torus", "zeros", "unseen", "noise")


def _origin(dims):
    """The grid centred a little off the origin, so that the fields' centre is between grid points."""
    return tuple(float(-VOXEL * (d - 1) / 2 + o) for d, o in zip(dims, (0.013, 0.021, -0.017)))


@functools.lru_cache(maxsize=None)
def _volume(kind, grid):
    dims = DIMS[grid]
    origin = _origin(dims)
    if kind == "noise":
        return Q.noise_volume(dims, seed=3)
    if kind == "torus":
        return R.field_volume(R.torus_field(dims, origin, VOXEL, (0.0, 0.0, 0.0), 0.4, 0.15))
    field = R.sphere_field(dims, origin, VOXEL, (0.0, 0.0, 0.0), 0.45)
    if kind == "zeros":
        field = field.astype(np.float32)
        field[np.abs(field) < 0.004] = 0.0
    vol = R.field_volume(field)
    if kind == "unseen":
        vol["weight"][:, :, dims[0] // 2] = 0.0            # (a plane through the middle of the sphere)
    return vol


@functools.lru_cache(maxsize=None)
def _shim():
    import test_tsdf_cubes_cpu as TC
    return TC, TC.load_cubes_shim()


def _upload(vol, origin):
    from splatam_amd.mesh import TsdfVolume
    nz, ny, nx = vol["tsdf"].shape
    volume = TsdfVolume(origin, (nx, ny, nz), VOXEL)
    for k, t in volume.arrays().items():
        t.copy_(torch.from_numpy(np.ascontiguousarray(vol[k], np.float32)))
    return volume


def _raw(volume, capacity, entry="splat_tsdf_cubes", guard=64):
    """The entry point into a guarded buffer: (keys [min(n, capacity), 3] on the host, n)."""
    from splatam_amd import _capi
    flat = torch.full((3 * capacity + guard,), GUARD, dtype=torch.int64, device="cuda")
    count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    _capi.check(getattr(_capi.lib(), entry)(C.byref(volume.struct), 1.0, flat.data_ptr() if capacity else None, capacity, count.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), entry)
    torch.cuda.synchronize()
    n, host = int(count.item()), flat.cpu().numpy()
    assert (host[3 * capacity:] == GUARD).all(), "a store at or beyond the capacity"
    assert (host[3 * min(n, capacity):3 * capacity] == GUARD).all()
    return host[:3 * min(n, capacity)].reshape(-1, 3), n


def _assert_is_host_mesh(mesh, volume, want):
    uniq, pos, faces, col = want
    torch.cuda.synchronize()
    assert mesh.faces.dtype == torch.int32 and mesh.vertices.dtype == torch.float32 and mesh.colors.dtype == torch.float32
    assert mesh.faces.cpu().numpy().tobytes() == faces.tobytes() and mesh.faces.shape == faces.shape
    assert mesh.vertices.cpu().numpy().tobytes() == pos.tobytes() and mesh.colors.cpu().numpy().tobytes() == col.tobytes()
    if len(faces):
        assert np.array_equal(volume.last_keys.cpu().numpy(), uniq)
    assert volume.last_triangle_count == len(faces)


# ---------------------------------------------------------------------------------------------------------------- 1. uploaded volumes
@pytest.mark.parametrize("grid", list(DIMS))
@pytest.mark.parametrize("kind", KINDS)
def test_uploaded_volumes_against_the_host_model(kind, grid):
    TC, shim = _shim()
    vol, origin = _volume(kind, grid), _origin(DIMS[grid])
    volume = _upload(vol, origin)
    host_keys, need = TC.shim_cubes(shim, vol, origin, VOXEL)
    want = TC.host_mesh(shim, vol, origin, VOXEL)
    assert need == len(host_keys) > (1000 if grid == "29x25x27" else 40)
    keys, n = _raw(volume, need + 100)
    assert n == need and R.canonical_triangles(keys) == R.canonical_triangles(host_keys)       # the key triples, as a set
    assert set((keys & 7).reshape(-1).tolist()) <= {1, 2, 4}
    # capacities: 0 (the count alone), n - 1 (one short), the default -- the same count, the same mesh after extract's rerun
    nothing, n0 = _raw(volume, 0)
    part, n1 = _raw(volume, need - 1)
    assert n0 == need == n1 and len(nothing) == 0 and len(part) == need - 1
    assert set(R.canonical_triangles(part)) <= set(R.canonical_triangles(host_keys))
    for capacity in (0, need - 1, None):
        _assert_is_host_mesh(volume.extract(capacity=capacity, method="cubes"), volume, want)
    # and beside it the tetrahedra pass is what it was: more triangles, the same axis-edge vertices
    tets = volume.extract()
    assert tets.faces.shape[0] > 2 * need
    tet_keys = volume.last_keys
    axis = ((tet_keys & 7) == 1) | ((tet_keys & 7) == 2) | ((tet_keys & 7) == 4)
    assert np.array_equal(tet_keys[axis].cpu().numpy(), want[0])
    assert tets.vertices[axis].cpu().numpy().tobytes() == want[1].tobytes() and tets.colors[axis].cpu().numpy().tobytes() == want[3].tobytes()


def test_a_volume_without_a_surface_and_a_volume_without_a_cell_give_empty_meshes():
    from splatam_amd.mesh import TsdfVolume
    for dims in ((9, 5, 3), (1, 1, 1), (70, 1, 4)):
        volume = TsdfVolume((0, 0, 0), dims, 0.1)
        mesh = volume.extract(method="cubes")
        assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and mesh.colors.shape == (0, 3) and volume.last_triangle_count == 0
    with pytest.raises(ValueError, match="unknown surface method"):
        volume.extract(method="dual")


# ---------------------------------------------------------------------------------------------------------------- 2. table
def test_the_library_table_is_the_rule():
    from splatam_amd.mesh import cubes_table
    got, want = cubes_table(), Q.table()
    assert got.dtype == np.int8 and got.shape == (256, 16) and got.tolist() == want.tolist()


# ---------------------------------------------------------------------------------------------------------------- 3. sparse
BRICKS = {name: tuple(1 << l for l in lg) for name, lg in S.SHAPES.items()}


def _assert_same_mesh(a, b, least):
    torch.cuda.synchronize()
    assert b.faces.shape[0] >= least
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("dims", S.UPDATE_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_sparse_cubes_of_fused_views_is_the_dense_cubes_mesh(dims, shape):
    from splatam_amd.mesh import SparseTsdfVolume, TsdfVolume
    out6 = torch.from_numpy(R.plane_view(*R.UPDATE_SIZE, R.UPDATE_INTR)).cuda()
    poses = [torch.from_numpy(np.ascontiguousarray(R.UPDATE_POSES[k], np.float32)).cuda() for k in S.THREE_POSES]
    sparse = SparseTsdfVolume(R.UPDATE_ORIGIN, dims, R.UPDATE_VOXEL, R.UPDATE_TRUNC, brick=BRICKS[shape])
    dense = TsdfVolume(R.UPDATE_ORIGIN, dims, R.UPDATE_VOXEL, R.UPDATE_TRUNC)
    for pose in poses:
        sparse.mark(out6, pose, R.UPDATE_INTR)
    assert sparse.allocate() > 0
    for pose in poses:
        sparse.integrate(out6, pose, R.UPDATE_INTR)
        dense.integrate(out6, pose, R.UPDATE_INTR)
    want = dense.extract(method="cubes")
    need = dense.last_triangle_count
    _assert_same_mesh(sparse.extract(method="cubes"), want, 100)
    assert sparse.last_triangle_count == need
    _assert_same_mesh(sparse.extract(capacity=need - 1, method="cubes"), want, 100)
    _assert_same_mesh(sparse.extract(capacity=0, method="cubes"), want, 100)
    keys, n = _raw(sparse, need + 100, "splat_tsdf_sparse_cubes")
    part, n1 = _raw(sparse, need - 1, "splat_tsdf_sparse_cubes")
    assert n == need == n1 and len(part) == need - 1
    assert R.canonical_triangles(keys) == R.canonical_triangles(_raw(dense, need, "splat_tsdf_cubes")[0])
    _assert_same_mesh(sparse.extract(), dense.extract(), need)                  # (the tetrahedra beside it, as before)


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_sparse_cubes_of_an_uploaded_sphere_is_the_host_mesh(shape):
    from splatam_amd.mesh import SparseTsdfVolume
    TC, shim = _shim()
    grid = "29x25x27"
    vol, origin = _volume("zeros", grid), _origin(DIMS[grid])
    dense = _upload(vol, origin)
    sparse = SparseTsdfVolume(origin, DIMS[grid], VOXEL, brick=BRICKS[shape])
    needed = S.needed_bricks(vol["tsdf"] < 0, S.SHAPES[shape])
    sparse.flags.copy_(torch.from_numpy(needed.astype(np.int32)))
    assert sparse.allocate() == int(needed.sum())
    at = sparse.point_offsets()
    have = at >= 0
    for n, k in enumerate(R.VOLUME_ARRAYS):
        sparse.pool.view(5, -1)[n][at[have]] = dense.arrays()[k][have]
    _assert_is_host_mesh(sparse.extract(method="cubes"), sparse, TC.host_mesh(shim, vol, origin, VOXEL))


# ---------------------------------------------------------------------------------------------------------------- 4. end to end
def test_extract_mesh_with_cubes_end_to_end(tmp_path):
    import test_gpu_mesh as T
    from splatam_amd import mesh as M
    from splatam_amd import mesh_score as MS
    from splatam_amd.mesh_clean import clean_mesh
    TC, shim = _shim()
    eng, intr = T._engine()
    args = (eng, [0, 1, 2], (T.W, T.H), intr)
    with torch.no_grad():
        cubes, volume = M.extract_mesh(*args, return_volume=True, method="cubes", **T.E2E)
        again = M.extract_mesh(*args, method="cubes", **T.E2E)
        sparse = M.extract_mesh(*args, method="cubes", sparse=True, **T.E2E)
        omitted = M.extract_mesh(*args, **T.E2E)
        named = M.extract_mesh(*args, method="tetrahedra", **T.E2E)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in volume.arrays().items()}
    want = TC.host_mesh(shim, got, volume.origin, 0.05)
    _assert_is_host_mesh(cubes, volume, want)
    _assert_same_mesh(again, cubes, 200)
    _assert_same_mesh(sparse, cubes, 200)
    _assert_same_mesh(named, omitted, 500)
    print(f"cubes {cubes.faces.shape[0]} faces, {cubes.vertices.shape[0]} vertices; tetrahedra {omitted.faces.shape[0]} faces, {omitted.vertices.shape[0]} vertices")
    assert cubes.faces.shape[0] < omitted.faces.shape[0] and cubes.vertices.shape[0] < omitted.vertices.shape[0]
    # downstream: the cleaner and the scorer take the mesh; against itself it scores exactly 0
    cleaned, found = clean_mesh(cubes, min_vertices=20, report=True)
    assert 0 < cleaned.faces.shape[0] <= cubes.faces.shape[0]
    score = MS.score_with_views(cubes, cubes, samples=20_000)
    assert score["accuracy_cm"] == 0.0 and score["completion_cm"] == 0.0 and score["completion_ratio"] == 100.0
    with pytest.raises(ValueError, match="unknown surface method"):
        M.extract_mesh(*args, method="dual", **T.E2E)


# ---------------------------------------------------------------------------------------------------------------- 5. session, tool
def _assert_ply_reads_back(path, mesh):
    from splatam_amd.export import load_mesh_ply
    pos, faces, col = load_mesh_ply(path)
    assert pos.tobytes() == mesh.vertices.cpu().numpy().tobytes() and np.array_equal(faces, mesh.faces.cpu().numpy()) and len(faces) > 50
    assert np.array_equal(np.rint(col * 255.0).astype(np.uint8), np.rint(np.clip(mesh.colors.cpu().numpy(), 0, 1) * 255.0).astype(np.uint8))


def test_session_extract_mesh_writes_the_cubes_mesh(tmp_path):
    import test_gpu_mesh as T
    from splatam_amd.session import SlamSession
    ds, cfg = T._sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(voxel_size=0.05, sil_thres=0.5)
    with SlamSession(cfg, len(ds)) as session:
        for t in range(len(ds)):
            session.add_frame(*ds[t])
        path = str(tmp_path / "cubes.ply")
        cubes = session.extract_mesh(method="cubes", path=path, **kw)
        tets = session.extract_mesh(**kw)
        torch.cuda.synchronize()
        _assert_ply_reads_back(path, cubes)
        assert cubes.faces.shape[0] < tets.faces.shape[0] and cubes.vertices.shape[0] < tets.vertices.shape[0]
        with pytest.raises(ValueError, match="unknown surface method"):
            session.extract_mesh(method="dual")
        session.finish()


def test_the_tool_writes_the_cubes_mesh_of_a_saved_map(tmp_path):
    import test_gpu_mesh as T
    from splatam_amd import mesh as M
    from splatam_amd import pipeline
    ds, cfg = T._sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    params, variables, stats = pipeline.rgbd_slam(ds, cfg, engine="fused")
    out = {n: v for n, v in params.items()}
    out['timestep'] = variables['timestep']
    out['intrinsics'] = ds[0][2][:3, :3].cpu().numpy()
    out['w2c'] = torch.linalg.inv(ds[0][3]).cpu().numpy()
    out['org_width'], out['org_height'] = 72, 40
    out['keyframe_time_indices'] = np.array(stats['keyframe_time_indices'])
    saved = pipeline.save_params(out, str(tmp_path / "run"))
    ply = str(tmp_path / "run" / "mesh.ply")
    root = os.path.dirname(HERE)
    done = subprocess.run([sys.executable, "-m", "splatam_amd.mesh", saved, "--out", ply, "--voxel", "0.05", "--sil-thres", "0.5", "--method", "cubes"],
                          cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    mesh = M.mesh_from_params(saved, str(tmp_path / "again.ply"), voxel_size=0.05, sil_thres=0.5, verbose=False, method="cubes")
    _assert_ply_reads_back(ply, mesh)
    assert open(ply, "rb").read() == open(tmp_path / "again.ply", "rb").read()
    assert f"{mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces" in done.stdout
