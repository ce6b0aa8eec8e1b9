"""The sparse volume on the device (csrc/tsdf_sparse.hip through ``splatam_amd.mesh.SparseTsdfVolume``, ``extract_mesh(..., sparse=True)``,
``SlamSession.extract_mesh`` and ``python -m splatam_amd.mesh --sparse``) against the DENSE volume on the same device: the two run the
same float32 functions, so every comparison is exact.  Both brick shapes the library accepts are run.

  5. S1: after one view into a fresh dense volume ``tsdf < 0`` is exactly the set of grid points updated with f < 0; the bricks S1
     marks contain every brick that meets its 3 x 3 x 3 dilation -- on the update check's planes, poses and grids and on the six
     fronto-parallel planes at brick boundaries, where the mark is also tight.  The ``behind`` pose, a silhouette of 0.5 everywhere
     and NaN depth mark nothing; a non-zero ``skip`` leaves the flags bit-unchanged and counts 1.
  6. S2: ``to_dense()`` after two-phase fusion of three poses equals the dense volume on every allocated point, bit for bit, also at
     depth_max = 1.3 / weight_max = 2 with out6 a view at an odd float offset into a larger buffer; unallocated points hold the reset
     values; a guard region behind the pool is intact.
  7. S3 / S4: ``extract()`` of the sparse volume equals ``extract()`` of the dense one (``torch.equal`` on vertices, faces, colours) on
     item 6's volumes and on the uploaded sphere, torus, zeroed-corner sphere and slab fields (29 x 25 x 27) in a sparse volume whose
     bricks come from the field's own dilated negative set; at half the triangle capacity the count reports the need and a guard
     behind ``keys`` is intact; two extractions are identical.
  8. End to end on ``slam.synthetic_params(4000, 160, 112, ...)``, time indices 0..2, voxel 0.05: ``extract_mesh(..., sparse=True)``
     equals ``extract_mesh(...)`` tensor for tensor; the map, Adam moments, variables and current camera are bit-equal before and
     after; a view camera with too small a list capacity is repeated (in the mark pass, whose ``check_overflow`` sizes the lists; the
     integrate pass repeats whatever it still turns away) and gives the same mesh; a box ``plan_volume`` refuses as a dense
     volume gives a non-empty mesh from a pool below ``max_bytes``, and a ValueError stating the need when ``max_bytes`` is below it.
  9. ``SlamSession.extract_mesh(path, sparse=True)`` and ``python -m splatam_amd.mesh ... --sparse`` write the dense PLY, byte for byte."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tsdf_ref as R
import tsdf_sparse_cases as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = -7
BRICKS = {name: tuple(1 << l for l in lg) for name, lg in S.SHAPES.items()}
GRIDS = {"37x21x13": ((37, 21, 13), R.UPDATE_ORIGIN), "40x21x13": ((40, 21, 13), R.UPDATE_ORIGIN), "68x9x10": ((68, 9, 10), R.UPDATE_ORIGIN),
         "16x16x8": ((16, 16, 8), (-0.413, -0.407, 1.111))}          # (the last: exactly one 16 x 16 x 8 brick, around the plane)


def _w2c(pose):
    return torch.from_numpy(np.ascontiguousarray(pose, np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def _planes():
    return R.plane_view(*R.UPDATE_SIZE, R.UPDATE_INTR)


def _volumes(dims, origin, shape, voxel=R.UPDATE_VOXEL, trunc=R.UPDATE_TRUNC, spare=0):
    from splatam_amd.mesh import SparseTsdfVolume, TsdfVolume
    bricks = int(np.prod(S.bricks_per_axis(dims, S.SHAPES[shape])))
    sparse = SparseTsdfVolume(origin, dims, voxel, trunc, capacity_bricks=bricks + spare if spare else 0, brick=BRICKS[shape])
    return sparse, TsdfVolume(origin, dims, voxel, trunc)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_the_library_lists_its_brick_shapes():
    from splatam_amd import mesh
    shapes = mesh.brick_shapes()
    assert sorted(shapes) == sorted(BRICKS.values()) and all(x * y * z == mesh.BRICK_POINTS == S.BRICK_POINTS and x % 4 == 0 for x, y, z in shapes)
    with pytest.raises(ValueError, match="brick shape"):
        mesh.SparseTsdfVolume((0, 0, 0), (8, 8, 8), 0.1, brick=(8, 16, 16))


# ---------------------------------------------------------------------------------------------------------------- 5. S1
def _assert_marks_cover(sparse, dense, out6, w2c, intr, what, **kw):
    """One view into the fresh ``dense`` volume and marked in ``sparse``: the marked bricks contain the needed ones.  Returns (flags,
    negative) on the host."""
    dense.reset()
    sparse.flags.zero_()
    dense.integrate(out6, w2c, intr, **kw)
    sparse.mark(out6, w2c, intr, **kw)
    torch.cuda.synchronize()
    negative = (dense.tsdf < 0).cpu().numpy()
    flags = sparse.flags.cpu().numpy()
    lg = tuple(int(b).bit_length() - 1 for b in sparse.brick)
    needed = S.needed_bricks(negative, lg)
    print(f"\n{what}: {int(negative.sum())} grid points below zero, {int(needed.sum())} bricks needed, {int((flags != 0).sum())} marked of {len(flags)}")
    assert set(np.unique(flags).tolist()) <= {0, 1} and not (needed & (flags == 0)).any(), what
    return flags, negative


@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("grid", ("37x21x13", "40x21x13", "68x9x10"))
def test_marked_bricks_cover_what_one_view_needs(grid, shape):
    dims, origin = GRIDS[grid]
    sparse, dense = _volumes(dims, origin, shape)
    out6 = torch.from_numpy(_planes()).cuda()
    total = 0
    for kw in (dict(), dict(depth_max=1.3)):
        for pose in R.UPDATE_POSES:
            flags, negative = _assert_marks_cover(sparse, dense, out6, _w2c(R.UPDATE_POSES[pose]), R.UPDATE_INTR, f"{grid} {shape} {pose} {kw}", **kw)
            total += int(negative.sum())
            if pose == "behind":
                assert not flags.any() and not negative.any()
    assert total > 500 and int(sparse.mark_skipped.item()) == 0


@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("axis,first_of_next", S.AXIS_CASES, ids=S.AXIS_IDS)
def test_the_mark_covers_and_is_tight_at_brick_boundaries(axis, first_of_next, shape):
    lg = S.SHAPES[shape]
    case = S.axis_case(axis, lg, first_of_next)
    sparse, dense = _volumes(case["dims"], case["origin"], shape, case["voxel"], case["trunc"])
    flags, negative = _assert_marks_cover(sparse, dense, torch.from_numpy(case["out6"]).cuda(), _w2c(case["w2c"]), case["intr"],
                                          f"axis {axis} L {case['L']} {shape}")
    layers = np.nonzero(negative.any(axis=tuple(a for a in range(3) if a != 2 - axis)))[0]
    assert layers.tolist() == list(range(case["L"], case["L"] + 4))
    S.assert_mark_is_tight(case, lg, flags)


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_views_that_see_nothing_mark_nothing_and_a_skipped_view_is_counted(shape):
    dims, origin = GRIDS["40x21x13"]
    sparse, _ = _volumes(dims, origin, shape)
    planes = _planes()
    identity = _w2c(R.UPDATE_POSES["identity"])
    thin = planes.copy()
    thin[:5] *= 0.5 / np.maximum(thin[4], 1e-6)                                      # the silhouette 0.5 everywhere, depth and colour with it
    assert np.allclose(thin[4], 0.5)
    nan = planes.copy()
    nan[3] = np.nan
    for what, out6 in (("silhouette 0.5", thin), ("NaN depth", nan)):
        sparse.mark(torch.from_numpy(out6).cuda(), identity, R.UPDATE_INTR)
        assert not sparse.flags.any().item(), what
    out6 = torch.from_numpy(planes).cuda()
    sparse.mark(out6, identity, R.UPDATE_INTR)
    before = sparse.flags.clone()
    assert 0 < int(before.sum().item())
    skip = torch.tensor([2], dtype=torch.int32, device="cuda")
    sparse.mark(out6, _w2c(R.UPDATE_POSES["oblique"]), R.UPDATE_INTR, skip=skip)
    assert torch.equal(before, sparse.flags) and int(sparse.mark_skipped.item()) == 1 and int(sparse.skipped.item()) == 0
    skip.zero_()
    sparse.mark(out6, _w2c(R.UPDATE_POSES["oblique"]), R.UPDATE_INTR, skip=skip)
    assert int(sparse.mark_skipped.item()) == 1 and int((sparse.flags - before).min().item()) >= 0


# ---------------------------------------------------------------------------------------------------------------- 6. S2
def _fuse_two_phase(grid, shape, limits):
    """(sparse, dense) after the three poses (the first once more, so that weight_max bites): marked, allocated, integrated; out6 a view
    at an odd float offset into a larger buffer when ``limits``.  The pool has two spare bricks, filled with GUARD before integration."""
    dims, origin = GRIDS[grid]
    sparse, dense = _volumes(dims, origin, shape, spare=2)
    W, H = R.UPDATE_SIZE
    if limits:
        big = torch.full((3 + 6 * H * W + 64,), float("nan"), dtype=torch.float32, device="cuda")
        out6 = big[3:3 + 6 * H * W].view(6, H, W)
        out6.copy_(torch.from_numpy(_planes()))
        assert out6.data_ptr() % 16 != 0
    else:
        out6 = torch.from_numpy(_planes()).cuda()
    kw = dict(depth_max=1.3, weight_max=2.0) if limits else {}
    poses = [_w2c(R.UPDATE_POSES[k]) for k in S.THREE_POSES + ("identity",)]
    for pose in poses:
        sparse.mark(out6, pose, R.UPDATE_INTR, **{k: v for k, v in kw.items() if k != "weight_max"})
    count = sparse.marked_count()
    assert sparse.allocate() == count == sparse.slots > 0 and sparse.marked_count() == 0
    assert sparse.bytes() == (20 * 2048 + 4) * count + 8 * sparse.num_bricks
    sparse.pool[:, sparse.slots:] = GUARD
    for pose in poses:
        sparse.integrate(out6, pose, R.UPDATE_INTR, **kw)
        dense.integrate(out6, pose, R.UPDATE_INTR, **kw)
    torch.cuda.synchronize()
    return sparse, dense


@functools.lru_cache(maxsize=None)
def _fused(grid, shape, limits):
    return _fuse_two_phase(grid, shape, limits)


@pytest.mark.parametrize("limits", (False, True), ids=("plain", "limits-odd-offset"))
@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_two_phase_fusion_holds_the_dense_volumes_bits(grid, shape, limits):
    sparse, dense = _fused(grid, shape, limits)
    assert (sparse.pool[:, sparse.slots:] == GUARD).all().item() and sparse.pool.shape[1] == sparse.slots + 2 + (sparse.num_bricks - sparse.slots)
    got = sparse.to_dense()
    have = sparse.point_offsets() >= 0
    fresh = R.new_volume(sparse.dims)
    for k in R.VOLUME_ARRAYS:
        a, b = got.arrays()[k], dense.arrays()[k]
        assert torch.equal(_bits(a[have]), _bits(b[have])), k
        assert torch.equal(_bits(a[~have]), _bits(torch.from_numpy(fresh[k]).cuda()[~have])), k
    assert (dense.tsdf < 0).any().item() and not (dense.tsdf[~have] < 0).any().item()
    assert float(dense.weight.max().item()) == 2 if limits else float(dense.weight.max().item()) >= 3      # (views overlap; weight_max bites)
    assert int(sparse.skipped.item()) == 0
    # the brick list and the directory are each other's inverse
    slots = torch.arange(sparse.slots, dtype=torch.int32, device="cuda")
    assert torch.equal(sparse.directory[sparse.brick_of_slot[:sparse.slots].long()], slots)
    assert int((sparse.directory >= 0).sum().item()) == sparse.slots
    with pytest.raises(ValueError, match="max_bytes"):
        sparse.to_dense(max_bytes=1000)


def test_a_nonzero_skip_leaves_the_pool_and_counts():
    sparse, dense = _fuse_two_phase("40x21x13", "16x16x8", False)
    before = sparse.pool.clone()
    out6 = torch.from_numpy(_planes()).cuda()
    skip = torch.tensor([1], dtype=torch.int32, device="cuda")
    sparse.integrate(out6, _w2c(R.UPDATE_POSES["tilted"]), R.UPDATE_INTR, skip=skip)
    assert torch.equal(_bits(before), _bits(sparse.pool)) and int(sparse.skipped.item()) == 1


def test_allocating_view_by_view_grows_the_pool_and_keeps_what_it_holds():
    dims, origin = GRIDS["68x9x10"]
    sparse, _ = _volumes(dims, origin, "16x16x8")
    out6 = torch.from_numpy(_planes()).cuda()
    held = None
    for name in S.THREE_POSES:
        pose = _w2c(R.UPDATE_POSES[name])
        sparse.mark(out6, pose, R.UPDATE_INTR)
        before = sparse.slots
        sparse.allocate()
        if held is not None:
            assert torch.equal(_bits(held), _bits(sparse.pool[:, :before]))         # what was there moved with the pool
            assert (sparse.pool[0, before:sparse.slots] == 1).all().item() and (sparse.pool[1:, before:sparse.slots] == 0).all().item()
        sparse.integrate(out6, pose, R.UPDATE_INTR)
        held = sparse.pool[:, :sparse.slots].clone()
    assert sparse.slots == int((sparse.flags != 0).sum().item()) > 2 and sparse.extract().faces.shape[0] > 0


# ---------------------------------------------------------------------------------------------------------------- 7. S3 and S4
def _assert_same_mesh(a, b, least):
    assert a.faces.shape[0] >= least
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)


@pytest.mark.parametrize("limits", (False, True), ids=("plain", "limits-odd-offset"))
@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_extract_of_the_fused_volumes_is_the_dense_mesh(grid, shape, limits):
    sparse, dense = _fused(grid, shape, limits)
    _assert_same_mesh(sparse.extract(), dense.extract(), 20)
    assert sparse.last_triangle_count == dense.last_triangle_count and torch.equal(sparse.last_keys, dense.last_keys)


def _raw_triangles(sparse, capacity, guard=64):
    from splatam_amd import _capi
    flat = torch.full((3 * capacity + guard,), GUARD, dtype=torch.int64, device="cuda")
    count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    _capi.check(_capi.lib().splat_tsdf_sparse_triangles(C.byref(sparse.struct), 1.0, flat.data_ptr(), capacity, count.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream), "splat_tsdf_sparse_triangles")
    torch.cuda.synchronize()
    n, host = int(count.item()), flat.cpu().numpy()
    assert (host[3 * capacity:] == GUARD).all(), "a store at or beyond the capacity"
    assert (host[3 * min(n, capacity):3 * capacity] == GUARD).all()
    return host[:3 * min(n, capacity)].reshape(-1, 3), n


@functools.lru_cache(maxsize=None)
def _topology_volumes():
    import test_gpu_mesh as T
    return T._topology_volumes()


@pytest.mark.parametrize("shape", list(S.SHAPES))
@pytest.mark.parametrize("name", ("sphere", "torus", "zeroed", "slab"))
def test_extract_of_uploaded_fields_is_the_dense_mesh(name, shape):
    import test_gpu_mesh as T
    from splatam_amd.mesh import SparseTsdfVolume
    vol, _ = _topology_volumes()[name]
    dense = T._upload(vol)
    lg = S.SHAPES[shape]
    sparse = SparseTsdfVolume(T.TOPO_ORIGIN, T.TOPO_DIMS, T.TOPO_VOXEL, brick=BRICKS[shape])
    needed = S.needed_bricks(vol["tsdf"] < 0, lg)
    sparse.flags.copy_(torch.from_numpy(needed.astype(np.int32)))
    assert sparse.allocate() == int(needed.sum()) < sparse.num_bricks                # (not every brick: the field's far corners are left out)
    at = sparse.point_offsets()
    have = at >= 0
    for n, k in enumerate(R.VOLUME_ARRAYS):
        sparse.pool.view(5, -1)[n][at[have]] = dense.arrays()[k][have]
    want = dense.extract()
    need = dense.last_triangle_count
    _assert_same_mesh(sparse.extract(capacity=need // 2), want, 1000)                # (half the capacity: complete after the rerun)
    assert sparse.last_triangle_count == need
    _assert_same_mesh(sparse.extract(), want, 1000)
    keys, n = _raw_triangles(sparse, need + 100)
    assert n == need and R.canonical_triangles(keys) == R.canonical_triangles(R.triangles(vol["tsdf"], vol["weight"], 1.0))
    part, n_half = _raw_triangles(sparse, need // 2)
    assert n_half == need and len(part) == need // 2 and set(R.canonical_triangles(part)) <= set(R.canonical_triangles(keys))


def test_a_sparse_volume_without_bricks_gives_an_empty_mesh():
    from splatam_amd.mesh import SparseTsdfVolume
    sparse = SparseTsdfVolume((0, 0, 0), (40, 30, 20), 0.1)
    assert sparse.marked_count() == 0 and sparse.allocate() == 0 and sparse.slots == 0
    mesh = sparse.extract()
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and mesh.colors.shape == (0, 3)
    got = sparse.to_dense()
    assert (got.tsdf == 1).all().item() and (got.weight == 0).all().item()


# ---------------------------------------------------------------------------------------------------------------- 8. end to end
def test_extract_mesh_sparse_is_extract_mesh():
    import test_gpu_mesh as T
    from splatam_amd import mesh as M
    from splatam_amd.fused import PARAM_ORDER
    eng, intr = T._engine()
    main = eng._camera
    W, H, E2E = T.W, T.H, T.E2E

    def snapshot():
        s = {f"param {n}": eng.params[n].detach().clone() for n in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        s.update({f"exp_avg {n}": eng.exp_avg[n].clone() for n in PARAM_ORDER})
        s.update({f"exp_avg_sq {n}": eng.exp_avg_sq[n].clone() for n in PARAM_ORDER})
        s.update({f"variables {n}": eng.variables[n].clone() for n in ('max_2D_radius', 'timestep', 'means2D_gradient_accum', 'denom')})
        s.update({f"rendered {i}": t.clone() for i, t in enumerate(eng.rendered())})
        s.update({f"main {n}": main.buf[n].clone() for n in ('status', 'd_cam')})
        return s
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    with torch.no_grad():
        want, dense = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, return_volume=True, **E2E)
    before = snapshot()
    with torch.no_grad():
        mesh, volume = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, return_volume=True, sparse=True, **E2E)
    torch.cuda.synchronize()
    after = snapshot()
    for name, t in before.items():
        assert torch.equal(bits(t), bits(after[name])), name
    assert eng._camera is main and volume.repeated == [] and volume.repeated_marks == []
    assert int(volume.skipped.item()) == 0 and int(volume.mark_skipped.item()) == 0
    assert isinstance(volume, M.SparseTsdfVolume) and volume.origin == dense.origin and volume.dims == dense.dims and volume.trunc == dense.trunc
    _assert_same_mesh(mesh, want, 500)
    print(f"\nend to end: {volume.slots} of {volume.num_bricks} bricks, {volume.bytes()} bytes against {M.volume_bytes(dense.dims)} dense")
    # a view camera whose lists are far too small: its views are turned away on the device in the mark pass, digested and repeated
    small = eng.view_camera(W, H, capacity=1024)
    with torch.no_grad():
        mesh2, volume2 = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, view=small, return_volume=True, sparse=True, **E2E)
    torch.cuda.synchronize()
    assert len(volume2.repeated_marks) >= 1 and int(volume2.mark_skipped.item()) >= 1
    assert int(volume2.skipped.item()) >= len(volume2.repeated)                      # (the integrate pass repeats whatever it turned away)
    _assert_same_mesh(mesh2, want, 500)
    assert volume2.slots == volume.slots
    for name, t in before.items():
        if not name.startswith("main "):
            assert torch.equal(bits(t), bits(snapshot()[name])), name
    # a box the dense volume is refused for: a finer voxel under a max_bytes below the dense need
    fine = dict(E2E, voxel_size=0.02)
    lo, hi = M.default_bounds(eng.params['means3D'][:eng.P], eng.params['logit_opacities'][:eng.P], 5 * 0.02)
    dense_need = M.volume_bytes(M.plan_volume((lo, hi), 0.02)[1])
    max_bytes = dense_need // 2
    with pytest.raises(ValueError, match="max_bytes"):
        M.extract_mesh(eng, [0, 1, 2], (W, H), intr, max_bytes=max_bytes, **fine)
    with torch.no_grad():
        mesh3, volume3 = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, max_bytes=max_bytes, return_volume=True, sparse=True, **fine)
    print(f"refused dense: {dense_need} bytes dense, {volume3.bytes()} sparse ({volume3.slots} of {volume3.num_bricks} bricks), max_bytes {max_bytes}")
    assert mesh3.faces.shape[0] > 500 and volume3.bytes() < max_bytes < dense_need
    with pytest.raises(ValueError) as e:
        M.extract_mesh(eng, [0, 1, 2], (W, H), intr, max_bytes=volume3.bytes() - 1, sparse=True, **fine)
    assert str(volume3.bytes()) in str(e.value) and "max_bytes" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- 9. session, tool
def test_session_extract_mesh_sparse_writes_the_dense_ply(tmp_path):
    import test_gpu_mesh as T
    from splatam_amd.session import SlamSession
    ds, cfg = T._sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(voxel_size=0.05, sil_thres=0.5)
    with SlamSession(cfg, len(ds)) as session:
        for t in range(len(ds)):
            session.add_frame(*ds[t])
        dense = session.extract_mesh(path=str(tmp_path / "dense.ply"), **kw)
        sparse = session.extract_mesh(path=str(tmp_path / "sparse.ply"), sparse=True, **kw)
        torch.cuda.synchronize()
        _assert_same_mesh(sparse, dense, 100)
        session.finish()
    assert open(tmp_path / "dense.ply", "rb").read() == open(tmp_path / "sparse.ply", "rb").read()
    T._assert_ply_is(str(tmp_path / "sparse.ply"), dense)


def test_the_tool_writes_the_dense_ply_with_sparse(tmp_path):
    import test_gpu_mesh as T
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
    path = pipeline.save_params(out, str(tmp_path / "run"))
    root = os.path.dirname(HERE)
    from splatam_amd import mesh as M
    dense, sparse = str(tmp_path / "run" / "dense.ply"), str(tmp_path / "run" / "sparse.ply")
    M.mesh_from_params(path, dense, voxel_size=0.05, sil_thres=0.5, every=1, verbose=False)             # (the dense tool: tests/test_gpu_mesh.py)
    done = subprocess.run([sys.executable, "-m", "splatam_amd.mesh", path, "--out", sparse, "--voxel", "0.05", "--sil-thres", "0.5", "--every", "1", "--sparse"],
                          cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    assert open(dense, "rb").read() == open(sparse, "rb").read()
    assert len(R.read_mesh_ply(sparse)[2]) > 100
    with pytest.raises(SystemExit, match="max_bytes"):                                                  # (the refusal, through the tool's own entry point)
        M.main([path, "--out", sparse, "--voxel", "0.05", "--sparse", "--max-bytes", "1000"])
