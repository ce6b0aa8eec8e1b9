"""The mesh layer on the device (csrc/tsdf.hip through ``splatam_amd.mesh``, ``SlamSession.extract_mesh`` and
``python -m splatam_amd.mesh``), held to the float64 restatement tests/tsdf_ref.py by the rules of tests/test_tsdf_math_cpu.py:

  5. T1 on the update check's volume, planes and poses: the same decisions as float64 off the grid points within rounding of a
     threshold (at most 2 %), values within 4 x the float32 numpy form's own largest error.  nx = 37 (scalar path), nx = 40 (16-byte
     path), nx = 68 (two bricks along x, the second partly outside the grid); out6 as a view into a larger buffer at an odd offset; a
     non-zero ``skip`` leaves the volume bit-unchanged and counts 1.
  6. T2 / T3 on the uploaded sphere, torus, zeroed-corner sphere and slab volumes of the topology check: the triangle key set equals
     the restatement's exactly; vertices within 4 x the float32 form's own error; half the capacity: the count reports the need, a
     guard behind ``keys`` is intact, ``extract`` returns the full mesh after its rerun; two extractions return identical tensors.
  7. End to end on ``slam.synthetic_params(4000, 160, 112, ...)`` at time indices 0..2: the volume equals the restatement run on the
     downloaded planes, the faces equal the restatement's, the map / Adam moments / variables / current camera are bit-equal before
     and after, a view camera with too small a capacity is repeated and gives the same mesh.
  8. ``SlamSession.extract_mesh`` after three frames and ``python -m splatam_amd.mesh`` on a saved ``params.npz`` write a PLY that the
     test's parser reads and that matches ``extract_mesh``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tsdf_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOPO_DIMS, TOPO_VOXEL, TOPO_ORIGIN = (29, 25, 27), 0.05, (-0.7, -0.6, -0.65)
SPHERE_C, SPHERE_R = (0.013, 0.021, -0.017), 0.45
GUARD = -7


def _download(volume):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in volume.arrays().items()}


def _upload(vol, origin=TOPO_ORIGIN, voxel=TOPO_VOXEL):
    from splatam_amd.mesh import TsdfVolume
    nz, ny, nx = vol["tsdf"].shape
    volume = TsdfVolume(origin, (nx, ny, nz), voxel)
    for k, t in volume.arrays().items():
        t.copy_(torch.from_numpy(np.ascontiguousarray(vol[k], np.float32)))
    return volume


# ---------------------------------------------------------------------------------------------------------------- 5. T1
@pytest.fixture(scope="module")
def planes():
    return R.plane_view(*R.UPDATE_SIZE, R.UPDATE_INTR)


def _update_volume(dims):
    from splatam_amd.mesh import TsdfVolume
    return TsdfVolume(R.UPDATE_ORIGIN, dims, R.UPDATE_VOXEL, R.UPDATE_TRUNC)


def _w2c(pose):
    return torch.from_numpy(np.ascontiguousarray(pose, np.float32)).cuda()


@pytest.mark.parametrize("dims", ((37, 21, 13), (40, 21, 13), (68, 9, 10)), ids=("nx37-scalar", "nx40-vector", "nx68-two-bricks"))
def test_integrate_against_the_restatement(planes, dims):
    out6 = torch.from_numpy(planes).cuda()
    fresh = R.new_volume(dims)
    for pose in R.UPDATE_POSES:
        volume = _update_volume(dims)
        volume.integrate(out6, _w2c(R.UPDATE_POSES[pose]), R.UPDATE_INTR)
        got = _download(volume)
        R.check_update(got, dims, [R.UPDATE_POSES[pose]], planes, f"{dims} {pose}")
        if pose == "behind":
            assert all(got[k].tobytes() == fresh[k].tobytes() for k in R.VOLUME_ARRAYS)
        else:
            assert (got["weight"] > 0).mean() > 0.03
    poses = [R.UPDATE_POSES[k] for k in ("identity", "tilted", "oblique")]
    volume = _update_volume(dims)
    for pose in poses:
        volume.integrate(out6, _w2c(pose), R.UPDATE_INTR)
    R.check_update(_download(volume), dims, poses, planes, f"{dims} three views")
    assert int(volume.skipped.item()) == 0


def test_integrate_limits_and_planes_inside_a_larger_buffer(planes):
    """depth_max / weight_max, with out6 a view at an odd float offset into a larger buffer (no 16-byte alignment of the planes)."""
    W, H = R.UPDATE_SIZE
    big = torch.full((3 + 6 * H * W + 64,), float("nan"), dtype=torch.float32, device="cuda")
    out6 = big[3:3 + 6 * H * W].view(6, H, W)
    out6.copy_(torch.from_numpy(planes))
    assert out6.data_ptr() % 16 != 0
    poses = [R.UPDATE_POSES["identity"], R.UPDATE_POSES["tilted"], R.UPDATE_POSES["identity"]]
    kw = dict(depth_max=1.3, weight_max=2.0)
    for dims in ((37, 21, 13), (40, 21, 13)):
        volume = _update_volume(dims)
        for pose in poses:
            volume.integrate(out6, _w2c(pose), R.UPDATE_INTR, **kw)
        got = _download(volume)
        R.check_update(got, dims, poses, planes, f"{dims} limits", **kw)
        assert got["weight"].max() == 2


@pytest.mark.parametrize("dims", ((37, 21, 13), (40, 21, 13)))
def test_a_nonzero_skip_leaves_the_volume_and_counts(planes, dims):
    out6 = torch.from_numpy(planes).cuda()
    volume = _update_volume(dims)
    volume.integrate(out6, _w2c(R.UPDATE_POSES["identity"]), R.UPDATE_INTR)
    before = _download(volume)
    skip = torch.tensor([2], dtype=torch.int32, device="cuda")
    volume.integrate(out6, _w2c(R.UPDATE_POSES["tilted"]), R.UPDATE_INTR, skip=skip)
    after = _download(volume)
    assert all(before[k].tobytes() == after[k].tobytes() for k in R.VOLUME_ARRAYS) and int(volume.skipped.item()) == 1
    skip.zero_()
    volume.integrate(out6, _w2c(R.UPDATE_POSES["tilted"]), R.UPDATE_INTR, skip=skip)
    R.check_update(_download(volume), dims, [R.UPDATE_POSES["identity"], R.UPDATE_POSES["tilted"]], planes, f"{dims} after a skipped view")
    assert int(volume.skipped.item()) == 1


# ---------------------------------------------------------------------------------------------------------------- 6. T2 and T3
def _topology_volumes():
    sphere = R.sphere_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, SPHERE_R)
    zeroed = sphere.astype(np.float32)
    zeroed[np.abs(zeroed) < 0.004] = 0.0
    slab = R.field_volume(sphere)
    slab["weight"][:, :, 14] = 0.0
    return {"sphere": (R.field_volume(sphere), 2), "torus": (R.field_volume(R.torus_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, 0.4, 0.15)), 0),
            "zeroed": (R.field_volume(zeroed), 2), "slab": (slab, None)}


@pytest.fixture(scope="module")
def topology_volumes():
    return _topology_volumes()


def _raw_triangles(volume, capacity, guard=64):
    """splat_tsdf_triangles into a guarded buffer: (keys [min(n, capacity), 3] on the host, n)."""
    from splatam_amd import _capi
    flat = torch.full((3 * capacity + guard,), GUARD, dtype=torch.int64, device="cuda")
    count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    _capi.check(_capi.lib().splat_tsdf_triangles(C.byref(volume.struct), 1.0, flat.data_ptr(), capacity, count.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "splat_tsdf_triangles")
    torch.cuda.synchronize()
    n, host = int(count.item()), flat.cpu().numpy()
    assert (host[3 * capacity:] == GUARD).all(), "a store at or beyond the capacity"
    assert (host[3 * min(n, capacity):3 * capacity] == GUARD).all()
    return host[:3 * min(n, capacity)].reshape(-1, 3), n


@pytest.mark.parametrize("name", ("sphere", "torus", "zeroed", "slab"))
def test_triangles_and_vertices_of_uploaded_volumes(topology_volumes, name):
    vol, euler = topology_volumes[name]
    volume = _upload(vol)
    want = R.canonical_triangles(R.triangles(vol["tsdf"], vol["weight"], 1.0))
    need = len(want)
    keys, n = _raw_triangles(volume, need + 100)
    assert n == need > 1000 and R.canonical_triangles(keys) == want          # the key set, exactly: the decisions read stored floats only
    # half the capacity: the count reports the need, nothing lands behind the capacity, what landed are triangles of the mesh
    part, n_half = _raw_triangles(volume, need // 2)
    assert n_half == need and len(part) == need // 2 and set(R.canonical_triangles(part)) <= set(want)
    # extract(): canonical, complete after its rerun, the same tensors twice
    mesh = volume.extract(capacity=need // 2)
    again = volume.extract()
    torch.cuda.synchronize()
    assert volume.last_triangle_count == need
    for a, b in zip(mesh, again):
        assert a.dtype == b.dtype and torch.equal(a, b)
    faces, uniq = mesh.faces.cpu().numpy(), volume.last_keys.cpu().numpy()
    assert mesh.faces.dtype == torch.int32 and mesh.vertices.dtype == torch.float32 and faces.shape == (need, 3)
    assert (np.diff(uniq) > 0).all() and faces.min() == 0 and faces.max() == len(uniq) - 1
    assert R.canonical_triangles(uniq[faces]) == want
    order = np.lexsort((faces[:, 2], faces[:, 1], faces[:, 0]))
    assert np.array_equal(order, np.arange(need)) or np.array_equal(faces[order], faces)          # rows in lexicographic order
    # vertices and colours against float64, within 4 x the float32 numpy form's own error
    pos, col = mesh.vertices.cpu().numpy(), mesh.colors.cpu().numpy()
    p64, c64 = R.vertices(uniq, vol, TOPO_ORIGIN, TOPO_VOXEL, np.float64)
    p32, c32 = R.vertices(uniq, vol, TOPO_ORIGIN, TOPO_VOXEL, np.float32)
    print(f"\n{name}: {len(uniq)} vertices, {need} faces; position error {np.abs(pos - p64).max():.3e} (own {np.abs(p32 - p64).max():.3e}), "
          f"colour error {np.abs(col - c64).max():.3e} (own {np.abs(c32 - c64).max():.3e})")
    assert np.abs(pos - p64).max() <= 4 * np.abs(p32 - p64).max() and np.abs(col - c64).max() <= 4 * np.abs(c32 - c64).max()
    V, E, F, closed = R.topology(faces)
    if euler is not None:
        assert closed and V - E + F == euler and R.signed_volume(pos, faces) > 0
    else:
        assert not closed and all(R.decode_key(TOPO_DIMS, int(k))[0][0] != 14 and R.decode_key(TOPO_DIMS, int(k))[1][0] != 14 for k in uniq)


def test_a_volume_nothing_was_fused_into_gives_an_empty_mesh():
    from splatam_amd.mesh import TsdfVolume
    volume = TsdfVolume((0, 0, 0), (9, 5, 3), 0.1)
    got = _download(volume)
    assert (got["tsdf"] == 1).all() and all((got[k] == 0).all() for k in ("weight", "r", "g", "b"))
    mesh = volume.extract()
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and mesh.colors.shape == (0, 3)
    assert TsdfVolume((0, 0, 0), (1, 1, 1), 0.1).extract().faces.shape == (0, 3)                  # no cell at all


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
W, H, F_PX = 160, 112, 150.0
E2E = dict(voxel_size=0.05, sil_thres=0.5, depth_max=6.0)


def _engine():
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    params, variables = slam.synthetic_params(4000, W, H, F_PX, F_PX, cx, cy, num_frames=3, seed=0, device="cuda")
    with torch.no_grad():
        params['cam_trans'][0, :, 1] = torch.tensor([0.06, -0.02, 0.03], device="cuda")
        params['cam_trans'][0, :, 2] = torch.tensor([-0.05, 0.03, 0.08], device="cuda")
        params['cam_unnorm_rots'][0, :, 1] = torch.tensor([0.999, 0.01, 0.03, -0.01], device="cuda")
        params['cam_unnorm_rots'][0, :, 2] = torch.tensor([0.998, -0.02, -0.04, 0.02], device="cuda")
    w2c = torch.eye(4, device="cuda")
    k = [[F_PX, 0, cx], [0, F_PX, cy], [0, 0, 1]]
    cam = slam.setup_camera(W, H, k, w2c.cpu().numpy(), device="cuda")
    im, depth = slam.synthetic_frame(params, cam, w2c, 1, rot_deg=0.4, trans_m=0.01)
    frame = {'cam': cam, 'im': im, 'depth': depth, 'id': 1, 'w2c': w2c}
    with torch.no_grad():
        eng = FusedEngine(params, cam, gaussian_capacity=8192, variables=variables)
        for _ in range(2):
            eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
        assert not eng.check_overflow()
        eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
    torch.cuda.synchronize()
    return eng, (F_PX, F_PX, cx, cy)


def test_extract_mesh_end_to_end_against_the_restatement():
    from splatam_amd import mesh as M
    from splatam_amd.fused import PARAM_ORDER
    eng, intr = _engine()
    main = eng._camera

    def snapshot():
        s = {f"param {n}": eng.params[n].detach().clone() for n in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        s.update({f"exp_avg {n}": eng.exp_avg[n].clone() for n in PARAM_ORDER})
        s.update({f"exp_avg_sq {n}": eng.exp_avg_sq[n].clone() for n in PARAM_ORDER})
        s.update({f"variables {n}": eng.variables[n].clone() for n in ('max_2D_radius', 'timestep', 'means2D_gradient_accum', 'denom')})
        s.update({f"rendered {i}": t.clone() for i, t in enumerate(eng.rendered())})
        s.update({f"main {n}": main.buf[n].clone() for n in ('status', 'd_cam')})
        return s
    before = snapshot()
    assert float(before["exp_avg means3D"].abs().max()) > 0
    with torch.no_grad():
        mesh, volume = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, return_volume=True, **E2E)
    torch.cuda.synchronize()
    after = snapshot()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    for name, t in before.items():
        assert torch.equal(bits(t), bits(after[name])), name
    assert eng._camera is main and volume.repeated == [] and int(volume.skipped.item()) == 0
    # default bounds: the opaque Gaussians' box padded by trunc + voxel
    lo, hi = M.default_bounds(eng.params['means3D'][:eng.P], eng.params['logit_opacities'][:eng.P], 5 * 0.05)
    assert volume.origin == lo and volume.dims == M.plan_volume((lo, hi), 0.05)[1] and volume.trunc == pytest.approx(0.2)
    # the restatement on the planes and poses of the same views, downloaded
    view = eng.view_camera(W, H)
    planes, poses = [], []
    with torch.no_grad():
        for t in range(3):
            img = eng.render_view(view, time_idx=t, intrinsics=intr, rgb8=False)
            assert int(img.truncated.item()) == 0
            planes.append(img.out6.cpu().numpy().copy())
            poses.append(view.w2c.cpu().numpy().astype(np.float64))
    grid = dict(origin=volume.origin, voxel=0.05, trunc=volume.trunc, intr=intr)
    got = _download(volume)
    fig = R.check_update(got, volume.dims, poses, planes, "end to end", grid=grid, sil_thres=0.5, depth_max=6.0)
    assert fig["updated"] > 0.05 and got["weight"].max() == 3
    faces, uniq = mesh.faces.cpu().numpy(), volume.last_keys.cpu().numpy()
    want = R.canonical_triangles(R.triangles(got["tsdf"], got["weight"], 1.0))
    assert len(want) > 500 and R.canonical_triangles(uniq[faces]) == want
    pos, col = mesh.vertices.cpu().numpy(), mesh.colors.cpu().numpy()
    p64, c64 = R.vertices(uniq, got, volume.origin, 0.05, np.float64)
    p32, c32 = R.vertices(uniq, got, volume.origin, 0.05, np.float32)
    assert np.abs(pos - p64).max() <= 4 * np.abs(p32 - p64).max() and np.abs(col - c64).max() <= 4 * np.abs(c32 - c64).max()
    assert col.min() >= 0 and col.max() <= 1
    # a view camera whose lists are far too small: its views are turned away on the device, digested and repeated -- the same mesh
    small = eng.view_camera(W, H, capacity=1024)
    with torch.no_grad():
        mesh2, volume2 = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, view=small, return_volume=True, **E2E)
    torch.cuda.synchronize()
    assert len(volume2.repeated) >= 1 and int(volume2.skipped.item()) >= 1
    for a, b in zip(mesh, mesh2):
        assert torch.equal(a, b)
    for name, t in before.items():
        if not name.startswith("main "):                    # (the digest of a flagged view is allowed the engine's accumulator, nothing of the map)
            assert torch.equal(bits(t), bits(snapshot()[name])), name
    # a volume beyond max_bytes is refused before anything is allocated
    with pytest.raises(ValueError, match="max_bytes"):
        M.extract_mesh(eng, [0], (W, H), intr, voxel_size=0.05, max_bytes=1 << 16)


# ---------------------------------------------------------------------------------------------------------------- 8. session, tool
def _sequence(num_frames=3, w=72, h=40):
    from splatam_amd import pipeline
    f = 0.9 * w
    ds = pipeline.SyntheticRGBDSequence(1500, w, h, f, f, w / 2 - 0.5, h / 2 - 0.5, num_frames=num_frames, seed=2, step_m=0.012, step_deg=0.4).preload()
    cfg = pipeline.replica_config(tracking_iters=4, mapping_iters=6, keyframe_every=2)
    return ds, cfg


def _assert_ply_is(path, mesh):
    pos, col, faces = R.read_mesh_ply(path)
    assert pos.tobytes() == mesh.vertices.cpu().numpy().tobytes() and np.array_equal(faces, mesh.faces.cpu().numpy())
    assert np.array_equal(col, np.rint(np.clip(mesh.colors.cpu().numpy(), 0, 1) * 255.0).astype(np.uint8))
    assert len(faces) > 100


def test_session_extract_mesh_writes_the_mesh(tmp_path):
    from splatam_amd import mesh as M
    from splatam_amd.session import SlamSession
    ds, cfg = _sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(voxel_size=0.05, sil_thres=0.5)
    with SlamSession(cfg, len(ds)) as session:
        for t in range(len(ds)):
            session.add_frame(*ds[t])
        before = {n: session.params[n].detach().clone() for n in session.params}
        path = str(tmp_path / "mesh.ply")
        mesh = session.extract_mesh(path=path, **kw)
        torch.cuda.synchronize()
        for n, p in before.items():
            assert torch.equal(p, session.params[n].detach()), n
        _assert_ply_is(path, mesh)
        k = session.intrinsics.detach().cpu().double().numpy()
        frames = list(session.keyframe_time_indices) or list(range(session.frames_seen))
        with torch.no_grad():
            direct = M.extract_mesh(session.engine, frames, (72, 40), (k[0][0], k[1][1], k[0][2], k[1][2]),
                                    first_w2c=session.first_frame_w2c.contiguous(), **kw)
        for a, b in zip(mesh, direct):
            assert torch.equal(a, b)
        session.finish()
    with SlamSession(cfg, len(ds), engine="dropin") as other:
        with pytest.raises(NotImplementedError, match="fused"):
            other.extract_mesh()


def test_the_tool_writes_the_mesh_of_a_saved_map(tmp_path):
    from splatam_amd import mesh as M
    from splatam_amd import pipeline
    ds, cfg = _sequence()
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
    ply = str(tmp_path / "run" / "mesh.ply")
    root = os.path.dirname(HERE)
    done = subprocess.run([sys.executable, "-m", "splatam_amd.mesh", path, "--out", ply, "--voxel", "0.05", "--sil-thres", "0.5", "--every", "1"],
                          cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    mesh = M.mesh_from_params(path, str(tmp_path / "again.ply"), voxel_size=0.05, sil_thres=0.5, every=1, verbose=False)
    _assert_ply_is(ply, mesh)
    assert open(ply, "rb").read() == open(tmp_path / "again.ply", "rb").read()
    refused = subprocess.run([sys.executable, "-m", "splatam_amd.mesh", path, "--out", ply, "--voxel", "0.05", "--max-bytes", "1000"],
                             cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert refused.returncode != 0 and "max_bytes" in refused.stdout
