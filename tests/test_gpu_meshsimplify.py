"""The mesh simplification layer on the device (splatam_amd/csrc/meshsimplify.hip through splatam_amd/mesh_simplify.py).  Kernel =
header, bit for bit, in every case: vertices, faces and colours of ``simplify_mesh`` equal the result of the HOST BUILD of
csrc/meshsimplify_math.h (tests/meshsimplify_math_shim.cpp, driven by tests/meshsimplify_ref.py) byte for byte.

1. A 64 x 64-per-side cube (49 152 faces, more than 16 workgroups of 256) at about 20 faces per cluster, vertices permuted and faces
   shuffled: the bytes are the host's, and those of the unpermuted run.
2. Contention: 70 000 faces with all vertices inside ONE cell plus one far triangle across three cells -- every atomic of S1 and S2
   lands on the same 17 words.  The sums equal the restatement's integers; the output is exactly the far triangle.
3. Two cells sharing a face plane, vertices on the boundary x = j cell: ids and output are the host's.
4. The edge semantics of tests/test_meshsimplify_cpu.py item 6 on the device, with colours and without.
5. A million-face grid, ids permuted, faces shuffled, 1 % of the faces deleted: two runs, the same bytes; the invariants hold.
6. A fused mesh (a small run, as in tests/test_gpu_mesh.py) at cell = 3 voxels, for both extraction methods: fewer vertices and
   faces, the invariants, ``clean`` then ``simplify`` through ``mesh_from_params`` and ``SlamSession.extract_mesh(simplify=...)`` equal
   ``simplify_mesh(clean_mesh(extract))`` byte for byte, without the option the PLY's bytes are what they were, the report's counts.
7. ONE host read in ``simplify_mesh``."""
import numpy as np
import pytest
import torch

import meshclean_ref as K
import meshsimplify_ref as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def shim():
    return Q.load_shim()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_mesh(v, f, c=None):
    from splatam_amd.mesh import Mesh
    return Mesh(_t(np.asarray(v, np.float32)), _t(np.asarray(f, np.int32)), None if c is None else _t(np.asarray(c, np.float32)))


def host(mesh):
    return tuple(None if t is None else t.cpu().numpy() for t in mesh)


def assert_mesh_is(mesh, v, f, c=None):
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert tuple(mesh.vertices.shape) == (len(v), 3) and tuple(mesh.faces.shape) == (len(f), 3)
    assert mesh.vertices.cpu().numpy().tobytes() == np.ascontiguousarray(v, np.float32).tobytes()
    assert mesh.faces.cpu().numpy().tobytes() == np.ascontiguousarray(f, np.int32).tobytes()
    if c is None:
        assert mesh.colors is None
    else:
        assert mesh.colors.cpu().numpy().tobytes() == np.ascontiguousarray(c, np.float32).tobytes()


def assert_device_is_host(shim, v, f, c, cell, **options):
    """simplify_mesh on the device against the header on the host: mesh and report; returns (the device's Mesh, the report)."""
    from splatam_amd import mesh_simplify as MS
    want = Q.simplify(v, f, c, cell, shim=shim, **options)
    got, report = MS.simplify_mesh(gpu_mesh(v, f, c), cell, report=True, **options)
    assert_mesh_is(got, *want[:3])
    for k, x in want[3].items():
        if k == "rms_plane_distance_m":                                 # (a sum of doubles in another order)
            assert abs(report[k] - x) <= 1e-6 * max(x, report[k]) + 1e-9, (report[k], x)
        else:
            assert report[k] == x, (k, report[k], x)
    return got, report


# ---------------------------------------------------------------------------------------------------------------- 1. the cube
@pytest.mark.parametrize("placement", ("quadric", "mean"))
def test_a_64_per_side_cube_permuted_and_shuffled(shim, placement):
    rng = np.random.default_rng(31)
    v, f = Q.welded_cube(64, (0.013,) * 3)
    c = rng.random((len(v), 3)).astype(np.float32)
    assert len(f) == 49152 > 16 * 256
    cell = 0.05
    plain, report = assert_device_is_host(shim, v, f, c, cell, placement=placement)
    assert 15 < len(f) / report["cells"] < 25
    pv, pf, pc = Q.renumbered(v, f, rng.permutation(len(v)), c)
    pf = pf[rng.permutation(len(pf))]
    for dedupe in (True, False):
        mixed, _ = assert_device_is_host(shim, pv, pf, pc, cell, placement=placement, dedupe=dedupe)
        assert mixed.vertices.cpu().numpy().tobytes() == plain.vertices.cpu().numpy().tobytes()
        assert mixed.colors.cpu().numpy().tobytes() == plain.colors.cpu().numpy().tobytes()
        Q.check_invariants(pv, pf, pc, cell, host(mixed), dedupe, closed=True)
        if dedupe:
            assert np.array_equal(np.unique(mixed.faces.cpu().numpy(), axis=0), np.unique(plain.faces.cpu().numpy(), axis=0))
    if placement == "quadric":
        assert report["fallbacks"] == 0 and report["rank3"] == 8 and report["rms_plane_distance_m"] < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 2. contention
def test_70000_faces_in_one_cell(shim):
    from splatam_amd import mesh_simplify as MS
    rng = np.random.default_rng(32)
    F, cell = 70_000, 0.5
    inside = (1.0 + rng.uniform(0.02, 0.48, size=(3 * F, 3))).astype(np.float32)          # all in the cell (2, 2, 2)
    far = np.array([[5.1, 5.2, 5.3], [5.7, 5.2, 5.3], [5.1, 5.8, 5.9]], dtype=np.float32)
    v = np.concatenate((inside[:F], far, inside[F:]))
    tri = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    tri = np.where(tri >= F, tri + 3, tri)
    f = np.concatenate((tri[:F // 2], np.array([[F, F + 1, F + 2]], dtype=np.int32), tri[F // 2:]))
    c = rng.random((len(v), 3)).astype(np.float32)
    keys = Q.keys(v, cell)
    cluster = Q.cluster_ids(keys)
    assert len(np.unique(keys)) == 4 and (cluster == 0).sum() == 3 * F
    count, acc, refused, ds = Q.sums(v, f, c, cell, cluster)
    m = gpu_mesh(v, f, c)
    got = MS.cluster_sums(m, cell)
    assert np.array_equal(got["keys"].cpu().numpy(), keys) and np.array_equal(got["cluster"].cpu().numpy(), cluster)
    assert np.array_equal(got["count"].cpu().numpy(), count) and count[0] == 3 * F
    assert np.array_equal(got["sums"].cpu().numpy(), acc) and int(got["refused"][0]) == 0
    assert np.array_equal(got["cell_keys"].cpu().numpy(), Q.cluster_keys(keys, cluster))
    assert np.array_equal(Q.shim_sums(shim, v, f, c, cell, cluster)[1], acc)
    out, report = assert_device_is_host(shim, v, f, c, cell)
    assert out.faces.cpu().numpy().tolist() == [[0, 1, 2]] and report["faces_kept"] == 1 and report["cells"] == 4
    assert np.abs(out.vertices.cpu().numpy() - far).max() < 1e-6 and np.abs(out.colors.cpu().numpy() - c[F:F + 3]).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 3. the boundary
def test_vertices_on_the_boundary_between_two_cells(shim):
    from splatam_amd import mesh_simplify as MS
    cell = 0.25
    g, f = K.grid(9, 13, spacing=0.125)                                 # y, z = j / 8: every other one ON a boundary
    wall = np.stack((np.full(len(g), 0.75), g[:, 0] - 0.5, g[:, 1] - 0.75), axis=1).astype(np.float32)      # the plane x = 3 cell, both signs of y and z
    floor_v, floor_f = K.grid(7, 9, spacing=0.125)
    floor_v = (floor_v + np.array([0.25, -0.5, -0.75])).astype(np.float32)                  # the plane z = -3 cell, x from 1 cell to 4 cell
    v, f = K.join([(wall, f), (floor_v, floor_f)])
    keys = MS.cell_keys(_t(v), cell)
    want = Q.shim_keys(shim, v, cell)
    assert np.array_equal(keys.cpu().numpy(), want) and np.array_equal(want, Q.keys(v, cell))
    ix = ((want & 0x1fffff) - (1 << 20))
    assert (ix[:len(wall)] == 3).all()                                  # x = 3 cell belongs to cell 3, not to cell 2
    assert np.array_equal(MS.cluster_ids(keys).cpu().numpy(), Q.cluster_ids(want))
    for dedupe in (True, False):
        out, _ = assert_device_is_host(shim, v, f, None, cell, dedupe=dedupe)
        Q.check_invariants(v, f, None, cell, host(out), dedupe)


# ---------------------------------------------------------------------------------------------------------------- 4. edge semantics
def edge_mesh():
    v = np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [np.nan, 0.1, 0.1], [2.1, 0.1, 0.1], [3.1, 0.1, 0.1], [4.1, 0.1, 0.1],
                  [9.0, 9.0, 9.0], [1.2, 1.2, 0.3]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 0, 1], [0, 1, 9], [-1, 0, 1], [0, 3, 1], [4, 5, 6], [1, 8, 2], [2 ** 31 - 1, 0, 1], [-2 ** 31, 1, 2]], dtype=np.int32)
    c = np.linspace(0, 1, 27, dtype=np.float32).reshape(9, 3)
    return v, f, c


@pytest.mark.parametrize("colours", (True, False))
@pytest.mark.parametrize("placement", ("quadric", "mean"))
def test_edge_semantics(shim, placement, colours):
    from splatam_amd import mesh_simplify as MS
    v, f, c = edge_mesh()
    c = c if colours else None
    out, report = assert_device_is_host(shim, v, f, c, 1.0, placement=placement)
    assert report["faces_kept"] == 3 and report["vertices_kept"] == 7 and report["cells"] == 8
    assert np.array_equal(out.vertices.cpu().numpy()[out.faces.cpu().numpy()[1]], v[[4, 5, 6]])          # the zero-area face survives
    none = np.zeros((0, 3), dtype=np.int32)
    for mesh in (gpu_mesh(v, none, c), gpu_mesh(v[:0], none, None if c is None else c[:0]), gpu_mesh(v[:0], f, None)):
        got, rep = MS.simplify_mesh(mesh, 1.0, placement=placement, report=True)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and rep["faces_kept"] == 0 and rep["cells"] == 0
    got, rep = MS.simplify_mesh(gpu_mesh(v[:3], f[:1], None if c is None else c[:3]), 10.0, placement=placement, report=True)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and rep["cells"] == 1          # everything in one cell: the empty mesh
    assert (got.colors is None) == (c is None)
    with pytest.raises(ValueError, match="2\\^20 cells"):
        MS.simplify_mesh(gpu_mesh(v, f, c), 1e-6, placement=placement)
    if placement == "quadric":
        big = np.array([[-3e19, -3e19, 0], [3e19, -3e19, 0], [0, 3e19, 0]], dtype=np.float32)
        with pytest.raises(ValueError, match="area"):
            MS.simplify_mesh(gpu_mesh(big, np.array([[0, 1, 2]], dtype=np.int32)), 1e14)
    # host arrays and a transform go through to_device_mesh
    shift = np.eye(4)
    shift[:3, 3] = (0.25, 0.5, -0.125)
    moved = MS.simplify_mesh((v, f, c), 1.0, placement=placement, transform=shift)
    want = Q.simplify((v.astype(np.float64) + shift[:3, 3]).astype(np.float32), f, c, 1.0, placement, shim=shim)
    assert_mesh_is(moved, *want[:3])


# ---------------------------------------------------------------------------------------------------------------- 5. a million faces
def test_a_million_face_grid_twice(shim):
    from splatam_amd import mesh_simplify as MS
    rng = np.random.default_rng(33)
    v, f = K.grid(710, 710, spacing=0.001, origin=(-0.3, -0.35, 0.0))
    v[:, 2] = (0.004 * np.sin(40.0 * v[:, 0]) * np.cos(31.0 * v[:, 1])).astype(np.float32)
    v, f = K.renumbered(v, f, rng.permutation(len(v)))
    f = f[rng.permutation(len(f))]
    f = np.ascontiguousarray(f[rng.random(len(f)) >= 0.01])
    assert len(f) > 990_000
    cell = 0.004
    m = gpu_mesh(v, f)
    runs = []
    for _ in range(2):
        acc = MS.cluster_sums(m, cell)
        out, report = MS.simplify_mesh(m, cell, report=True)
        torch.cuda.synchronize()
        runs.append([acc["count"].cpu().numpy().tobytes(), acc["sums"].cpu().numpy().tobytes(), out.vertices.cpu().numpy().tobytes(),
                     out.faces.cpu().numpy().tobytes(), repr(report)])
    assert runs[0] == runs[1]
    want = Q.simplify(v, f, None, cell, shim=shim, details=True)
    assert runs[0][1] == want[4]["sums"].tobytes() and runs[0][0] == want[4]["count"].tobytes()
    assert_mesh_is(out, *want[:3])
    assert report["faces_kept"] < len(f) / 10 and report["vertices_kept"] < len(v) / 10
    Q.check_invariants(v, f, None, cell, host(out), True)
    print(report)


# ---------------------------------------------------------------------------------------------------------------- 6. a fused mesh
VOXEL = 0.05
KW = dict(voxel_size=VOXEL, sil_thres=0.5)
CLEAN = dict(min_vertices=15)


@pytest.fixture(scope="module")
def finished_run(tmp_path_factory):
    """Three frames of the synthetic sequence through a session; the session stays open for the tests, its map is also saved."""
    from splatam_amd import pipeline
    from splatam_amd.session import SlamSession
    w, h = 72, 40
    fx = 0.9 * w
    ds = pipeline.SyntheticRGBDSequence(1500, w, h, fx, fx, w / 2 - 0.5, h / 2 - 0.5, num_frames=3, seed=2, step_m=0.012, step_deg=0.4).preload()
    cfg = pipeline.replica_config(tracking_iters=4, mapping_iters=6, keyframe_every=2)
    torch.manual_seed(0)
    np.random.seed(0)
    session = SlamSession(cfg, len(ds))
    session.__enter__()
    for t in range(len(ds)):
        session.add_frame(*ds[t])
    out = {n: p for n, p in session.params.items()}
    out['timestep'] = session.variables['timestep']
    out['intrinsics'] = ds[0][2][:3, :3].cpu().numpy()
    out['w2c'] = torch.linalg.inv(ds[0][3]).cpu().numpy()
    out['org_width'], out['org_height'] = w, h
    out['keyframe_time_indices'] = np.array(list(session.keyframe_time_indices))
    path = pipeline.save_params(out, str(tmp_path_factory.mktemp("run")))
    yield session, path
    session.finish()
    session.__exit__(None, None, None)


@pytest.mark.parametrize("method", ("tetrahedra", "cubes"))
def test_a_fused_mesh_through_every_door(shim, finished_run, tmp_path, method):
    from splatam_amd import mesh as M
    from splatam_amd import mesh_clean as MC
    from splatam_amd import mesh_simplify as MS
    session, path = finished_run
    cell = 3 * VOXEL
    plain = session.extract_mesh(method=method, **KW)
    assert plain.faces.shape[0] > 100
    v, f, c = host(plain)
    # the module against the header, the invariants, the report
    out, report = assert_device_is_host(shim, v, f, c, cell)
    assert 0 < out.vertices.shape[0] < len(v) and 0 < out.faces.shape[0] < len(f)
    assert report["vertices"] == len(v) and report["faces"] == len(f)
    assert report["vertices_kept"] == out.vertices.shape[0] and report["faces_kept"] == out.faces.shape[0]
    assert report["cells"] >= report["vertices_kept"] and report["rank1"] + report["rank2"] + report["rank3"] + report["fallbacks"] == report["cells"]
    assert 0 < report["rms_plane_distance_m"] < cell
    for dedupe in (True, False):
        got = MS.simplify_mesh(plain, cell, dedupe=dedupe)
        Q.check_invariants(v, f, c, cell, host(got), dedupe)
    # clean, then simplify: the session's door
    want = MS.simplify_mesh(MC.clean_mesh(plain, **CLEAN), cell)
    through = session.extract_mesh(method=method, clean=CLEAN, simplify=cell, **KW)
    for a, b in zip(through, want):
        assert torch.equal(a, b)
    as_dict = session.extract_mesh(method=method, clean=CLEAN, simplify=dict(cell=cell, placement="mean"), **KW)
    for a, b in zip(as_dict, MS.simplify_mesh(MC.clean_mesh(plain, **CLEAN), cell, placement="mean")):
        assert torch.equal(a, b)
    again = session.extract_mesh(method=method, simplify=None, **KW)     # without the option: what it was
    for a, b in zip(again, plain):
        assert torch.equal(a, b)
    # ... and mesh_from_params': without the option the PLY's bytes are what they are without the parameter
    found, cleaning = {}, {}
    bare = M.mesh_from_params(path, str(tmp_path / "bare.ply"), every=1, verbose=False, method=method, **KW)
    off = M.mesh_from_params(path, str(tmp_path / "off.ply"), every=1, verbose=False, method=method, simplify=None, simplification=found, **KW)
    assert open(tmp_path / "bare.ply", "rb").read() == open(tmp_path / "off.ply", "rb").read() and found == {}
    for a, b in zip(bare, off):
        assert torch.equal(a, b)
    made = M.mesh_from_params(path, str(tmp_path / "small.ply"), every=1, verbose=False, method=method, clean=CLEAN, cleaning=cleaning,
                              simplify=cell, simplification=found, **KW)
    direct, direct_report = MS.simplify_mesh(MC.clean_mesh(bare, **CLEAN), cell, report=True)
    for a, b in zip(made, direct):
        assert torch.equal(a, b)
    assert {k: x for k, x in found.items() if k != "rms_plane_distance_m"} == {k: x for k, x in direct_report.items() if k != "rms_plane_distance_m"}
    assert abs(found["rms_plane_distance_m"] - direct_report["rms_plane_distance_m"]) <= 1e-9 and cleaning["faces"] == bare.faces.shape[0]
    assert found["vertices_kept"] == made.vertices.shape[0] and found["faces_kept"] == made.faces.shape[0] < bare.faces.shape[0]
    from splatam_amd.export import load_mesh_ply
    loaded = load_mesh_ply(str(tmp_path / "small.ply"))
    assert np.asarray(loaded[0]).tobytes() == made.vertices.cpu().numpy().tobytes() and np.array_equal(np.asarray(loaded[1]), made.faces.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- 7. one host read
class _Reads:
    """Counts the host reads of device tensors made through .cpu(), .item() and .tolist() -- how every read of the mesh modules is made."""

    def __enter__(self):
        self.n, self.saved = 0, {k: getattr(torch.Tensor, k) for k in ("cpu", "item", "tolist")}
        for k, fn in self.saved.items():
            def counted(t, *a, _fn=fn, **kw):
                if t.is_cuda:
                    self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, counted)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)


def test_one_host_read():
    from splatam_amd import mesh_simplify as MS
    v, f = Q.welded_cube(24, (0.013,) * 3)
    c = np.random.default_rng(1).random((len(v), 3)).astype(np.float32)
    m = gpu_mesh(v, f, c)
    for options in (dict(), dict(placement="mean"), dict(dedupe=False), dict(report=True)):
        with _Reads() as reads:
            MS.simplify_mesh(m, 0.1, **options)
        assert reads.n == 1, (options, reads.n)
    with _Reads() as reads:
        keys = MS.cell_keys(m.vertices, 0.1)
        MS.cluster_sums(m, 0.1, MS.cluster_ids(keys))
    assert reads.n == 0
