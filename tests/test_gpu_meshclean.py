"""The mesh cleaning layer on the device (splatam_amd/csrc/meshclean.hip through splatam_amd/mesh_clean.py) against the numpy restatement
tests/meshclean_ref.py.  In every case the labels are compared EXACTLY -- the smallest vertex index of each component, not merely the
same partition.

1. A strip of 4 099 triangles (more than 16 workgroups of 256 faces) under three vertex numberings, faces shuffled: one component,
   label 0 -- the deepest forest hooking can build, across waves, workgroups and XCDs.
2. The first and the last face of a 70 000-face array share one vertex, everything between is disjoint triangles.
3. A mix of 3 000 loose triangles, 50 tetrahedra and a 40 x 40 grid with permuted ids: counts, vertices, faces, areas, boxes.
4. Edge semantics: a bow-tie, two coincident unwelded cubes, repeated and out-of-range indices, unreferenced vertices, F = 0, V = 0.
5. Thresholds: exactly ``min_vertices`` and one fewer, ``keep_largest`` with a tie, everything removed, colours, order and renumbering.
6. A million-vertex grid, ids permuted, faces shuffled, 1 % of the faces deleted: all XCDs' atomics at once; two runs, the same bytes.
7. A real mesh: the small TSDF scene of tests/test_gpu_mesh.py with a floater fused in free space.
8. Scoring: a reconstruction with a floater, cleaned inside the score, gives the figures of the reconstruction without it, bit for bit,
   with one more host read.  (``score_mesh``'s signature is pinned by tests/test_icp_cpu.py, so the option is ``score_with_views``'s,
   which without views is ``score_mesh``.)"""
import numpy as np
import pytest
import torch

import meshclean_ref as K
import meshscore_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_labels(V, faces):
    from splatam_amd import mesh_clean as MC
    return MC.label_components(V, _t(np.asarray(faces, dtype=np.int32).reshape(-1, 3))).cpu().numpy()


def gpu_mesh(v, f, c=None):
    from splatam_amd.mesh import Mesh
    return Mesh(_t(np.asarray(v, np.float32)), _t(np.asarray(f, np.int32)), None if c is None else _t(np.asarray(c, np.float32)))


def assert_mesh_is(mesh, v, f, c=None):
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert tuple(mesh.vertices.shape) == (len(v), 3) and tuple(mesh.faces.shape) == (len(f), 3)
    assert mesh.vertices.cpu().numpy().tobytes() == np.ascontiguousarray(v, np.float32).tobytes()
    assert mesh.faces.cpu().numpy().tobytes() == np.ascontiguousarray(f, np.int32).tobytes()
    if c is None:
        assert mesh.colors is None
    else:
        assert mesh.colors.cpu().numpy().tobytes() == np.ascontiguousarray(c, np.float32).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 1. the strip
@pytest.mark.parametrize("numbering", ("ascending", "descending", "permuted"))
def test_a_strip_of_4099_triangles_is_one_component(numbering):
    rng = np.random.default_rng(21)
    v, f = K.strip(4099)
    V = len(v)
    perm = {"ascending": np.arange(V), "descending": np.arange(V)[::-1], "permuted": rng.permutation(V)}[numbering]
    _, f = K.renumbered(v, f, perm)
    f = f[rng.permutation(len(f))]
    assert len(f) > 16 * 256
    want = K.labels(V, f)[0]
    got = gpu_labels(V, f)
    assert (want == 0).all() and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- 2. the two ends
def test_the_first_and_the_last_of_70000_faces_share_a_vertex():
    F = 70_000
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    f[-1, 2] = 0
    V = 3 * F - 1
    want = K.labels(V, f)[0]
    got = gpu_labels(V, f)
    assert np.array_equal(got, want)
    assert got[f[-1, 0]] == got[f[-1, 1]] == got[0] == got[1] == got[2] == 0 and len(np.unique(got)) == F - 1


# ---------------------------------------------------------------------------------------------------------------- 3. the mix
def test_a_mix_of_components_labels_and_statistics():
    from splatam_amd import mesh_clean as MC
    v, f = K.mix()
    V = len(v)
    want_lab = K.labels(V, f)[0]
    want = K.stats(v, f, want_lab)
    m = gpu_mesh(v, f)
    labels = MC.label_components(V, m.faces)
    assert np.array_equal(labels.cpu().numpy(), want_lab)
    st = {k: t.cpu().numpy() for k, t in MC.component_stats(m, labels).items()}
    roots = want["is_root"]
    assert np.array_equal(st["is_root"], roots) and roots.sum() == 3051
    assert np.array_equal(st["num_vertices"], want["num_vertices"]) and np.array_equal(st["num_faces"], want["num_faces"])
    assert sorted(set(st["num_vertices"][roots])) == [3, 4, 1600] and sorted(set(st["num_faces"][roots])) == [1, 4, 2 * 39 * 39]
    assert np.array_equal(st["area_quanta"], want["area_quanta"]) and st["area"].dtype == np.float64 and np.array_equal(st["area"], want["area"])
    assert np.array_equal(st["lo"][roots], want["lo"][roots]) and np.array_equal(st["hi"][roots], want["hi"][roots])
    assert np.isnan(st["lo"][~roots]).all() and np.isnan(st["hi"][~roots]).all()
    grid_root = int(np.flatnonzero(st["num_vertices"] == 1600)[0])
    assert abs(st["area"][grid_root] - 39 * 39 * 1e-4) < 1e-6
    again = MC.component_stats(m)                                        # labels computed inside
    assert all(np.array_equal(again[k].cpu().numpy(), st[k], equal_nan=k in ("lo", "hi")) for k in st)


# ---------------------------------------------------------------------------------------------------------------- 4. edge semantics
def test_edge_semantics():
    from splatam_amd import mesh_clean as MC
    bow = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    assert gpu_labels(5, bow).tolist() == [0, 0, 0, 0, 0]
    v, f = K.join([K.cube(), K.cube()])                                 # coincident, not welded
    assert gpu_labels(16, f).tolist() == [0] * 8 + [8] * 8
    deg = np.array([[5, 5, 5], [1, 1, 2], [3, 4, 10], [-1, 0, 1], [4, 3, 3], [7, 2, 2], [2 ** 31 - 1, 0, 1], [-2 ** 31, 2, 3]], dtype=np.int32)
    got = gpu_labels(10, deg)                                           # (vertices 8 and 9: no face names them)
    assert got.tolist() == [0, 1, 1, 3, 3, 5, 6, 1, 8, 9] and np.array_equal(got, K.labels(10, deg)[0])
    vd = np.random.default_rng(2).normal(size=(10, 3)).astype(np.float32)
    st = {k: t.cpu().numpy() for k, t in MC.component_stats(gpu_mesh(vd, deg)).items()}
    want = K.stats(vd, deg)
    assert np.array_equal(st["num_faces"], want["num_faces"]) and st["num_faces"].tolist() == [0, 2, 0, 1, 0, 1, 0, 0, 0, 0]
    assert np.array_equal(st["num_vertices"], want["num_vertices"]) and np.array_equal(st["area_quanta"], want["area_quanta"])
    assert st["area_quanta"][3] == 0 and st["area_quanta"][5] == 0       # a repeated index: a face of zero area
    # out-of-range faces are dropped by the filter, unreferenced vertices too
    cleaned, report = MC.clean_mesh(gpu_mesh(vd, deg), min_vertices=0, report=True)
    rv, rf, _, rrep = K.clean(vd, deg, min_vertices=0)
    assert_mesh_is(cleaned, rv, rf)
    assert report == rrep and report["faces_removed"] == 4 and report["components"] == 3 and len(rv) == 6
    # F = 0 and V = 0
    none = np.zeros((0, 3), dtype=np.int32)
    assert gpu_labels(6, none).tolist() == [0, 1, 2, 3, 4, 5] and gpu_labels(0, none).shape == (0,)
    st0 = MC.component_stats(gpu_mesh(vd[:6], none))
    assert st0["num_vertices"].tolist() == [1] * 6 and st0["num_faces"].tolist() == [0] * 6 and bool(st0["is_root"].all())
    assert np.array_equal(st0["lo"].cpu().numpy(), vd[:6]) and np.array_equal(st0["hi"].cpu().numpy(), vd[:6])
    for mesh in (gpu_mesh(vd[:6], none), gpu_mesh(vd[:0], none), gpu_mesh(vd[:0], bow)):
        out, rep = MC.clean_mesh(mesh, report=True)
        assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.colors is None and rep["components"] == 0
    with pytest.raises(ValueError, match="not finite"):
        bad = vd.copy()
        bad[4, 1] = np.inf
        MC.clean_mesh(gpu_mesh(bad, deg), min_vertices=0)


# ---------------------------------------------------------------------------------------------------------------- 5. thresholds
def threshold_mesh():
    rng = np.random.default_rng(8)
    parts = [K.strip(198), K.strip(197), K.cube((5, 0, 0)), K.cube((8, 0, 0)), K.grid(20, 20, origin=(0, 3, 0))]
    parts[1] = (parts[1][0] + np.float32(10.0), parts[1][1])
    v, f = K.join(parts)
    v, f = K.renumbered(v, f, rng.permutation(len(v)))
    return v, f[rng.permutation(len(f))], rng.random((len(v), 3)).astype(np.float32)


THRESHOLDS = {"defaults": (dict(), 200 + 400), "one-fewer": (dict(min_vertices=199), 200 + 199 + 400),
              "largest-4-tie": (dict(min_vertices=0, keep_largest=4), 200 + 199 + 400 + 8), "largest-1": (dict(min_vertices=0, keep_largest=1), 400),
              "area": (dict(min_vertices=0, min_area=5.9), 16), "extent-faces": (dict(min_vertices=0, min_extent=0.5, min_faces=13), 200 + 199),
              "largest-100": (dict(min_vertices=0, keep_largest=100), 815), "nothing-left": (dict(min_vertices=10 ** 6), 0)}


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_thresholds_order_renumbering_and_colours(name):
    from splatam_amd import mesh_clean as MC
    options, vertices_left = THRESHOLDS[name]
    v, f, c = threshold_mesh()
    rv, rf, rc, rrep = K.clean(v, f, c, **options)
    out, rep = MC.clean_mesh(gpu_mesh(v, f, c), report=True, **options)
    assert_mesh_is(out, rv, rf, rc)
    assert rep == rrep and rep["components"] == 5
    assert len(rv) == vertices_left
    if name == "defaults":                                              # exactly min_vertices survives, one fewer does not
        assert rep["components_kept"] == 2 and rep["faces_removed"] == 197 + 12 + 12
    if name == "largest-4-tie":                                         # the two cubes tie at 12 faces: the lower label stays
        lab = K.labels(len(v), f)[0]
        cubes = sorted(int(r) for r in np.unique(lab) if (lab == r).sum() == 8)
        kept_cube = v[lab == cubes[0]]
        assert len(cubes) == 2 and all((rv == p).all(axis=1).any() for p in kept_cube)
        assert not any((rv == p).all(axis=1).any() for p in v[lab == cubes[1]])
    if name == "nothing-left":
        assert out.colors.shape == (0, 3) and rep["area_removed_m2"] == rep["area_m2"] > 0
    assert MC.clean_mesh(gpu_mesh(v, f, c), **options).faces.shape == out.faces.shape          # (report=False: the Mesh alone)


# ---------------------------------------------------------------------------------------------------------------- 6. a million vertices
def test_a_million_vertex_grid_twice():
    from splatam_amd import mesh_clean as MC
    rng = np.random.default_rng(13)
    v, f = K.grid(1000, 1000, spacing=0.001)
    v, f = K.renumbered(v, f, rng.permutation(len(v)))
    f = f[rng.permutation(len(f))]
    f = np.ascontiguousarray(f[rng.random(len(f)) >= 0.01])
    V = len(v)
    want = K.labels_any(V, f)
    m = gpu_mesh(v, f)
    runs = []
    for _ in range(2):
        labels = MC.label_components(V, m.faces)
        st = MC.component_stats(m, labels)
        out = MC.clean_mesh(m)
        torch.cuda.synchronize()
        runs.append([labels.cpu().numpy().tobytes()] + [st[k].cpu().numpy().tobytes() for k in sorted(st)]
                    + [out.vertices.cpu().numpy().tobytes(), out.faces.cpu().numpy().tobytes()])
    got = np.frombuffer(runs[0][0], dtype=np.int32)
    assert np.array_equal(got, want)
    assert runs[0] == runs[1]
    big = int(np.bincount(want).argmax())
    nv = np.frombuffer(runs[0][1 + sorted(st).index("num_vertices")], dtype=np.int32)
    q = np.frombuffer(runs[0][1 + sorted(st).index("area_quanta")], dtype=np.int64)
    assert nv[big] == (want == big).sum() > 990_000 and nv.sum() == V
    assert q.sum() == K.area_quanta(v, f).sum()                         # exact in the quanta, whatever the order


# ---------------------------------------------------------------------------------------------------------------- 7. a real mesh
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


def test_a_real_mesh_with_a_floater():
    from splatam_amd import mesh as M
    from splatam_amd import mesh_clean as MC
    eng, intr = _engine()
    with torch.no_grad():
        plain, volume = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, return_volume=True, **E2E)
        plain2 = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, clean=None, **E2E)
        options = dict(min_vertices=15)
        cleaned = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, clean=options, **E2E)
        default = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, clean=True, **E2E)
    assert plain.faces.shape[0] > 500
    for a, b in zip(plain, plain2):                                     # without the option: what it was
        assert torch.equal(a, b)
    pv, pf, pc = (t.cpu().numpy() for t in plain)
    for got, opts in ((cleaned, options), (default, {})):               # extract_mesh(clean=...) is clean_mesh(extract_mesh()), is the restatement
        direct = MC.clean_mesh(plain, **opts)
        for a, b in zip(got, direct):
            assert torch.equal(a, b)
        assert_mesh_is(got, *K.clean(pv, pf, pc, **opts)[:3])
    # a floater: one grid point turned negative in the middle of 3 x 3 x 3 seen points of free space -- a closed shell of 14 vertices
    # on the 14 edges Kuhn's split gives a grid point, which shares no vertex with any other surface
    tsdf, weight = volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy()
    free = (weight >= 1) & (tsdf > 0)
    block = np.ones_like(free[1:-1, 1:-1, 1:-1])
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                block &= free[dz:dz + free.shape[0] - 2, dy:dy + free.shape[1] - 2, dx:dx + free.shape[2] - 2]
    spots = np.argwhere(block)
    assert len(spots) > 0, "the scene has no 3 x 3 x 3 block of seen free space"
    z, y, x = (int(t) + 1 for t in spots[len(spots) // 2])
    volume.tsdf[z, y, x] = -0.5
    with_floater = volume.extract(1.0)
    n_float = with_floater.vertices.shape[0] - plain.vertices.shape[0]
    assert n_float == 14 and with_floater.faces.shape[0] > plain.faces.shape[0]
    wv, wf, wc = (t.cpu().numpy() for t in with_floater)
    lab = K.labels(len(wv), wf)[0]
    centre = np.array(volume.origin) + 0.05 * np.array([x, y, z])
    shell = np.abs(wv - centre).max(axis=1) < 0.05
    assert shell.sum() == 14 and len(np.unique(lab[shell])) == 1 and (lab == lab[shell][0]).sum() == 14
    got = MC.clean_mesh(with_floater, **options)
    assert_mesh_is(got, *K.clean(wv, wf, wc, **options)[:3])
    for a, b in zip(got, cleaned):                                      # the floater went and nothing else: the cleaned mesh of before, byte for byte
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 8. scoring
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


def test_scoring_a_cleaned_reconstruction():
    from splatam_amd import mesh_score as S
    gv, gf = R.sphere_mesh(3, 0.5)
    sv, sf = R.sphere_mesh(3, 0.51, centre=(0.004, -0.003, 0.002))
    assert len(sv) >= 200
    fv, ff = K.join([(sv, sf), K.tetrahedron((0.9, 0.9, 0.9), 0.05), K.tetrahedron((-1.2, 0.3, 0.1), 0.03)])
    gt, rec, rec_floaters = gpu_mesh(gv, gf), gpu_mesh(sv, sf), gpu_mesh(fv, ff)
    with _Reads() as base:
        want = S.score_mesh(rec, gt, samples=20_000, seed=4)
    with _Reads() as cleaned:
        got = S.score_with_views(rec_floaters, gt, samples=20_000, seed=4, clean=True)
    dirty = S.score_mesh(rec_floaters, gt, samples=20_000, seed=4)
    assert "cleaning" not in want and "cleaning" not in dirty and set(want) == set(S.KEYS)
    assert "cleaning" not in S.score_with_views(rec, gt, samples=20_000, seed=4, clean=None)
    for k in S.KEYS:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), k
    assert dirty["accuracy_cm"] > want["accuracy_cm"] and dirty["max_rec_to_gt"] > 0.5          # the floaters were charged to accuracy
    assert set(got) == set(S.KEYS) | {"cleaning"}
    rep = got["cleaning"]
    assert rep["components"] == 3 and rep["components_kept"] == 1 and rep["faces_removed"] == 8 and rep["faces"] == len(ff)
    assert rep == K.clean(fv, ff)[3]
    assert cleaned.n == base.n + 1, (cleaned.n, base.n)                   # once more than before, and only once
    assert S.format_score(got).startswith("Cleaning: kept 1 of 3 components, removed 8 of ")
    # ... and in front of the ICP: the order is transform, clean, cull, ICP, samples
    both = S.score_with_views(rec_floaters, gt, samples=20_000, seed=4, clean=dict(min_vertices=200), align=True)
    only = S.score_mesh(rec, gt, samples=20_000, seed=4, align=True)
    assert both["cleaning"] == rep and np.array_equal(both["alignment"]["transformation"], only["alignment"]["transformation"])
    for k in S.KEYS:
        assert np.float64(both[k]).tobytes() == np.float64(only[k]).tobytes(), k
    with pytest.raises(ValueError, match="removed every component"):
        S.score_with_views(rec_floaters, gt, samples=100, clean=dict(min_vertices=10 ** 6))
