"""The mesh score layer on the device (csrc/meshscore.hip through ``splatam_amd.mesh_score``), held to the header on the host
(tests/meshscore_math_shim.cpp), to the numpy restatement tests/meshscore_ref.py and to closed-form geometry:

  1. M0 / M1: areas equal the header's; samples equal the header's bit for bit at n = 5 000 (not a multiple of 64) and n = 1, given
     the device's own prefix sum.
  2. M2 - M4: dist2 and index bit-equal to the float32 brute force, in the queries' original order, on every case of
     ``meshscore_ref.nn_cases``; the same without sorting the queries.
  3. M5 on the first case: count and n equal numpy's on the kernel's own dist2, max equal, sum within n 2^-53 relative, two launches
     the same bits.
  4. ``score_mesh`` on a sphere mesh of radius r = 0.45 (k = 5) against one of radius r + 0.02, 20 000 samples: every sample distance
     at least delta - e_gt; completion ratio 100 at threshold 0.05 and 0 at 0.01; a hemisphere's completion count equal to the float64 brute
     force on the same samples and inside the closed-form band; ``transform`` against the untransformed score.
     Every sample distance, and both means, also stay below delta + e_rec: the meshes are sampled with the same seed.
  5. Hands off: ``score_mesh`` of a mesh extracted from a live ``FusedEngine`` leaves the map, the Adam moments, ``variables`` and the
     current camera bit-unchanged; a mesh against itself scores 0 cm and 100 %.
  6. ``python -m splatam_amd.mesh_score`` on two small PLYs prints what ``score_mesh`` returns."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshscore_ref as R
from test_meshscore_cpu import load_shim, shim_areas, shim_sample

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -24
CASES = R.nn_cases()
RADIUS, DELTA, SAMPLES = 0.45, 0.02, 20_000


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


# ---------------------------------------------------------------------------------------------------------------- 1. M0, M1
@pytest.mark.parametrize("which", ("box", "sphere"))
def test_areas_and_samples_equal_the_header(which):
    from splatam_amd import mesh_score as S
    shim = load_shim()
    v, f = R.box_mesh() if which == "box" else R.sphere_mesh(3, 0.45, (0.2, -0.1, 0.3))
    dv, df = _dev(v), _dev(f)
    area, prefix = S.surface_prefix(dv, df)
    assert area.cpu().numpy().tobytes() == shim_areas(shim, v, f).tobytes()
    pre = prefix.cpu().numpy()
    assert np.allclose(pre, np.cumsum(R.areas(v, f)), rtol=1e-13, atol=0)
    for n, seed in ((5000, 0), (5000, 0xFEDCBA9876543210), (1, 7)):
        pts, face = S.sample_surface(dv, df, n, seed)
        want_pts, want_face = shim_sample(shim, v, f, pre, seed, n)
        assert face.cpu().numpy().tobytes() == want_face.tobytes() and pts.cpu().numpy().tobytes() == want_pts.tobytes()
        assert face.min() >= 0 and (which != "box" or int((face == 12).sum()) == 0)
    # sample i does not depend on n (nor on the launch's shape)
    few = S.sample_surface(dv, df, 77, 0)[0]
    assert torch.equal(few, S.sample_surface(dv, df, 5000, 0)[0][:77])


# ---------------------------------------------------------------------------------------------------------------- 2. M2 - M4
@pytest.fixture(scope="module")
def brute():
    return {name: R.brute32(q, t) for name, (t, q, _) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_nearest_equals_the_float32_brute_force(brute, name):
    from splatam_amd import mesh_score as S
    targets, queries, cell = CASES[name]
    grid = S.NearestGrid(_dev(targets), cell=cell)
    assert (grid.lo, grid.cell, grid.dims) == S.plan_grid(targets.min(axis=0), targets.max(axis=0), len(targets), cell)
    assert grid.cells <= 2 ** 21
    q = _dev(queries)
    d2, idx, acc = grid.query(q, account=True)
    ref_d2, ref_idx = brute[name]
    acc = acc.cpu().numpy()
    print(f"{name}: grid {grid.dims} of cell {grid.cell:.6g}; candidates per query mean {acc[:, 0].mean():.1f} max {acc[:, 0].max()}, "
          f"shells mean {acc[:, 1].mean():.2f} max {acc[:, 1].max()}")
    assert d2.cpu().numpy().tobytes() == ref_d2.tobytes() and idx.cpu().numpy().tobytes() == ref_idx.tobytes()
    d2u, idxu = grid.query(q, sort=False)
    assert torch.equal(d2u.view(torch.int32), d2.view(torch.int32)) and torch.equal(idxu, idx)
    start = grid.start.cpu().numpy()
    assert start[0] == 0 and start[-1] == len(targets) and (np.diff(start) >= 0).all()
    if name == "cell-cap":
        assert grid.cells > 2 ** 20
    if name == "one-cell":
        assert grid.dims == (1, 1, 1)
    if name == "coplanar":
        assert grid.dims[2] == 1


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C
    from splatam_amd import _capi
    L = _capi.lib()
    g = _capi.SplatNnGrid()
    g.lo[:], g.cell, g.dims[:], g.count = (0.0, 0.0, 0.0), 1.0, (1, 1, 1), 0
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    assert L.splat_nn_cell_keys(C.byref(g), p, 4, p + 128, None) == 0
    for field, value in (("cell", 0.0), ("cell", float("nan")), ("cell", float("inf")), ("count", -1)):
        bad = _capi.SplatNnGrid()
        C.memmove(C.byref(bad), C.byref(g), C.sizeof(g))
        setattr(bad, field, value)
        assert L.splat_nn_cell_keys(C.byref(bad), p, 4, p, None) != 0, (field, value)
    bad = _capi.SplatNnGrid()
    C.memmove(C.byref(bad), C.byref(g), C.sizeof(g))
    bad.dims[:] = (2048, 2048, 1)                                        # 2^22 cells
    assert L.splat_nn_cell_keys(C.byref(bad), p, 4, p, None) != 0
    bad.dims[:] = (0, 1, 1)
    assert L.splat_nn_cell_keys(C.byref(bad), p, 4, p, None) != 0
    bad.dims[:] = (1, 1, 1)
    bad.lo[0] = float("nan")
    assert L.splat_nn_cell_keys(C.byref(bad), p, 4, p, None) != 0
    assert L.splat_nn_cell_keys(C.byref(g), None, 4, p, None) != 0 and L.splat_nn_cell_keys(C.byref(g), p, -1, p, None) != 0
    assert L.splat_nn_query(C.byref(g), p, None, 4, p, p, None, None) != 0          # no start table bound
    assert L.splat_nn_cell_starts(C.byref(g), None, None, None, None, None, None) != 0
    assert L.splat_nn_reduce(p, 4, 0.05, None, p, None) != 0 and L.splat_nn_reduce(None, 4, 0.05, p, p, None) != 0
    assert L.splat_mesh_areas(p, 3, None, 1, p, None) != 0 and L.splat_mesh_areas(p, -1, p, 1, p, None) != 0
    assert L.splat_mesh_sample(p, 3, p, 1, None, 0, 4, p, p, None) != 0 and L.splat_mesh_sample(p, 3, p, 1, p, 0, 4, None, p, None) != 0
    torch.cuda.synchronize()
    assert not buf.any()                                                 # (the one accepted call wrote keys 0)


# ---------------------------------------------------------------------------------------------------------------- 3. M5
def test_reduce_against_numpy_and_bit_reproducible():
    from splatam_amd import mesh_score as S
    targets, queries, cell = CASES["uniform-box"]
    d2, _ = S.NearestGrid(_dev(targets), cell=cell).query(_dev(queries))
    d = np.sqrt(d2.cpu().numpy().astype(np.float64))
    threshold = float(np.median(d))
    rows = torch.zeros(2, 4, dtype=torch.float64, device="cuda")
    S.reduce_distances(d2, threshold, rows[0])
    S.reduce_distances(d2, threshold, rows[1])
    got = rows.cpu().numpy()
    n = len(d)
    assert got[0].tobytes() == got[1].tobytes()
    assert got[0, 1] == float((d < threshold).sum()) and 0 < got[0, 1] < n and got[0, 3] == n
    assert got[0, 2] == d.max()
    exact = float(np.sum(d.astype(np.longdouble)))
    assert abs(got[0, 0] - exact) <= n * 2.0 ** -53 * exact
    big = torch.rand(300_001, device="cuda")                             # more than 256 workgroups' worth: the grid-stride path
    S.reduce_distances(big, 0.25, rows[0])
    S.reduce_distances(big, 0.25, rows[1])
    got, db = rows.cpu().numpy(), np.sqrt(big.cpu().numpy().astype(np.float64))
    assert got[0].tobytes() == got[1].tobytes() and got[0, 1] == float((db < 0.25).sum()) and got[0, 2] == db.max() and got[0, 3] == len(db)
    assert abs(got[0, 0] - db.sum()) <= len(db) * 2.0 ** -53 * db.sum()


# ---------------------------------------------------------------------------------------------------------------- 4. closed form
@pytest.fixture(scope="module")
def spheres():
    """rec (radius r), gt (radius r + delta), each mesh's e = L^2 / (8 r_min), and the per-sample distances of both directions (the
    layer's own samples and search), computed once."""
    from splatam_amd import mesh_score as S
    rec, gt = R.sphere_mesh(5, RADIUS), R.sphere_mesh(5, RADIUS + DELTA)
    e_rec, e_gt = R.longest_edge(*rec) ** 2 / (8 * RADIUS), R.longest_edge(*gt) ** 2 / (8 * RADIUS)
    pr = S.sample_surface(_dev(rec[0]), _dev(rec[1]), SAMPLES, 0)[0]
    pg = S.sample_surface(_dev(gt[0]), _dev(gt[1]), SAMPLES, 0)[0]
    d_rg = torch.sqrt(S.NearestGrid(pg).query(pr)[0].double()).cpu().numpy()
    d_gr = torch.sqrt(S.NearestGrid(pr).query(pg)[0].double()).cpu().numpy()
    score = S.score_mesh(rec, gt, samples=SAMPLES, threshold=0.05)
    return dict(rec=rec, gt=gt, e_rec=e_rec, e_gt=e_gt, d_rg=d_rg, d_gr=d_gr, score=score, pr=pr, pg=pg)


def test_sphere_score_is_the_mean_of_the_sample_distances_and_bounded_below(spheres):
    from splatam_amd import mesh_score as S
    s, score = spheres, spheres["score"]
    print(f"e_rec {s['e_rec']:.3e} e_gt {s['e_gt']:.3e}; rec -> gt distances {s['d_rg'].min():.6f} .. {s['d_rg'].max():.6f} mean {s['d_rg'].mean():.6f}; "
          f"gt -> rec {s['d_gr'].min():.6f} .. {s['d_gr'].max():.6f} mean {s['d_gr'].mean():.6f}; score {score}")
    assert tuple(score) == S.KEYS and score["samples"] == SAMPLES
    assert abs(score["accuracy_cm"] / 100 - s["d_rg"].mean()) <= 1e-12 and abs(score["completion_cm"] / 100 - s["d_gr"].mean()) <= 1e-12
    assert score["max_rec_to_gt"] == s["d_rg"].max() and score["max_gt_to_rec"] == s["d_gr"].max()
    lower = DELTA - s["e_gt"]
    assert s["d_rg"].min() >= lower and s["d_gr"].min() >= lower
    assert score["accuracy_cm"] / 100 >= lower and score["completion_cm"] / 100 >= lower
    assert score["completion_ratio"] == 100.0 and score["precision"] == 1.0 and score["recall"] == 1.0 and score["fscore"] == 1.0
    tight = S.score_mesh(s["rec"], s["gt"], samples=SAMPLES, threshold=0.01)
    assert tight["completion_ratio"] == 0.0 and tight["fscore"] == 0.0 and tight["accuracy_cm"] == score["accuracy_cm"]


def test_sphere_distances_stay_below_delta_plus_e_rec(spheres):
    """Every sample distance, and therefore accuracy_cm / 100 and completion_cm / 100, lies in [delta - e_gt, delta + e_rec].  The upper
    half holds for distances between SAMPLES because both surfaces are sampled with the same seed: the two meshes are one subdivision
    at two radii, so sample i of the ground truth is sample i of the reconstruction pushed outward, at most delta away.  (The
    restatement's float64 brute force on its own bit-equal samples: 0.019981 .. 0.0199999, mean 0.019990, both ways.)"""
    s = spheres
    upper = DELTA + s["e_rec"]
    print(f"upper bound {upper:.6f}: rec -> gt mean {s['d_rg'].mean():.6f} max {s['d_rg'].max():.6f}, gt -> rec mean {s['d_gr'].mean():.6f} "
          f"max {s['d_gr'].max():.6f}")
    assert s["d_rg"].max() <= upper and s["d_gr"].max() <= upper
    assert s["score"]["accuracy_cm"] / 100 <= upper and s["score"]["completion_cm"] / 100 <= upper


def _brute64_device(queries, targets, chunk=500):
    """float64 distances to the nearest target by comparing every pair (explicit differences, on the device for speed)."""
    q, t = queries.double(), targets.double()
    out = torch.empty(len(q), dtype=torch.float64, device=q.device)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - t[None, :, :]
        out[s:s + chunk] = (d * d).sum(dim=2).min(dim=1).values.sqrt()
    return out.cpu().numpy()


def test_hemisphere_completion_count_equals_float64_brute_force(spheres):
    from splatam_amd import mesh_score as S
    tau, R_gt = 0.03, RADIUS + DELTA
    v, f = spheres["rec"]
    upper = f[v[f].astype(np.float64).mean(axis=1)[:, 2] > 0]
    assert len(upper) == len(f) // 2
    score = S.score_mesh((v, upper, None), spheres["gt"], samples=SAMPLES, threshold=tau)
    count = round(score["completion_ratio"] / 100 * SAMPLES)
    assert abs(count - score["recall"] * SAMPLES) < 1e-6
    ph = S.sample_surface(_dev(v), _dev(upper), SAMPLES, 0)[0]
    d64 = _brute64_device(spheres["pg"], ph)
    want, edge = int((d64 < tau).sum()), int((np.abs(d64 - tau) <= 1e-6).sum())
    sigma = 100 * np.sqrt(0.25 / SAMPLES)
    print(f"hemisphere: completion ratio {score['completion_ratio']:.3f} % (count {count}, float64 brute force {want}, {edge} samples within "
          f"1e-6 of the threshold); band {50 - 5 * sigma:.3f} .. {50 + 100 * tau / (2 * R_gt) + 5 * sigma:.3f}")
    assert edge <= SAMPLES // 1000 and abs(count - want) <= edge
    assert 50 - 5 * sigma <= score["completion_ratio"] <= 50 + 100 * tau / (2 * R_gt) + 5 * sigma


def test_transform_undoes_a_rigid_motion_of_the_reconstruction(spheres):
    from splatam_amd import mesh_score as S
    from tests.util import rigid_w2c
    v, f = spheres["rec"]
    M = rigid_w2c(0.7, (1.0, -2.0, 0.5), (0.3, -0.2, 0.5)).astype(np.float64)
    moved = (v.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    inv = np.linalg.inv(M)
    base = spheres["score"]
    bound = 8 * EPS * float(max(np.abs(moved).max(), np.abs(spheres["gt"][0]).max()))
    for rec in ((moved, f, None), (_dev(moved), _dev(f), None)):          # host arrays and device tensors
        got = S.score_mesh(rec, spheres["gt"], samples=SAMPLES, threshold=0.05, transform=inv)
        print({k: (got[k], base[k]) for k in ("accuracy_cm", "completion_cm", "max_rec_to_gt", "max_gt_to_rec")}, f"bound {bound:.3e} m")
        for k, scale in (("accuracy_cm", 100.0), ("completion_cm", 100.0), ("max_rec_to_gt", 1.0), ("max_gt_to_rec", 1.0)):
            assert abs(got[k] - base[k]) <= scale * bound, k
        assert got["completion_ratio"] == base["completion_ratio"] and got["fscore"] == base["fscore"]
    far = S.score_mesh((moved, f, None), spheres["gt"], samples=SAMPLES, threshold=0.05)          # (without it the motion shows)
    assert far["accuracy_cm"] > 10 * base["accuracy_cm"]
    with pytest.raises(ValueError, match="4 x 4"):
        S.score_mesh((moved, f, None), spheres["gt"], samples=100, transform=np.eye(3))


# ---------------------------------------------------------------------------------------------------------------- 5. hands off
W, H, F_PX = 160, 112, 150.0


def _engine():
    """A live engine on a 4 000-Gaussian scene at 160 x 112, three mapping iterations in (as tests/test_gpu_mesh.py builds one)."""
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


def test_score_mesh_leaves_a_live_engine_untouched():
    from splatam_amd import mesh as M
    from splatam_amd import mesh_score as S
    from splatam_amd.fused import PARAM_ORDER
    eng, intr = _engine()
    main = eng._camera
    with torch.no_grad():
        mesh = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, voxel_size=0.05, sil_thres=0.5, depth_max=6.0)
    torch.cuda.synchronize()
    assert mesh.faces.shape[0] > 500

    def snapshot():
        s = {f"param {n}": eng.params[n].detach().clone() for n in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        s.update({f"exp_avg {n}": eng.exp_avg[n].clone() for n in PARAM_ORDER})
        s.update({f"exp_avg_sq {n}": eng.exp_avg_sq[n].clone() for n in PARAM_ORDER})
        s.update({f"variables {n}": eng.variables[n].clone() for n in ('max_2D_radius', 'timestep', 'means2D_gradient_accum', 'denom')})
        s.update({f"rendered {i}": t.clone() for i, t in enumerate(eng.rendered())})
        s.update({f"main {n}": main.buf[n].clone() for n in ('status', 'd_cam')})
        s.update({f"mesh {n}": getattr(mesh, n).clone() for n in ("vertices", "faces", "colors")})
        return s
    before = snapshot()
    assert float(before["exp_avg means3D"].abs().max()) > 0
    shifted = M.Mesh(mesh.vertices + torch.tensor([0.01, 0.0, 0.0], device="cuda"), mesh.faces, mesh.colors)
    same = S.score_mesh(mesh, mesh, samples=SAMPLES)
    other = S.score_mesh(shifted, mesh, samples=SAMPLES)
    torch.cuda.synchronize()
    after = snapshot()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    for name, t in before.items():
        assert torch.equal(bits(t), bits(after[name])), name
    assert eng._camera is main
    assert same["accuracy_cm"] == 0.0 and same["completion_cm"] == 0.0 and same["completion_ratio"] == 100.0 and same["fscore"] == 1.0
    assert same["max_rec_to_gt"] == 0.0 and same["max_gt_to_rec"] == 0.0
    assert 0.0 < other["accuracy_cm"] <= 1.0 + 1e-4 and 0.0 < other["completion_cm"] <= 1.0 + 1e-4          # (a 1 cm shift: at most 1 cm away)


# ---------------------------------------------------------------------------------------------------------------- 6. command line
def test_the_command_prints_what_score_mesh_returns(tmp_path):
    from splatam_amd import mesh_score as S
    from splatam_amd.export import save_mesh_ply
    rec, gt = R.sphere_mesh(3, 0.45), R.sphere_mesh(3, 0.47, (0.3, -0.2, 0.5))
    M = np.eye(4)
    M[:3, 3] = (0.3, -0.2, 0.5)
    save_mesh_ply(str(tmp_path / "rec.ply"), *rec)
    save_mesh_ply(str(tmp_path / "gt.ply"), *gt)
    np.savetxt(str(tmp_path / "pose.txt"), M.reshape(1, 16))
    root = os.path.dirname(HERE)
    args = ["--samples", "5000", "--threshold", "0.01985", "--seed", "3", "--transform", str(tmp_path / "pose.txt")]
    done = subprocess.run([sys.executable, "-m", "splatam_amd.mesh_score", str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply")] + args, cwd=root,
                          env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    score = S.score_mesh(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), samples=5000, threshold=0.01985, seed=3, transform=M)
    assert done.stdout.strip() == S.format_score(score).strip(), done.stdout
    assert 0 < score["completion_ratio"] < 100 and score["accuracy_cm"] > 1.9
    lines = done.stdout.splitlines()
    assert lines[0].startswith("Accuracy: ") and lines[1].startswith("Completion: ") and lines[2].startswith("Completion ratio: ")
    assert lines[3].startswith("F-score: ")
    refused = subprocess.run([sys.executable, "-m", "splatam_amd.mesh_score", str(tmp_path / "rec.ply"), str(tmp_path / "missing.ply")], cwd=root,
                             env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert refused.returncode != 0 and "missing.ply" in refused.stdout and "Traceback" not in refused.stdout
