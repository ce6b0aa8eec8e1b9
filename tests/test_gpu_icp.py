"""The ICP layer on the device (csrc/icp.hip through ``splatam_amd.mesh_score.align_icp``), held to the numpy restatement
tests/icp_ref.py (float32 brute-force correspondences, SVD Kabsch updates):

  1. I1: ``moved`` bit-equal to numpy's float32(float64 product) at n = 1, 63, 64, 65, 3 001.
  2. I2 on the two-box case at iteration 0, and with n = 1, 64, 65 and 0: the count exact, each of the other 16 sums within
     n 2^-53 sum|terms| of numpy's (the worst case of a reordered double sum), two launches the same bits, a threshold below every
     distance all zeros.
  3. I3 and the loop on every case of ``icp_ref.cases``: as many history rows as the reference, equal counts, fitness and status at every
     iteration, inlier RMSE within 1e-9 relative, the final T within 1e-9 (double rounding, 1e-16, times a conditioning of at most 1e3
     is 1e-13: four decades of margin, two below a float32 slip).  subset: T within 1e-6 of G (the source was rounded to float32: 6e-8
     per coordinate, times a small conditioning factor); none: status 3 and T the identity bit for bit; outliers: T bit-equal to
     two-box's.  Condition on the inputs, asserted on the reference alone: the least |d - threshold| over every evaluation is above
     1e-7, so -- the device's float32 distances being the brute force's -- no correspondence decision can differ.
  4. Freezing: ``check_every`` of 1, 5 and 31 give the same bits in T and in the history; two runs the same bits; a passed-in grid the
     same bits as a built one.
  5. Through the score: the two-box mesh with every triangle split into four three times as ground truth, the same mesh moved by G^-1
     as reconstruction, 20 000 samples: without ``align`` accuracy and completion above 0.3 cm; with it both below 1e-3 cm and the
     completion ratio 100; the motion found matches G within 1e-3 (cm, degrees); ``align=False`` returns today's dict; with culling the
     ICP runs on the culled vertices.
  6. Hands off: ``align_icp`` on the vertices of a mesh extracted from a live ``FusedEngine`` leaves the map, the Adam moments,
     ``variables`` and the current camera bit-unchanged.
  7. ``python -m splatam_amd.mesh_score REC GT --align`` prints the ``Alignment:`` line and the figures ``score_mesh(align=True)`` returns;
     without ``--align`` the output is today's."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_ref as I
import meshscore_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = I.cases()
SAMPLES = 20_000


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def _state(T):
    s = np.zeros(I.STATE)
    s[:16] = np.asarray(T, dtype=np.float64).reshape(-1)
    return _dev(s)


# ---------------------------------------------------------------------------------------------------------------- 1. I1
@pytest.mark.parametrize("n", (1, 63, 64, 65, 3001))
def test_transform_equals_numpy_bit_for_bit(n):
    from splatam_amd import mesh_score as S
    src = CASES["two-box"]["source"][:n]
    for T in (I.G, np.linalg.inv(I.G), np.eye(4)):
        got = S.apply_state(_dev(src), _state(T)).cpu().numpy()
        assert got.shape == (n, 3) and got.tobytes() == I.move32(T, src).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2. I2
@pytest.fixture(scope="module")
def first_evaluation():
    """The two-box case at iteration 0 (T the identity): the restatement's distances, indices and mask."""
    k = CASES["two-box"]
    moved, d2, idx, mask, count, _, _, d = I.evaluate(np.eye(4), k["source"], k["target"], k["threshold"])
    return dict(source=k["source"], target=k["target"], d2=d2, idx=idx, mask=mask, count=count, d=d)


@pytest.mark.parametrize("n", (3001, 1, 64, 65, 0))
def test_moments_against_numpy(first_evaluation, n):
    from splatam_amd import _capi
    from splatam_amd import mesh_score as S
    e = first_evaluation
    src, tgt, thr, c = e["source"][:n], e["target"], 0.1, (0.2, 0.55, 0.3)
    dsrc, dtgt, state = _dev(src), _dev(tgt), _state(np.eye(4))
    grid = S.NearestGrid(dtgt)
    dist2, index = grid.query(S.apply_state(dsrc, state))
    assert dist2.cpu().numpy().tobytes() == e["d2"][:n].tobytes() and index.cpu().numpy().tobytes() == e["idx"][:n].tobytes()
    rows = [S.accumulate_moments(dsrc, dtgt, dist2, index, thr, c, state).cpu().numpy() for _ in range(2)]
    assert rows[0].shape == (_capi.SPLAT_ICP_ROWS, 17) and rows[0].tobytes() == rows[1].tobytes()
    used = max(1, -(-n // 256))                                          # (one workgroup per 256 points, at least one)
    assert not rows[0][used:].any()
    got = np.array([math.fsum(rows[0][:used, k]) for k in range(17)])   # the rows added exactly: only the kernel's own order is judged
    want, mag = I.sums17(src.astype(np.float64), tgt[e["idx"][:n]], e["d2"][:n], e["mask"][:n], c)
    print(f"n = {n}: count {got[0]:.0f} (numpy {want[0]:.0f}); worst |sum - numpy| / (n 2^-53 sum|terms|) "
          f"{(np.abs(got - want)[1:] / np.maximum(max(n, 1) * 2.0 ** -53 * mag[1:], 1e-300)).max():.3f}")
    assert got[0] == want[0] == int(e["mask"][:n].sum())
    assert (np.abs(got - want) <= n * 2.0 ** -53 * mag).all()
    if n == 3001:
        assert got[0] == 3001
    # a threshold below every distance: all zeros
    low = float(e["d"][:n].min()) * 0.5 if n else 0.05
    assert low > 0
    zero = S.accumulate_moments(dsrc, dtgt, dist2, index, low, c, state).cpu().numpy()
    assert not zero[:used].any()


# ---------------------------------------------------------------------------------------------------------------- 3. I3 and the loop
@pytest.fixture(scope="module")
def device_runs():
    """``align_icp`` of every case, once."""
    from splatam_amd import mesh_score as S
    return {name: S.align_icp(_dev(k["source"]), _dev(k["target"]), threshold=k["threshold"], init=k["init"]) for name, k in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_loop_against_the_restatement(device_runs, name):
    ref, got = I.reference(name), device_runs[name]
    h, rh = got["history"], ref["history"]
    print(f"{name}: {len(rh)} evaluations, status {ref['status']}, margin {ref['margin']:.3e}; device {len(h)} evaluations, status {got['status']}, "
          f"|T - ref| {np.abs(got['transformation'] - ref['T']).max():.2e}, |T - G| {np.abs(got['transformation'] - I.G).max():.2e}")
    assert ref["margin"] > 1e-7
    assert h.shape == rh.shape and got["status"] == ref["status"] and got["iterations"] == len(rh) - 1
    assert np.array_equal(h[:, 0], rh[:, 0]) and np.array_equal(h[:, 1], rh[:, 1]) and np.array_equal(h[:, 3], rh[:, 3])
    assert (np.abs(h[:, 2] - rh[:, 2]) <= 1e-9 * np.abs(rh[:, 2])).all()
    assert np.abs(got["transformation"] - ref["T"]).max() <= 1e-9
    assert np.array_equal(got["transformation"][3], (0.0, 0.0, 0.0, 1.0))
    assert got["correspondences"] == rh[-1, 0] and got["fitness"] == rh[-1, 1] and abs(got["inlier_rmse"] - rh[-1, 2]) <= 1e-9 * max(rh[-1, 2], 1e-300)
    if name == "subset":
        assert np.abs(got["transformation"] - I.G).max() <= 1e-6
    if name == "none":
        assert got["status"] == 3 and got["correspondences"] == 0 and got["transformation"].tobytes() == np.eye(4).tobytes()
    if name == "outliers":
        assert got["transformation"].tobytes() == device_runs["two-box"]["transformation"].tobytes()
        assert got["fitness"] == 3001 / 3601


def test_bad_inputs_are_refused():
    from splatam_amd import mesh_score as S
    src, tgt = _dev(CASES["subset"]["source"]), _dev(CASES["subset"]["target"])
    for kw in (dict(threshold=0.0), dict(threshold=float("inf")), dict(threshold=float("nan")), dict(init=np.diag([1.0, 1.0, -1.0, 1.0])),
               dict(init=np.full((4, 4), np.nan)), dict(init=2 * np.eye(4)), dict(max_iterations=-1), dict(check_every=0)):
        with pytest.raises(ValueError):
            S.align_icp(src, tgt, **kw)
    with pytest.raises(ValueError):
        S.align_icp(src[:0], tgt)
    with pytest.raises(ValueError):
        S.align_icp(src, tgt[:0])
    limit = S.align_icp(src, tgt, max_iterations=2)
    ref = I.icp(CASES["subset"]["source"], CASES["subset"]["target"], max_iterations=2)
    assert limit["status"] == 2 == ref["status"] and limit["iterations"] == 2 and len(limit["history"]) == 3
    assert np.abs(limit["transformation"] - ref["T"]).max() <= 1e-9
    none = S.align_icp(src, tgt, max_iterations=0)
    assert none["status"] == 2 and none["transformation"].tobytes() == np.eye(4).tobytes() and len(none["history"]) == 1


# ---------------------------------------------------------------------------------------------------------------- 4. freezing
def test_the_result_does_not_depend_on_check_every(device_runs):
    from splatam_amd import mesh_score as S
    k = CASES["tight"]
    src, tgt = _dev(k["source"]), _dev(k["target"])
    base = device_runs["tight"]
    grid = S.NearestGrid(tgt)
    runs = [S.align_icp(src, tgt, threshold=k["threshold"], check_every=c) for c in (1, 5, 31)]
    runs.append(S.align_icp(src, tgt, threshold=k["threshold"]))
    runs.append(S.align_icp(src, tgt, threshold=k["threshold"], grid=grid))
    runs.append(S.align_icp(src, tgt, threshold=k["threshold"], grid=grid, check_every=2))
    for r in runs:
        assert r["transformation"].tobytes() == base["transformation"].tobytes() and r["history"].tobytes() == base["history"].tobytes()
        assert {key: r[key] for key in ("fitness", "inlier_rmse", "correspondences", "iterations", "status")} == \
               {key: base[key] for key in ("fitness", "inlier_rmse", "correspondences", "iterations", "status")}


# ---------------------------------------------------------------------------------------------------------------- 5. through the score
def subdivide(vertices, faces, k):
    """Every triangle into four, ``k`` times, midpoints shared (formed in float64, rounded once at the end)."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    for _ in range(k):
        e = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        n, F = len(v), len(f)
        m01, m12, m20 = n + inv[:F], n + inv[F:2 * F], n + inv[2 * F:]
        v = np.concatenate((v, 0.5 * (v[uniq[:, 0]] + v[uniq[:, 1]])))
        f = np.concatenate((np.stack((f[:, 0], m01, m20), 1), np.stack((m01, f[:, 1], m12), 1), np.stack((m20, m12, f[:, 2]), 1),
                            np.stack((m01, m12, m20), 1)))
    return v.astype(np.float32), f.astype(np.int32)


@pytest.fixture(scope="module")
def pair():
    gv, gf = subdivide(*I.two_box_mesh(), 3)
    assert 700 < len(gv) < 900
    return (I.moved_back(gv), gf, None), (gv, gf, None)


def test_score_with_and_without_alignment(pair):
    from splatam_amd import mesh_score as S
    rec, gt = pair
    plain = S.score_mesh(rec, gt, samples=SAMPLES)
    off = S.score_mesh(rec, gt, samples=SAMPLES, align=False)
    on = S.score_mesh(rec, gt, samples=SAMPLES, align=True)
    a = on["alignment"]
    print(f"without: accuracy {plain['accuracy_cm']:.4f} cm, completion {plain['completion_cm']:.4f} cm; with: {on['accuracy_cm']:.3e} cm, "
          f"{on['completion_cm']:.3e} cm, ratio {on['completion_ratio']}; {S.format_alignment(a)}")
    assert tuple(plain) == S.KEYS and "alignment" not in plain and plain == off
    assert plain["accuracy_cm"] > 0.3 and plain["completion_cm"] > 0.3
    assert tuple(on) == S.KEYS + ("alignment",)
    assert on["accuracy_cm"] < 1e-3 and on["completion_cm"] < 1e-3 and on["completion_ratio"] == 100.0
    want_cm, want_deg = 100.0 * float(np.linalg.norm(I.G[:3, 3])), 3.0
    assert abs(a["translation_cm"] - want_cm) <= 1e-3 and abs(a["rotation_deg"] - want_deg) <= 1e-3
    assert a["status"] == 1 and a["fitness"] == 1.0 and np.abs(a["transformation"] - I.G).max() <= 1e-6
    ref = I.icp(rec[0], gt[0])
    assert len(a["history"]) == len(ref["history"]) and np.abs(a["transformation"] - ref["T"]).max() <= 1e-9
    # keywords reach align_icp; device meshes score the same as host ones
    short = S.score_mesh((_dev(rec[0]), _dev(rec[1]), None), (_dev(gt[0]), _dev(gt[1]), None), samples=SAMPLES, align=dict(max_iterations=1))
    assert short["alignment"]["status"] == 2 and short["alignment"]["iterations"] == 1 and short["accuracy_cm"] > on["accuracy_cm"]
    again = S.score_mesh((_dev(rec[0]), _dev(rec[1]), None), (_dev(gt[0]), _dev(gt[1]), None), samples=SAMPLES, align=True)
    assert again["alignment"]["transformation"].tobytes() == a["transformation"].tobytes() and again["accuracy_cm"] == on["accuracy_cm"]


def test_alignment_runs_on_the_culled_vertices(pair):
    from splatam_amd import mesh_score as S
    import meshrender_ref as MRR
    rec, gt = pair
    # a component straight above the ring of cameras, outside every frustum, 5 m from everything
    ev, ef = R.box_mesh(sides=(0.2, 0.2, 0.2), origin=(0.1, 0.45, 6.0), zero_area=False)
    with_extra = (np.concatenate((rec[0], ev)), np.concatenate((rec[1], ef + len(rec[0]))).astype(np.int32), None)
    views = MRR.ring_views(6, 3.0, centre=(0.2, 0.55, 0.3), height=0.8).astype(np.float64)       # (the pair fills 18 of the 25 degrees)
    intr, size = (120.0, 120.0, 79.5, 55.5), (160, 112)
    base = S.score_with_views(rec, gt, samples=SAMPLES, cull_w2c=views, intrinsics=intr, size=size, align=True)
    got = S.score_with_views(with_extra, gt, samples=SAMPLES, cull_w2c=views, intrinsics=intr, size=size, align=True, depth_l1_views=2)
    uncull = S.score_mesh(with_extra, gt, samples=SAMPLES, align=True)
    a, b, u = got["alignment"], base["alignment"], uncull["alignment"]
    print(f"culled: fitness {a['fitness']} of {a['correspondences']}; without the component {b['fitness']}; not culled {u['fitness']}")
    assert a["fitness"] == b["fitness"] == 1.0 and a["correspondences"] == b["correspondences"] == len(rec[0])
    assert a["transformation"].tobytes() == b["transformation"].tobytes()
    assert u["fitness"] == len(rec[0]) / (len(rec[0]) + len(ev)) < 1.0  # (the component counts when nothing removes it)
    assert got["accuracy_cm"] < 1e-3 and got["completion_cm"] < 1e-3 and got["views"] == 2
    assert got["depth_l1_cm"] < 0.05                                     # (a pixel that flips across a silhouette is 100 cm / 35 840 pixels)
    in_map = S.score_culled_in_map_frame(with_extra, gt, views, intr, size, samples=SAMPLES, align=True)      # (run --cull --align)
    assert in_map["alignment"]["transformation"].tobytes() == b["transformation"].tobytes() and in_map["accuracy_cm"] == base["accuracy_cm"]
    off = S.score_with_views(with_extra, gt, samples=SAMPLES, cull_w2c=views, intrinsics=intr, size=size, depth_l1_views=2)
    assert "alignment" not in off and off["accuracy_cm"] > 0.3 and off["depth_l1_cm"] > got["depth_l1_cm"]


# ---------------------------------------------------------------------------------------------------------------- 6. hands off
def test_align_icp_leaves_a_live_engine_untouched():
    from splatam_amd import mesh as M
    from splatam_amd import mesh_score as S
    from splatam_amd.fused import PARAM_ORDER
    from test_gpu_meshscore import H, W, _engine
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
    shifted = (mesh.vertices + torch.tensor([0.01, 0.0, 0.0], device="cuda")).contiguous()
    found = S.align_icp(shifted, mesh.vertices)
    scored = S.score_mesh(M.Mesh(shifted, mesh.faces, mesh.colors), mesh, samples=SAMPLES, align=True)
    torch.cuda.synchronize()
    after = snapshot()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    for name, t in before.items():
        assert torch.equal(bits(t), bits(after[name])), name
    assert eng._camera is main
    assert found["status"] in (1, 2) and found["fitness"] == 1.0 and found["history"][-1, 2] < found["history"][0, 2] <= 0.01 + 1e-6
    assert scored["alignment"]["transformation"].tobytes() == found["transformation"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 7. command line
def test_the_command_prints_the_alignment(pair, tmp_path):
    from splatam_amd import mesh_score as S
    from splatam_amd.export import save_mesh_ply
    rec, gt = pair
    save_mesh_ply(str(tmp_path / "rec.ply"), rec[0], rec[1])
    save_mesh_ply(str(tmp_path / "gt.ply"), gt[0], gt[1])
    root = os.path.dirname(HERE)
    base = [sys.executable, "-m", "splatam_amd.mesh_score", str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "--samples", "5000", "--seed", "3"]
    run = lambda args: subprocess.run(args, cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE,  # noqa: E731
                                      stderr=subprocess.PIPE, text=True)
    done = run(base + ["--align", "--align-threshold", "0.08", "--align-iterations", "20"])
    assert done.returncode == 0, done.stdout + done.stderr
    score = S.score_mesh(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), samples=5000, seed=3, align=dict(threshold=0.08, max_iterations=20))
    assert done.stdout == S.format_score(score) + "\n", done.stdout
    lines = done.stdout.splitlines()
    assert len(lines) == 5 and lines[0].startswith("Alignment: fitness 1.000000, inlier RMSE ") and lines[1].startswith("Accuracy: ")
    assert "(converged)" in lines[0] and "rotation 3.0000 deg" in lines[0]
    assert score["alignment"]["status"] == 1 and score["accuracy_cm"] < 1e-3
    plain = run(base)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    want = S.score_mesh(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), samples=5000, seed=3)
    assert "alignment" not in want and plain.stdout == S.format_score(want) + "\n" and len(plain.stdout.splitlines()) == 4
    assert want["accuracy_cm"] > 0.3
    refused = run(base + ["--align-threshold", "0.05"])
    assert refused.returncode != 0 and "need --align" in refused.stderr
