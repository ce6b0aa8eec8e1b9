"""The ICP layer without a GPU: splatam_amd/csrc/icp_math.h compiled for the host (tests/icp_math_shim.cpp: the loop bodies of the kernels
of csrc/icp.hip) against numpy and the restatement tests/icp_ref.py.

1. SOLVER: Horn's quaternion solve (cyclic Jacobi on the symmetric 4 x 4) against numpy's SVD Kabsch with the determinant fix, on the
   cross-covariances of generic clouds, a planar cloud, a collinear cloud (the rotation is not unique: the residual sum |U p - q|^2 is
   compared, not the matrix), a cloud whose unconstrained optimum is a reflection, the identity and a 180 degree turn.  U^T U - I and
   det U - 1 within 1e-12; U within 1e-9 of numpy's wherever the two largest eigenvalues of Horn's matrix differ by more than 1e-3 of
   the largest.  (Double rounding, 1e-16, times that conditioning, 1e3, is 1e-13: 1e-9 leaves four decades over it and stays two below
   what a float32 slip anywhere would produce, about 1e-7 on coordinates of order 1.)
   The header as a stand-alone program under the address and undefined-behaviour sanitizers, on degenerate inputs.
2. THE LOOP on the host: I1 / I2 / I3 through the shim, with the restatement's float32 brute force for the correspondences, against
   ``icp_ref.icp`` on a small cloud: the same history, T within 1e-9; a frozen T once the status is set.
3. ``icp_ref`` itself: a pure translation of an exact subset is recovered in one update.
4. PLUMBING: the entry points and constants exist, the ABI is still 17, NULL pointers and negative sizes are refused; ``align_icp`` and
   ``score_mesh(align=True)`` on ``device="cpu"`` raise the module's "no CPU path" error; ``align`` false leaves ``score_mesh``'s
   signature defaults and keys as they were."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import icp_ref as I
import meshscore_ref as R
from tests.util import host_shim

F32P, F64P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


def load_shim():
    lib = host_shim("icp_math_shim", "icp_math.h", "meshscore_math.h")
    lib.im_horn.restype = None
    lib.im_horn.argtypes = [F64P, F64P]
    lib.im_transform.restype = None
    lib.im_transform.argtypes = [F64P, F32P, C.c_longlong, F32P]
    lib.im_accumulate.restype = None
    lib.im_accumulate.argtypes = [F64P, F32P, F32P, C.c_longlong, F32P, I32P, C.c_longlong, C.c_double, F64P, F64P]
    lib.im_solve_sums.restype = None
    lib.im_solve_sums.argtypes = [F64P, F64P, F64P, F64P]
    lib.im_step.restype = None
    lib.im_step.argtypes = [F64P, F64P, C.c_longlong, C.c_int32, C.c_double, C.c_double, F64P, F64P]
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _p(a, t):
    return a.ctypes.data_as(t)


def shim_horn(shim, H):
    H, U = np.ascontiguousarray(H, dtype=np.float64), np.empty((3, 3))
    shim.im_horn(_p(H, F64P), _p(U, F64P))
    return U


def shim_transform(shim, T, source):
    T, s = np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(source, dtype=np.float32)
    moved = np.empty_like(s)
    shim.im_transform(_p(T, F64P), _p(s, F32P), len(s), _p(moved, F32P))
    return moved


def shim_accumulate(shim, T, source, targets, d2, idx, thr, origin):
    T, s, t = np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(source, np.float32), np.ascontiguousarray(targets, np.float32)
    d2, idx, c, sums = np.ascontiguousarray(d2, np.float32), np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(origin, np.float64), np.empty(17)
    shim.im_accumulate(_p(T, F64P), _p(s, F32P), _p(t, F32P), len(t), _p(d2, F32P), _p(idx, I32P), len(s), thr, _p(c, F64P), _p(sums, F64P))
    return sums


# ---------------------------------------------------------------------------------------------------------------- 1. the solver
def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _covariance(p, q):
    return (p - p.mean(axis=0)).T @ (q - q.mean(axis=0))


def solver_cases():
    """name -> (p, q) float64 [n, 3]: q is what the solve should bring p onto."""
    rng = np.random.default_rng(11)
    out = {}
    for k in range(6):
        p = rng.normal(size=(200, 3)) * (1.0, 0.6, 0.3)
        out[f"generic-{k}"] = (p, p @ _rotation(rng).T + rng.normal(size=3) + (0.0 if k % 2 else 0.02) * rng.normal(size=p.shape))
    small = I.rigid(3.0, (0.3, -0.5, 0.8), (0, 0, 0))[:3, :3]
    p = rng.normal(size=(300, 3))
    out["small-angle"] = (p, p @ small.T + 0.01 * rng.normal(size=p.shape))
    plane = rng.normal(size=(150, 3)) * (1.0, 0.7, 0.0)
    out["planar"] = (plane, plane @ _rotation(rng).T + 0.3)
    line = np.outer(rng.normal(size=80), (0.6, -0.3, 0.74))
    out["collinear"] = (line, line @ _rotation(rng).T)
    p = rng.normal(size=(120, 3)) * (1.0, 0.8, 0.25)
    out["reflection"] = (p, p * (1.0, 1.0, -1.0) + 0.01 * rng.normal(size=p.shape))          # the best ORTHOGONAL map is the mirror z -> -z
    out["identity"] = (p, p.copy())
    out["half-turn"] = (p, p * (-1.0, -1.0, 1.0))
    return out


SOLVER = solver_cases()


@pytest.mark.parametrize("name", list(SOLVER))
def test_horn_solve_against_numpy_kabsch(shim, name):
    p, q = SOLVER[name]
    H = _covariance(p, q)
    U = shim_horn(shim, H)
    ref = I.kabsch_from_covariance(H)[:3, :3]
    lam = np.linalg.eigvalsh(I.horn_matrix(H))[::-1]
    gap = (lam[0] - lam[1]) / abs(lam[0])
    a, b = p - p.mean(axis=0), q - q.mean(axis=0)
    res, res_ref = float(((a @ U.T - b) ** 2).sum()), float(((a @ ref.T - b) ** 2).sum())
    print(f"{name}: |U^T U - I| {np.abs(U.T @ U - np.eye(3)).max():.2e}, det - 1 {np.linalg.det(U) - 1:.2e}, eigenvalue gap {gap:.3e}, "
          f"|U - numpy| {np.abs(U - ref).max():.2e}, residual {res:.6e} (numpy {res_ref:.6e})")
    assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(U) - 1.0) <= 1e-12
    assert abs(np.linalg.det(ref) - 1.0) <= 1e-12
    if name == "reflection":                                             # (the unconstrained optimum IS improper: the fix had work to do)
        u, _, vt = np.linalg.svd(H)
        assert np.linalg.det(vt.T @ u.T) < 0
    if name == "collinear":
        assert gap <= 1e-9                                               # (not unique: any turn about the line)
    else:
        assert gap > 1e-3
    if gap > 1e-3:
        assert np.abs(U - ref).max() <= 1e-9
    assert abs(res - res_ref) <= 1e-9 * max(float((b ** 2).sum()), 1.0)
    if name == "identity":
        assert np.abs(U - np.eye(3)).max() <= 1e-15
    if name == "half-turn":
        assert np.abs(U - np.diag([-1.0, -1.0, 1.0])).max() <= 1e-12


def test_degenerate_sums_give_a_proper_rotation(shim):
    for H in (np.zeros((3, 3)), np.diag([1.0, 0.0, 0.0]), -np.eye(3), np.diag([1.0, 1.0, -1.0]), 1e-300 * np.eye(3), 1e150 * np.eye(3)):
        U = shim_horn(shim, H)
        assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(U) - 1.0) <= 1e-12, H
    assert np.array_equal(shim_horn(shim, np.zeros((3, 3))), np.eye(3))                           # no information: stay


def test_header_under_address_and_ub_sanitizers(tmp_path):
    """The shim's host functions as a stand-alone program (its own main) built with -fsanitize=address,undefined: cross-covariances
    that are zero, improper, huge, denormal and not numbers; correspondences with an index out of range, a NaN and an infinite distance;
    the loop run past its stop and past its iteration limit; no points at all.  Any sanitizer report or wrong answer is a non-zero
    exit.  The runtimes are linked statically; nothing loaded into python is involved."""
    exe = str(tmp_path / "icp_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DICP_SHIM_MAIN", "-o", exe,
                           os.path.join(os.path.dirname(__file__), "icp_math_shim.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout


def test_solve_from_sums_does_not_depend_on_the_origin(shim):
    rng = np.random.default_rng(3)
    p = rng.normal(size=(500, 3)) + (4.0, -2.0, 1.0)
    M = I.rigid(7.0, (1.0, 2.0, -1.0), (0.05, 0.02, -0.03))
    q = (p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    ref = I.kabsch(p, q.astype(np.float64))
    for c in ((0.0, 0.0, 0.0), (4.0, -2.0, 1.0), (-30.0, 10.0, 5.0)):
        sums, _ = I.sums17(p, q, np.zeros(len(p), np.float32), np.ones(len(p), bool), c)
        U, u, cc = np.empty((3, 3)), np.empty(3), np.array(c)
        shim.im_solve_sums(_p(sums, F64P), _p(cc, F64P), _p(U, F64P), _p(u, F64P))
        assert np.abs(U - ref[:3, :3]).max() <= 1e-9 and np.abs(u - ref[:3, 3]).max() <= 1e-9, c
    assert np.abs(ref - M).max() < 1e-6                                  # (q was rounded to float32)


# ---------------------------------------------------------------------------------------------------------------- 2. the loop on the host
def host_loop(shim, src, tgt, thr, init=None, max_iterations=30, rel=1e-6, extra=0):
    """``align_icp``'s loop with the shim for I1 / I2 / I3 and the restatement's brute force for the query; ``extra`` evaluations are
    run after the stop."""
    state = np.zeros(I.STATE)
    state[:16] = (np.eye(4) if init is None else init).reshape(-1)
    history = np.zeros((max_iterations + 1, 4))
    c = 0.5 * (tgt.min(axis=0) + tgt.max(axis=0)).astype(np.float64)
    stopped = None
    for k in range(max_iterations + 1 + extra):
        moved = shim_transform(shim, state[:16], src)
        d2, idx = R.brute32(moved, tgt)
        sums = shim_accumulate(shim, state[:16], src, tgt, d2, idx, thr, c)
        shim.im_step(_p(state, F64P), _p(sums, F64P), len(src), max_iterations, rel, rel, _p(c, F64P), _p(history, F64P))
        if state[17] != 0 and stopped is None:
            stopped = k
            if not extra:
                break
    return state, history[:int(state[16]) + 1], stopped


def small_case():
    v, f = I.two_box_mesh()
    target = R.sample(v, f, 700, 3)[0]
    source = I.moved_back(R.sample(v, f, 401, 4)[0])
    return source, target


def test_host_loop_equals_the_restatement(shim):
    src, tgt = small_case()
    ref = I.icp(src, tgt, 0.1)
    state, history, _ = host_loop(shim, src, tgt, 0.1)
    print(f"small case: {len(history)} evaluations, status {state[17]:.0f}, |T - ref| {np.abs(state[:16].reshape(4, 4) - ref['T']).max():.2e}, "
          f"margin {ref['margin']:.2e}")
    assert ref["margin"] > 1e-7 and ref["status"] == 1 and 3 < len(ref["history"]) < 31
    assert len(history) == len(ref["history"]) and state[17] == ref["status"]
    assert np.array_equal(history[:, 0], ref["history"][:, 0]) and np.array_equal(history[:, 1], ref["history"][:, 1])
    assert np.array_equal(history[:, 3], ref["history"][:, 3])
    assert np.abs(history[:, 2] - ref["history"][:, 2]).max() <= 1e-9 * ref["history"][:, 2].max()
    assert np.abs(state[:16].reshape(4, 4) - ref["T"]).max() <= 1e-9
    # the limit: two updates, then status 2 with the evaluation of iteration 2
    ref2 = I.icp(src, tgt, 0.1, max_iterations=2)
    state2, history2, _ = host_loop(shim, src, tgt, 0.1, max_iterations=2)
    assert ref2["status"] == 2 and state2[17] == 2 and state2[16] == 2 and len(history2) == 3 == len(ref2["history"])
    assert np.abs(state2[:16].reshape(4, 4) - ref2["T"]).max() <= 1e-9
    # frozen: evaluations after the stop change nothing
    state3, history3, stopped = host_loop(shim, src, tgt, 0.1, extra=4)
    assert stopped == len(history) - 1 and state3.tobytes() == state.tobytes() and history3.tobytes() == history.tobytes()


def test_transform_and_sums_of_the_shim(shim):
    src, tgt = small_case()
    assert shim_transform(shim, I.G, src).tobytes() == I.move32(I.G, src).tobytes()
    moved, d2, idx, mask, count, _, _, _ = I.evaluate(I.G, src, tgt, 0.02)
    c = (0.2, 0.5, 0.3)
    sums = shim_accumulate(shim, I.G, src, tgt, d2, idx, 0.02, c)
    want, mag = I.sums17(I.move64(I.G, src), tgt[idx], d2, mask, c)
    assert 0 < count < len(src) and sums[0] == count
    assert (np.abs(sums - want) <= len(src) * 2.0 ** -53 * mag).all()


# ---------------------------------------------------------------------------------------------------------------- 3. icp_ref itself
def test_the_restatement_recovers_a_pure_translation_in_one_update():
    k = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3)
    target = (0.25 * k).astype(np.float32)                               # a lattice of spacing 0.25: exact in float32
    t = np.array([0.03125, -0.0625, 0.015625])                           # dyadic: the moved subset is exact too
    source = (target[::3].astype(np.float64) - t).astype(np.float32)
    assert np.array_equal(source.astype(np.float64) + t, target[::3].astype(np.float64))
    r = I.icp(source, target, 0.1)
    want = np.eye(4)
    want[:3, 3] = t
    assert r["status"] == 1 and len(r["history"]) == 3                   # evaluation 0, the update, evaluation 1 (exact), evaluation 2 (no change)
    assert np.abs(r["T"] - want).max() <= 1e-13                          # (the SVD's own rounding: a few units of 2^-52 on entries of order 1)
    assert r["history"][0, 1] == 1.0 and r["history"][0, 2] == pytest.approx(np.linalg.norm(t), rel=1e-7)
    assert r["history"][1, 2] <= 1e-15 and r["history"][2, 2] <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- 4. plumbing
def test_binding_and_header_name_the_entry_points():
    from splatam_amd import _capi
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "splat_hip.h")).read()
    L = _capi.lib()
    for name in ("splat_icp_transform", "splat_icp_accumulate", "splat_icp_solve"):
        assert hasattr(L, name) and name in _capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    for name in ("SPLAT_ICP_STATE", "SPLAT_ICP_ROWS", "SPLAT_ICP_SUMS", "SPLAT_ICP_ITERATION", "SPLAT_ICP_STATUS", "SPLAT_ICP_FITNESS",
                 "SPLAT_ICP_RMSE", "SPLAT_ICP_PREV_FITNESS", "SPLAT_ICP_PREV_RMSE", "SPLAT_ICP_COUNT", "SPLAT_ICP_POINTS"):
        assert getattr(_capi, name) == int(re.search(rf"#define {name} (\d+)", header).group(1)), name
    assert (_capi.SPLAT_ICP_STATE, _capi.SPLAT_ICP_ROWS, _capi.SPLAT_ICP_SUMS) == (I.STATE, I.ROWS, I.SUMS)
    shim = load_shim()
    assert shim.im_sums() == _capi.SPLAT_ICP_SUMS
    assert [shim.im_state_slot(k) for k in range(8)] == [_capi.SPLAT_ICP_ITERATION, _capi.SPLAT_ICP_STATUS, _capi.SPLAT_ICP_FITNESS,
                                                         _capi.SPLAT_ICP_RMSE, _capi.SPLAT_ICP_PREV_FITNESS, _capi.SPLAT_ICP_PREV_RMSE,
                                                         _capi.SPLAT_ICP_COUNT, _capi.SPLAT_ICP_POINTS]
    assert L.splat_abi_version() == 17 and _capi.ABI_VERSION == 17
    # refusals need no device: nothing is launched
    c, p = (C.c_double * 3)(0.0, 0.0, 0.0), 1 << 12
    assert L.splat_icp_transform(p, -1, p, p, None) == 1 and L.splat_icp_transform(None, 4, p, p, None) == 1
    assert L.splat_icp_transform(p, 4, None, p, None) == 1 and L.splat_icp_transform(p, 4, p, None, None) == 1
    assert L.splat_icp_accumulate(p, p, 4, p, p, -1, 0.1, c, p, p, None) == 1 and L.splat_icp_accumulate(p, p, -1, p, p, 4, 0.1, c, p, p, None) == 1
    assert L.splat_icp_accumulate(None, p, 4, p, p, 4, 0.1, c, p, p, None) == 1 and L.splat_icp_accumulate(p, None, 4, p, p, 4, 0.1, c, p, p, None) == 1
    assert L.splat_icp_accumulate(p, p, 4, None, p, 4, 0.1, c, p, p, None) == 1 and L.splat_icp_accumulate(p, p, 4, p, None, 4, 0.1, c, p, p, None) == 1
    assert L.splat_icp_accumulate(p, p, 4, p, p, 4, 0.1, None, p, p, None) == 1 and L.splat_icp_accumulate(p, p, 4, p, p, 4, 0.1, c, None, p, None) == 1
    assert L.splat_icp_accumulate(p, p, 4, p, p, 4, 0.1, c, p, None, None) == 1 and L.splat_icp_accumulate(p, p, 4, p, p, 4, float("nan"), c, p, p, None) == 1
    assert L.splat_icp_solve(None, 4, 30, 1e-6, 1e-6, c, p, p, None) == 1 and L.splat_icp_solve(p, -1, 30, 1e-6, 1e-6, c, p, p, None) == 1
    assert L.splat_icp_solve(p, 4, -1, 1e-6, 1e-6, c, p, p, None) == 1 and L.splat_icp_solve(p, 4, 30, 1e-6, 1e-6, None, p, p, None) == 1
    assert L.splat_icp_solve(p, 4, 30, 1e-6, 1e-6, c, None, p, None) == 1 and L.splat_icp_solve(p, 4, 30, 1e-6, 1e-6, c, p, None, None) == 1


def test_there_is_no_cpu_path():
    import torch
    from splatam_amd import mesh_score as S
    v, f = I.two_box_mesh()
    pts = torch.from_numpy(v)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.align_icp(pts, pts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.score_mesh((v, f, None), (v, f, None), samples=100, align=True, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.score_with_views((v, f, None), (v, f, None), samples=100, align=True, device="cpu")


def test_align_off_leaves_the_signature_and_the_keys():
    from splatam_amd import mesh_score as S
    sig = inspect.signature(S.score_mesh).parameters
    assert [(k, p.default) for k, p in sig.items()][2:] == [("samples", 200_000), ("threshold", 0.05), ("seed", 0), ("transform", None),
                                                            ("device", "cuda:0"), ("cell", None), ("align", False)]
    views = inspect.signature(S.score_with_views).parameters
    assert views["align"].default is False and list(views)[-1] == "align" and views["depth_l1_views"].default == 0
    assert S.KEYS == ("accuracy_cm", "completion_cm", "completion_ratio", "precision", "recall", "fscore", "max_rec_to_gt", "max_gt_to_rec",
                      "samples") and "alignment" not in S.KEYS
    score = dict.fromkeys(S.KEYS, 0.0)
    score["samples"] = 10
    assert not S.format_score(score).startswith("Alignment:") and S.format_score(score).startswith("Accuracy: ")
    found = dict(fitness=1.0, inlier_rmse=0.01, iterations=7, status=1, translation_cm=2.5, rotation_deg=3.0)
    text = S.format_score(dict(score, alignment=found))
    assert text.startswith("Alignment: fitness 1.000000, inlier RMSE 1.0000 cm, 7 iterations (converged), translation 2.5000 cm, rotation 3.0000 deg\n")
    assert text.split("\n", 1)[1] == S.format_score(score)
    cm, deg = S.motion_of(I.G)
    assert abs(cm - 100 * np.linalg.norm([0.02, -0.015, 0.01])) <= 1e-12 and abs(deg - 3.0) <= 1e-12
    for bad in (np.eye(3), np.diag([1.0, 1.0, -1.0, 1.0]), 2.0 * np.eye(4), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            S._rigid(bad)
    assert np.array_equal(S._rigid(I.G), I.G)


def test_the_commands_refuse_alignment_options_without_what_they_need(capsys):
    from splatam_amd import mesh_score, run
    with pytest.raises(SystemExit):
        run.main(["experiment.py", "--mesh", "--align"])
    assert "--align needs --gt-mesh" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh_score.main(["rec.ply", "gt.ply", "--align-iterations", "5"])
    assert "need --align" in capsys.readouterr().err
    assert inspect.signature(run.run).parameters["align"].default is False
