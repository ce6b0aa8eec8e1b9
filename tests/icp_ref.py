"""numpy restatement of the ICP layer (splatam_amd/csrc/icp_math.h, csrc/icp.hip, ``mesh_score.align_icp``), the yardstick of
tests/test_icp_cpu.py and tests/test_gpu_icp.py.  Independent of the code under test: correspondences by the float32 brute force of
tests/meshscore_ref.py, the rigid update by ``numpy.linalg.svd`` (Kabsch with the determinant fix) on the double moved points.

Per iteration: ``moved = float32(float64(src) @ R^T + t)``; ``brute32(moved, tgt)``; the mask ``sqrt(float64(d2)) < thr``; fitness =
count / n and inlier RMSE = sqrt(sum d2 / count) (0 without correspondences); the Open3D-style stop (iteration > 0 and both changed by
less than the relative_*: status 1; iteration == max_iterations: 2; count < 3: 3); otherwise ``T <- U @ T``.

It also builds the cases both test files run (``cases``)."""
import numpy as np

import meshscore_ref as R

STATE, ROWS, SUMS = 24, 256, 17


def rigid(angle_deg, axis, t):
    """float64 4 x 4: rotation by ``angle_deg`` about ``axis`` (Rodrigues), translation ``t``."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(angle_deg)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = t
    return M


def move64(T, points):
    return np.asarray(points, dtype=np.float32).astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def move32(T, points):
    """float32(float64 product): one rounding at the end."""
    return move64(T, points).astype(np.float32)


def kabsch(p, q):
    """The rigid motion (4 x 4) that minimises sum |U p + u - q|^2 over the paired float64 rows, U a PROPER rotation: SVD of the
    cross-covariance with the determinant fix."""
    a, b = p.mean(axis=0), q.mean(axis=0)
    H = (p - a).T @ (q - b)
    return kabsch_from_covariance(H, a, b)


def kabsch_from_covariance(H, a=(0.0, 0.0, 0.0), b=(0.0, 0.0, 0.0)):
    """... from H = sum (p - a)(q - b)^T and the centroids."""
    u, _, vt = np.linalg.svd(np.asarray(H, dtype=np.float64))
    d = np.sign(np.linalg.det(vt.T @ u.T))
    U = vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T
    M = np.eye(4)
    M[:3, :3] = U
    M[:3, 3] = np.asarray(b) - U @ np.asarray(a)
    return M


def horn_matrix(H):
    """Horn's symmetric 4 x 4 of the cross-covariance H (row: source component): its largest eigenvalue's eigenvector is the rotation's
    quaternion (w, x, y, z)."""
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = np.asarray(H, dtype=np.float64)
    return np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                     [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                     [zx - xz, xy + yx, -xx + yy - zz, yz + zy],
                     [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])


def sums17(moved64, q32, d2, mask, c):
    """The 17 sums of I2 over the masked rows, each by ``math.fsum`` (exact, rounded once), and per sum the sum of |terms|."""
    import math
    a = moved64[mask] - np.asarray(c, dtype=np.float64)
    b = np.asarray(q32, dtype=np.float32).astype(np.float64)[mask] - np.asarray(c, dtype=np.float64)
    terms = [np.ones(len(a)), np.asarray(d2, dtype=np.float32).astype(np.float64)[mask]] + [a[:, k] for k in range(3)] + [b[:, k] for k in range(3)]
    terms += [a[:, r] * b[:, k] for r in range(3) for k in range(3)]
    return np.array([math.fsum(t) for t in terms]), np.array([math.fsum(np.abs(t)) for t in terms])


def evaluate(T, src, tgt, thr):
    """One evaluation at ``T``: (moved float32, d2 float32, index, mask, count, fitness, inlier RMSE)."""
    moved = move32(T, src)
    d2, idx = R.brute32(moved, tgt)
    d = np.sqrt(d2.astype(np.float64))
    mask = d < thr
    count = int(mask.sum())
    fitness = count / len(src) if count else 0.0
    rmse = float(np.sqrt(d2.astype(np.float64)[mask].sum() / count)) if count else 0.0
    return moved, d2, idx, mask, count, fitness, rmse, d


def icp(src, tgt, thr=0.1, init=None, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """dict(T, status, history [k, 4] = (count, fitness, inlier RMSE, status after the evaluation), margin = the least |d - thr| over
    every evaluation)."""
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    history, prev, margin, status = [], None, np.inf, 0
    for it in range(max_iterations + 1):
        _, _, idx, mask, count, fitness, rmse, d = evaluate(T, src, tgt, thr)
        margin = min(margin, float(np.abs(d - thr).min()))
        if it > 0 and abs(fitness - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            status = 1
        elif it == max_iterations:
            status = 2
        elif count < 3:
            status = 3
        history.append((count, fitness, rmse, status))
        if status:
            break
        T = kabsch(move64(T, src)[mask], np.asarray(tgt, dtype=np.float32).astype(np.float64)[idx[mask]]) @ T
        prev = (fitness, rmse)
    return dict(T=T, status=status, history=np.array(history, dtype=np.float64), margin=margin)


# ---------------------------------------------------------------------------------------------------------------- the cases
G = rigid(3.0, (0.3, -0.5, 0.8), (0.02, -0.015, 0.01))


def two_box_mesh():
    """Two boxes of unequal sides, one mesh: no symmetry."""
    v0, f0 = R.box_mesh(zero_area=False)
    v1, f1 = R.box_mesh(sides=(0.3, 0.2, 0.25), origin=(0.1, 0.35, 0.5), zero_area=False)
    return np.concatenate((v0, v1)), np.concatenate((f0, f1 + len(v0))).astype(np.int32)


def moved_back(points):
    """``points`` moved by G^-1, rounded to float32: G registers them again."""
    return move32(np.linalg.inv(G), points)


_cases = None


def cases():
    """name -> dict(source, target, threshold, init): the clouds every ICP test runs."""
    global _cases
    if _cases is None:
        v, f = two_box_mesh()
        target = R.sample(v, f, 4000, 1)[0]
        source = moved_back(R.sample(v, f, 3001, 2)[0])
        rng = np.random.default_rng(5)
        far = (np.array([3.0, 0.5, 0.3]) + 0.2 * rng.random((600, 3))).astype(np.float32)         # about 3 m away
        subset = moved_back(target[rng.permutation(4000)[:1777]])
        c = lambda s, thr=0.1, init=None: dict(source=np.ascontiguousarray(s), target=target, threshold=thr, init=init)      # noqa: E731
        _cases = {"two-box": c(source), "tight": c(source, 0.03), "outliers": c(np.concatenate((source, far))), "subset": c(subset),
                  "none": c(far), "init": c(source, init=G)}
    return _cases


_results = {}


def reference(name):
    """``icp`` of a case, computed once."""
    if name not in _results:
        k = cases()[name]
        _results[name] = icp(k["source"], k["target"], k["threshold"], k["init"])
    return _results[name]
