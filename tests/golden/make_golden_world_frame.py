"""Generates tests/golden/world_frame_reference.npz: the cases of make_golden.py (same scenes, same recorded arrays) at a
NON-IDENTITY first-frame matrix, by running the REFERENCE's own Python on CPU exactly as make_golden.py does.

Everything make_golden.py records is recorded with ``w2c = I``: row 2 of the matrix equals its column 2, its translation
is zero and the view matrix equals its transpose, so a mirror that confused any of these would reproduce those vectors.
Here

  * the camera is ``setup_camera(W, H, k, M)`` of /root/reference/utils/recon_helpers.py and ``curr_data['w2c'] = M``
    (cases ``iso_M``, ``aniso_M``) for a GENERAL rigid M: 0.35 rad about (1, 2, 3) -- every off-diagonal pair of R differs
    by more than 0.05, so no transposition of any pair goes unseen -- and three distinct non-zero translation components;
  * in ``iso_M2`` the camera is built from M while ``curr_data['w2c'] = M2 != M``, as the reference's post-optimisation
    scripts call it (/root/reference/scripts/post_splatam_opt.py:275,307): the depth channel and the camera disagree;
  * the map of make_scene is moved by M^-1 (centres only), so that it still fills the frame.

The file is written with fixed zip timestamps: running the generator twice gives the same bytes.

Run:  python tests/golden/make_golden_world_frame.py     (needs /root/reference; not needed on the GPU box)
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as base  # noqa: E402  (installs the device shim, puts the repository and /root/reference on sys.path)

from oracle import raster_ref as R  # noqa: E402
from utils import recon_helpers as ref_recon  # noqa: E402
from utils import slam_external as ref_ext  # noqa: E402
from utils import slam_helpers as ref_h  # noqa: E402


def rigid(angle, axis, t):
    """float32 4x4 world-to-camera: rotation by ``angle`` (rad) about ``axis`` (Rodrigues, formed in float64), translation ``t``."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    M[:3, 3] = t
    return M.astype(np.float32)


M_FIRST = rigid(0.35, (1.0, 2.0, 3.0), (0.1, -0.07, 0.2))
M_OTHER = rigid(0.25, (-2.0, 1.0, 1.5), (-0.06, 0.12, 0.15))


def check_general(M):
    """The conditions that make M tell a row from a column, a matrix from its transpose and a dropped translation."""
    Rm, t = M[:3, :3].astype(np.float64), M[:3, 3].astype(np.float64)
    assert np.arccos((np.trace(Rm) - 1) / 2) >= 0.2
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert abs(Rm[i, j] - Rm[j, i]) >= 0.05, (i, j, Rm[i, j], Rm[j, i])
    assert (np.abs(t) >= 0.05).all() and len({round(abs(float(x)), 3) for x in t}) == 3, t


def run_case(name, n, W, H, f, anisotropic, seed, M_cam, M_curr, out):
    params, (W, H, f, cx, cy) = base.make_scene(n, W, H, f, anisotropic, seed)
    c2w = np.linalg.inv(M_cam.astype(np.float64))
    params['means3D'] = (params['means3D'].double() @ torch.tensor(c2w[:3, :3].T) + torch.tensor(c2w[:3, 3])).float()
    for k, v in params.items():
        out[f"{name}/param/{k}"] = v.numpy()
    k_mat = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], dtype=np.float32)
    cam = ref_recon.setup_camera(W, H, k_mat, M_cam)
    w2c = torch.tensor(M_curr)
    out[f"{name}/meta"] = np.array([n, W, H, f, cx, cy], dtype=np.float64)
    out[f"{name}/w2c_cam"], out[f"{name}/w2c_curr"] = M_cam, M_curr
    out[f"{name}/cam/viewmatrix"] = cam.viewmatrix.numpy()
    out[f"{name}/cam/projmatrix"] = cam.projmatrix.numpy()
    out[f"{name}/cam/campos"] = cam.campos.numpy()
    out[f"{name}/cam/tanfov"] = np.array([cam.tanfovx, cam.tanfovy], dtype=np.float64)
    time_idx = 1

    # (1) helper functions
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    tg = ref_h.transform_to_frame(P, time_idx, gaussians_grad=True, camera_grad=True)
    dv = ref_h.transformed_params2depthplussilhouette(P, w2c, tg)
    out[f"{name}/tg/means3D"] = tg['means3D'].detach().numpy()
    out[f"{name}/dv/colors_precomp"] = dv['colors_precomp'].detach().numpy()

    # (2) ground truth frame (a render from a perturbed pose) and both loss modes
    with torch.no_grad():
        P2 = {k: v.clone() for k, v in params.items()}
        P2['cam_trans'][..., time_idx] += torch.tensor([[0.01, -0.005, 0.005]])
        tg2 = ref_h.transform_to_frame(P2, time_idx, False, False)
        gt_im, radii, _ = R.OracleRasterizer(cam)(**ref_h.transformed_params2rendervar(P2, tg2))
        ds, _, _ = R.OracleRasterizer(cam)(**ref_h.transformed_params2depthplussilhouette(P2, w2c, tg2))
        gt_depth = torch.where(ds[1:2] > 0.5, ds[0:1] / ds[1:2].clamp_min(1e-6), torch.zeros_like(ds[0:1]))
    out[f"{name}/gt_im"] = gt_im.numpy()
    out[f"{name}/gt_depth"] = gt_depth.numpy()
    visible, covered = int((radii > 0).sum()), float((ds[1] > 0.5).float().mean())
    print(f"{name}: {visible} of {n} Gaussians visible, {100 * covered:.0f} % of the pixels have silhouette > 0.5")
    assert visible >= 0.9 * n and covered >= 0.8, "the moved map does not fill the frame"

    get_loss = base.reference_get_loss()
    for mode in ("tracking", "mapping"):
        P = {k: torch.nn.Parameter(v.clone()) for k, v in params.items()}
        variables = {'max_2D_radius': torch.zeros(n), 'means2D_gradient_accum': torch.zeros(n), 'denom': torch.zeros(n),
                     'timestep': torch.zeros(n)}
        curr = {'cam': cam, 'im': gt_im, 'depth': gt_depth, 'id': time_idx, 'w2c': w2c}
        kw = dict(tracking=True) if mode == "tracking" else dict(mapping=True)
        loss, variables, wl = get_loss(P, curr, variables, time_idx, dict(im=0.5, depth=1.0),
                                       mode == "tracking", 0.99 if mode == "tracking" else 0.5, True, False, **kw)
        loss.backward()
        out[f"{name}/{mode}/loss"] = np.array([loss.item(), wl['im'].item(), wl['depth'].item()])
        for k, v in P.items():
            out[f"{name}/{mode}/grad/{k}"] = (torch.zeros_like(v) if v.grad is None else v.grad).numpy()
        out[f"{name}/{mode}/max_2D_radius"] = variables['max_2D_radius'].numpy()
        out[f"{name}/{mode}/means2D_grad"] = variables['means2D'].grad.numpy()


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    check_general(M_FIRST)
    check_general(M_OTHER)
    assert np.abs(M_FIRST - M_OTHER).max() > 0.05
    out = {}
    run_case("iso_M", 1500, 96, 64, 80.0, False, 0, M_FIRST, M_FIRST, out)
    run_case("aniso_M", 1200, 80, 64, 70.0, True, 1, M_FIRST, M_FIRST, out)
    run_case("iso_M2", 1500, 96, 64, 80.0, False, 0, M_FIRST, M_OTHER, out)
    # iso_M2 is iso_M with another curr_data['w2c']: what the two share is stored once
    for key in [k for k in out if k.startswith("iso_M2/")]:
        twin = "iso_M/" + key[len("iso_M2/"):]
        if "/param/" in key or "/cam/" in key or key.endswith(("/meta", "/gt_im", "/tg/means3D", "/w2c_cam")):
            assert np.array_equal(out[key], out[twin]), key
            del out[key]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "world_frame_reference.npz")
    save_deterministic(path, out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", len(out), "arrays")
