"""The host-side mirror (splatam_amd/slam.py) against golden vectors produced by
the REFERENCE's own Python (tests/golden/make_golden.py, run where /root/reference
exists).  CPU only; the rasterizer inside get_loss is the oracle here, exactly as
it was when the fixture was generated."""
import os

import numpy as np
import pytest
import torch

from oracle import raster_ref as R
from splatam_amd import slam

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slam_reference.npz"))
PARAM_KEYS = ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales', 'cam_unnorm_rots', 'cam_trans')


def _params(name, grad=False):
    return {k: torch.tensor(GOLD[f"{name}/param/{k}"]).requires_grad_(grad) for k in PARAM_KEYS}


@pytest.mark.parametrize("name", ["iso", "aniso"])
def test_render_variable_assembly(name):
    P = _params(name)
    tg = slam.transform_to_frame(P, 1, gaussians_grad=True, camera_grad=True)
    np.testing.assert_allclose(tg['means3D'].numpy(), GOLD[f"{name}/tg/means3D"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(tg['unnorm_rotations'].numpy(), GOLD[f"{name}/tg/unnorm_rotations"], rtol=1e-5, atol=1e-6)
    rv = slam.transformed_params2rendervar(P, tg)
    for k in ('rotations', 'opacities', 'scales', 'colors_precomp'):
        np.testing.assert_allclose(rv[k].detach().numpy(), GOLD[f"{name}/rv/{k}"], rtol=1e-5, atol=1e-6)
    assert rv['means2D'].shape == P['means3D'].shape and not rv['means2D'].is_leaf
    dv = slam.transformed_params2depthplussilhouette(P, torch.eye(4), tg)
    np.testing.assert_allclose(dv['colors_precomp'].numpy(), GOLD[f"{name}/dv/colors_precomp"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(slam.build_rotation(P['cam_unnorm_rots'][..., 1]).numpy(), GOLD[f"{name}/build_rotation"],
                               rtol=1e-6, atol=1e-7)


def test_detach_wiring():
    P = _params("iso", grad=True)
    tg = slam.transform_to_frame(P, 1, gaussians_grad=False, camera_grad=True)
    tg['means3D'].sum().backward()
    assert P['means3D'].grad is None and P['cam_trans'].grad is not None and P['cam_unnorm_rots'].grad is not None
    P = _params("iso", grad=True)
    tg = slam.transform_to_frame(P, 1, gaussians_grad=True, camera_grad=False)
    tg['means3D'].sum().backward()
    assert P['means3D'].grad is not None and P['cam_trans'].grad is None


def test_ssim_and_camera():
    gt = torch.tensor(GOLD["iso/gt_im"])
    assert abs(slam.calc_ssim(gt, gt * 0.9 + 0.02).item() - float(GOLD["iso/ssim"])) < 1e-6
    n, W, H, f, cx, cy = GOLD["iso/meta"]
    W, H = int(W), int(H)
    k = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    cam = slam.setup_camera(W, H, k, np.eye(4), device="cpu")
    ref = R.make_camera(W, H, f, f, cx, cy)
    assert cam.image_height == H and cam.image_width == W and len(cam) == 11
    assert abs(cam.tanfovx - ref.tanfovx) < 1e-9 and abs(cam.tanfovy - ref.tanfovy) < 1e-9
    assert torch.allclose(cam.viewmatrix, ref.viewmatrix) and torch.allclose(cam.projmatrix, ref.projmatrix)
    assert not cam.viewmatrix.is_contiguous() or cam.viewmatrix.shape == (1, 4, 4)


@pytest.mark.parametrize("name", ["iso", "aniso"])
@pytest.mark.parametrize("mode", ["tracking", "mapping"])
def test_get_loss_matches_reference_code(monkeypatch, name, mode):
    monkeypatch.setattr(slam, "Renderer", R.OracleRasterizer)
    n, W, H, f, cx, cy = GOLD[f"{name}/meta"]
    n, W, H = int(n), int(W), int(H)
    cam = R.make_camera(W, H, f, f, cx, cy)
    P = {k: torch.nn.Parameter(torch.tensor(GOLD[f"{name}/param/{k}"])) for k in PARAM_KEYS}
    variables = {'max_2D_radius': torch.zeros(n), 'means2D_gradient_accum': torch.zeros(n), 'denom': torch.zeros(n),
                 'timestep': torch.zeros(n)}
    curr = {'cam': cam, 'im': torch.tensor(GOLD[f"{name}/gt_im"]), 'depth': torch.tensor(GOLD[f"{name}/gt_depth"]),
            'id': 1, 'w2c': torch.eye(4)}
    cfg = slam.REPLICA_TRACKING if mode == "tracking" else slam.REPLICA_MAPPING
    loss, variables, wl = slam.get_loss(P, curr, variables, 1, cfg['loss_weights'], cfg['use_sil_for_loss'],
                                        cfg['sil_thres'], cfg['use_l1'], cfg['ignore_outlier_depth_loss'],
                                        tracking=mode == "tracking", mapping=mode == "mapping")
    loss.backward()
    want = GOLD[f"{name}/{mode}/loss"]
    got = np.array([loss.item(), wl['im'].item(), wl['depth'].item()])
    np.testing.assert_allclose(got, want, rtol=2e-5)
    for k in PARAM_KEYS:
        ref = GOLD[f"{name}/{mode}/grad/{k}"]
        g = torch.zeros_like(P[k]) if P[k].grad is None else P[k].grad
        scale = np.abs(ref).max() + 1e-20
        assert np.abs(g.numpy() - ref).max() <= 2e-4 * scale + 1e-12, (k, np.abs(g.numpy() - ref).max(), scale)
    np.testing.assert_array_equal(variables['max_2D_radius'].numpy(), GOLD[f"{name}/{mode}/max_2D_radius"])
    ref = GOLD[f"{name}/{mode}/means2D_grad"]
    assert np.abs(variables['means2D'].grad.numpy() - ref).max() <= 2e-4 * (np.abs(ref).max() + 1e-20)


@pytest.mark.parametrize("mode", ["tracking", "mapping"])
def test_mirror_get_loss_makes_the_reference_call_sequence(mode, monkeypatch):
    """splatam_amd.slam.get_loss against the recording of the REFERENCE's get_loss at the rasterizer boundary
    (tests/golden/caller_reference.npz): same kwargs into both Renderer calls, same loss, same gradient planes back."""
    from oracle import c_ref
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_reference.npz"))
    n, W, H = (int(x) for x in gold["meta"][:3])
    f, cx, cy = (float(x) for x in gold["meta"][3:6])
    calls = []

    class Rec:
        def __init__(self, raster_settings):
            self.inner = c_ref.CRasterizer(raster_settings)

        def __call__(self, **kw):
            out = self.inner(**kw)
            out[0].retain_grad()
            calls.append((kw, out))
            return out
    monkeypatch.setattr(slam, "Renderer", Rec)
    params = {k[len("param/"):]: torch.nn.Parameter(torch.tensor(gold[k])) for k in gold.files if k.startswith("param/")}
    cam = slam.setup_camera(W, H, [[f, 0, cx], [0, f, cy], [0, 0, 1]], np.eye(4, dtype=np.float32), device="cpu")
    for fld in ("viewmatrix", "projmatrix"):
        assert np.array_equal(getattr(cam, fld).numpy(), gold[f"cam/{fld}"])
    variables = {'max_2D_radius': torch.zeros(n), 'means2D_gradient_accum': torch.zeros(n), 'denom': torch.zeros(n), 'timestep': torch.zeros(n)}
    curr = {'cam': cam, 'im': torch.tensor(gold["gt_im"]), 'depth': torch.tensor(gold["gt_depth"]), 'id': 1, 'w2c': torch.eye(4)}
    tracking = mode == "tracking"
    loss, variables, _ = slam.get_loss(params, curr, variables, 1, dict(im=0.5, depth=1.0), tracking, 0.99 if tracking else 0.5, True, False,
                                       tracking=tracking, mapping=not tracking)
    loss.backward()
    assert len(calls) == 2
    for ci, (kw, out) in enumerate(calls):
        assert set(kw) == {'means3D', 'colors_precomp', 'rotations', 'opacities', 'scales', 'means2D'}
        for k, v in kw.items():
            ref = gold[f"call{ci}/in/{k}"] if f"call{ci}/in/{k}" in gold.files else gold[f"call0/in/{k}"]
            np.testing.assert_allclose(v.detach().numpy(), ref, rtol=2e-6, atol=1e-7, err_msg=f"call {ci} {k}")
        g = out[0].grad if out[0].grad is not None else torch.zeros_like(out[0])
        ref = gold[f"{mode}/call{ci}/grad_out/color"]
        # the planes agree except where a loss term sits on a kink (|gt - render| ~ 0, a mask edge): a handful of pixels
        bad = np.abs(g.numpy() - ref) > 1e-6 * max(1.0, np.abs(ref).max())
        assert bad.mean() < 2e-4, (ci, bad.sum())
    assert abs(float(loss) - float(gold[f"{mode}/loss"])) <= 1e-5 * abs(float(gold[f"{mode}/loss"]))
    assert variables['means2D'] is calls[0][0]['means2D'] and variables['means2D'].grad is not None
    assert np.array_equal(variables['seen'].numpy(), gold[f"{mode}/seen"])
    assert np.array_equal(variables['max_2D_radius'].numpy(), gold[f"{mode}/max_2D_radius"])


# ---------------------------------------------------------------------------------------------------------------------
# a NON-IDENTITY first-frame matrix (tests/golden/make_golden_world_frame.py): with w2c = I row 2 of the matrix equals its
# column 2, its translation is zero and the view matrix equals its transpose -- the cases above cannot tell those apart
# ---------------------------------------------------------------------------------------------------------------------
WORLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_frame_reference.npz"))
WORLD_SHARED = {"iso_M2": "iso_M"}          # iso_M2 is iso_M with another curr_data['w2c']; what they share is stored once


def _world(name, key):
    full = f"{name}/{key}"
    return WORLD[full] if full in WORLD.files else WORLD[f"{WORLD_SHARED[name]}/{key}"]


def _world_camera(name):
    n, W, H, f, cx, cy = _world(name, "meta")
    W, H = int(W), int(H)
    k = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], dtype=np.float32)
    return int(n), W, H, slam.setup_camera(W, H, k, _world(name, "w2c_cam"), device="cpu")


def _misses_by(got, want, rtol, atol=0.0):
    """Largest |got - want| in units of the tolerance atol + rtol |want| a correct evaluation has to meet."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def _wrong_matrices(M):
    """What a reader of the matrix gets wrong without the identity noticing: a column for the row, a dropped translation."""
    no_t = M.copy()
    no_t[:3, 3] = 0.0
    return {"transposed": np.ascontiguousarray(M.T), "translation dropped": no_t}


def test_world_frame_matrices_are_general():
    """The fixture's matrices keep what makes them worth having: a rotation of at least 0.2 rad whose every off-diagonal pair
    differs by at least 0.05, three distinct translation components of at least 0.05; camera and depth matrix differ in iso_M2."""
    for M in (WORLD["iso_M/w2c_cam"], WORLD["aniso_M/w2c_cam"], WORLD["iso_M2/w2c_curr"]):
        Rm, t = M[:3, :3].astype(np.float64), M[:3, 3].astype(np.float64)
        np.testing.assert_allclose(Rm @ Rm.T, np.eye(3), atol=1e-6)
        assert np.arccos((np.trace(Rm) - 1) / 2) >= 0.2
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert abs(Rm[i, j] - Rm[j, i]) >= 0.05
        assert (np.abs(t) >= 0.05).all() and len({round(abs(float(x)), 3) for x in t}) == 3
    assert np.array_equal(WORLD["iso_M/w2c_cam"], WORLD["iso_M/w2c_curr"])
    assert np.abs(WORLD["iso_M2/w2c_curr"] - WORLD["iso_M/w2c_cam"]).max() > 0.05


@pytest.mark.parametrize("name", ["iso_M", "aniso_M"])
def test_setup_camera_at_a_general_pose(name):
    """slam.setup_camera against the settings tuple the reference's own setup_camera built from M."""
    n, W, H, cam = _world_camera(name)
    assert cam.image_height == H and cam.image_width == W and len(cam) == 11
    view, proj = _world(name, "cam/viewmatrix"), _world(name, "cam/projmatrix")
    assert cam.viewmatrix.shape == view.shape == (1, 4, 4) and cam.projmatrix.shape == proj.shape
    np.testing.assert_allclose(cam.viewmatrix.numpy(), view, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cam.projmatrix.numpy(), proj, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cam.campos.numpy(), _world(name, "cam/campos"), rtol=1e-6, atol=1e-7)
    # (the reference divides by the float32 entries of k in float32: its tangents carry float32 rounding)
    np.testing.assert_allclose([cam.tanfovx, cam.tanfovy], _world(name, "cam/tanfov"), rtol=2.0 ** -23)
    # the stored view matrix is the TRANSPOSE of the row-major M (column-major as the kernels read it), and M is far from symmetric
    assert np.array_equal(view[0], _world(name, "w2c_cam").T)
    assert np.abs(view[0] - view[0].T).max() >= 0.05


@pytest.mark.parametrize("name", ["iso_M", "aniso_M", "iso_M2"])
def test_depth_channel_at_a_general_pose(name):
    """transformed_params2depthplussilhouette with curr_data['w2c'] = M (iso_M2: a matrix other than the camera's) against the
    reference's; the same call with a column for the row or the translation dropped misses by >= 100x the tolerance."""
    P = {k: torch.tensor(_world(name, f"param/{k}")) for k in PARAM_KEYS}
    tg = slam.transform_to_frame(P, 1, gaussians_grad=True, camera_grad=True)
    np.testing.assert_allclose(tg['means3D'].numpy(), _world(name, "tg/means3D"), rtol=1e-5, atol=1e-6)
    M = _world(name, "w2c_curr")
    want = _world(name, "dv/colors_precomp")
    dv = slam.transformed_params2depthplussilhouette(P, torch.tensor(M), tg)
    np.testing.assert_allclose(dv['colors_precomp'].numpy(), want, rtol=1e-5, atol=1e-6)
    for what, wrong in _wrong_matrices(M).items():
        got = slam.transformed_params2depthplussilhouette(P, torch.tensor(wrong), tg)['colors_precomp'].numpy()
        miss = _misses_by(got, want, 1e-5, 1e-6)
        print(f"{name}: depth channel with the matrix {what} misses the reference by {miss:.3g}x the tolerance")
        assert miss >= 100.0, (name, what, miss)


def _world_get_loss(name, mode, w2c, monkeypatch):
    monkeypatch.setattr(slam, "Renderer", R.OracleRasterizer)
    n, W, H, cam = _world_camera(name)
    P = {k: torch.nn.Parameter(torch.tensor(_world(name, f"param/{k}"))) for k in PARAM_KEYS}
    variables = {'max_2D_radius': torch.zeros(n), 'means2D_gradient_accum': torch.zeros(n), 'denom': torch.zeros(n),
                 'timestep': torch.zeros(n)}
    curr = {'cam': cam, 'im': torch.tensor(_world(name, "gt_im")), 'depth': torch.tensor(_world(name, "gt_depth")),
            'id': 1, 'w2c': torch.tensor(w2c)}
    cfg = slam.REPLICA_TRACKING if mode == "tracking" else slam.REPLICA_MAPPING
    loss, variables, wl = slam.get_loss(P, curr, variables, 1, cfg['loss_weights'], cfg['use_sil_for_loss'],
                                        cfg['sil_thres'], cfg['use_l1'], cfg['ignore_outlier_depth_loss'],
                                        tracking=mode == "tracking", mapping=mode == "mapping")
    return P, variables, loss, np.array([loss.item(), wl['im'].item(), wl['depth'].item()])


@pytest.mark.parametrize("name", ["iso_M", "aniso_M", "iso_M2"])
@pytest.mark.parametrize("mode", ["tracking", "mapping"])
def test_get_loss_matches_reference_code_at_a_general_pose(monkeypatch, name, mode):
    """get_loss with the camera of setup_camera(M) and curr_data['w2c'] = M (iso_M2: M2 != M) against the reference's get_loss;
    tolerances of test_get_loss_matches_reference_code."""
    M = _world(name, "w2c_curr")
    P, variables, loss, got = _world_get_loss(name, mode, M, monkeypatch)
    loss.backward()
    want = _world(name, f"{mode}/loss")
    np.testing.assert_allclose(got, want, rtol=2e-5)
    for k in PARAM_KEYS:
        ref = _world(name, f"{mode}/grad/{k}")
        g = torch.zeros_like(P[k]) if P[k].grad is None else P[k].grad
        scale = np.abs(ref).max() + 1e-20
        assert np.abs(g.numpy() - ref).max() <= 2e-4 * scale + 1e-12, (k, np.abs(g.numpy() - ref).max(), scale)
    moved = [k for k in (('cam_unnorm_rots', 'cam_trans') if mode == "tracking" else ('means3D', 'log_scales'))
             if np.abs(_world(name, f"{mode}/grad/{k}")).max() > 0]
    assert moved, "the case has no gradient to compare"
    np.testing.assert_array_equal(variables['max_2D_radius'].numpy(), _world(name, f"{mode}/max_2D_radius"))
    ref = _world(name, f"{mode}/means2D_grad")
    assert np.abs(variables['means2D'].grad.numpy() - ref).max() <= 2e-4 * (np.abs(ref).max() + 1e-20)


@pytest.mark.parametrize("name", ["iso_M", "aniso_M"])
@pytest.mark.parametrize("mode", ["tracking", "mapping"])
def test_get_loss_at_a_general_pose_tells_a_wrong_matrix(monkeypatch, name, mode):
    """Sensitivity of the case above: with M.T for the depth channel, or M without its translation, the mirror misses the
    reference's loss by at least 100x the 2e-5 the right matrix has to meet."""
    M = _world(name, "w2c_curr")
    want = _world(name, f"{mode}/loss")
    for what, wrong in _wrong_matrices(M).items():
        got = _world_get_loss(name, mode, wrong, monkeypatch)[3]
        miss = _misses_by(got[0], want[0], 2e-5)
        print(f"{name} {mode}: loss with the matrix {what} is {got[0]:.6g} for {want[0]:.6g}: {miss:.3g}x the tolerance")
        assert miss >= 100.0, (name, mode, what, got, want)
