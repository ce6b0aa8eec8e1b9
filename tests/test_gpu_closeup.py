"""Close, frame-filling splats (tests/closeup_cases.py: the walk-through scene) through the drop-in rasterizer and the fused engine,
against the C oracle: the guard-band clamp of the projection (splat_math.h ewa_setup: clamped tx / ty, xmul / ymul; the masked
dtx / dty of project_gaussian_backward), tile rectangles that overshoot the grid on every side (clampi), the live-rectangle cull
(live_tile_rect) and the 4 x 4-block cull of the composites (render.hip gather()) on splats whose centre lies hundreds of pixels
outside the frame, and the near plane.

Gradients are bounded per GROUP of rows (clamped in x / y / both, near, wider than the frame, plain) by 1e-3 of the group's own
maximum, on top of the checks of tests/test_gpu_parity.py; tests/test_closeup_cases_cpu.py shows on the CPU that the groups are
populated, that the reference alone stays within every bound used here, and that the bound catches a dropped mask, a dropped
clamp and a moved near plane.  Every test asserts which path it took."""
import numpy as np
import pytest
import torch

from oracle import raster_ref as R
from tests import closeup_cases as cc
from tests.test_gpu_configs import _check_pose_gradient, _fused_stages
from tests.test_gpu_parity import GRAD_MAP, _c_oracle, _check_forward, _check_grads, _gpu_render, _to_cuda_settings
from tests.util import assert_close_outliers, assert_grad_calibrated, grad_scale

pytestmark = pytest.mark.gpu

CELL_IDS = [f"{c[0]}-{'aniso' if c[5] else 'iso'}" for c in cc.CELLS]


def _flagged_before():
    from splatam_amd import rasterizer as rz
    return rz.fast_path_stats["flagged"]


def _assert_behind_untouched(gr, gg, groups):
    behind = groups['behind']
    assert (gr[behind] == 0).all()
    for k, g in gg.items():
        assert float(np.abs(g.reshape(g.shape[0], -1)[behind]).max()) == 0.0, k


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
@pytest.mark.parametrize("path", ["exact", "fast", "exact + staged records", "fast + staged records"])
def test_closeup_forward_backward_parity(cell, path):
    """test_forward_backward_parity of tests/test_gpu_parity.py on the walk-through scene, plus the group-wise gradient bound and
    exact zeros behind the near plane."""
    from splatam_amd import rasterizer as rz
    ref = cc.closeup_reference(*cell)
    cam, rv, groups, gout = ref['cam'], ref['rv'], ref['groups'], ref['gout']
    W, H = cell[1], cell[2]
    if path.endswith("staged records"):
        rz.USE_TILE_RECS = True
        path = path.split(" ")[0]
    flagged = _flagged_before()
    gc, gr, gd, gg = _gpu_render(cam, rv, gout, path=path)          # (asserts that the call under test took ``path``)
    rz.check_pending()
    assert rz.fast_path_stats["flagged"] == flagged
    oc, orad, od, og, _ = ref['f32']
    _, rad64, _, og64, cr64 = ref['f64']
    flips = _check_forward(gc, gr, gd, oc, orad, od, W * H, cam, rv)
    _check_grads(gg, og, og64, flips)
    rows_ok = cc.rows_clear_of(flips[0], cr64.geom(), rad64)
    print(f"{int(flips[0].sum())} pixels with a decision flip; {int((~rows_ok).sum())} rows blend at one of them")
    for k, ok in GRAD_MAP:
        cc.assert_groupwise(gg[k].reshape(og64[ok].shape), og64[ok], groups, rows_ok, what=f"{path} grad {k}")
    _assert_behind_untouched(gr, gg, groups)


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
def test_closeup_fast_path_equals_exact_path(cell):
    """The live-rectangle cull of group binning and the block cull of the composites on off-screen centres: whatever they drop blends
    nowhere, so the fast path's image is the exact path's BIT FOR BIT, the gradients agree to float-atomic order (the 2e-4 of
    test_culls_drop_nothing_on_extreme_splats) and the radii are the oracle's."""
    from splatam_amd import rasterizer as rz
    ref = cc.closeup_reference(*cell)
    cam, rv, gout = ref['cam'], ref['rv'], ref['gout']
    flagged = _flagged_before()
    ec, er, ed, eg = _gpu_render(cam, rv, gout, path="exact")
    fc, fr, fd, fg = _gpu_render(cam, rv, gout, path="fast")
    rz.check_pending()
    assert rz.fast_path_stats["flagged"] == flagged
    assert np.array_equal(er, fr) and np.array_equal(er, ref['f32'][1])
    assert np.array_equal(ec, fc) and np.array_equal(ed, fd), (np.abs(ec - fc).max(), np.abs(ed - fd).max())
    for k in eg:
        print(f"grad {k}: fast - exact {np.abs(eg[k] - fg[k]).max() / grad_scale(eg[k]):.2e} of the maximum")
        assert np.abs(eg[k] - fg[k]).max() <= 2e-4 * grad_scale(eg[k]) + 1e-12, k
    _assert_behind_untouched(fr, fg, ref['groups'])


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
def test_closeup_internal_state_matches_oracle(cell):
    """test_internal_state_matches_oracle on rectangles clamped on up to four sides: instance count, tile ranges and sorted lists
    exactly the oracle's."""
    from splatam_amd import rasterizer as rz
    ref = cc.closeup_reference(*cell)
    cam, rv = ref['cam'], ref['rv']
    cs = _to_cuda_settings(cam)
    empty = torch.empty(0, device="cuda")
    before = dict(rz.fast_path_stats)
    col, radii, dep, pk = rz.rasterize_forward(cs, rv['means3D'].cuda(), rv['colors_precomp'].cuda(), rv['opacities'].cuda().reshape(-1),
                                               rv['scales'].cuda(), rv['rotations'].cuda(), empty, empty)
    torch.cuda.synchronize()
    assert rz.fast_path_stats["exact"] == before["exact"] + 1 and rz.fast_path_stats["fast"] == before["fast"]
    _, orad, _, _, cr = ref['f32']
    rect = np.diff(cr.ranges())
    assert (rect > 0).all()                             # every tile holds a list: the wide splats reach all of them
    assert pk.num_rendered == cr.num_rendered()
    assert (pk.tensors['tile_base'].cpu().numpy() == cr.ranges()).all()
    assert (pk.tensors['point_list'].cpu().numpy()[:pk.num_rendered] == cr.point_list()).all()
    assert (radii.cpu().numpy() == orad).all()
    ncg, nco = pk.tensors['n_contrib'].cpu().numpy(), cr.n_contrib()
    assert (ncg != nco).sum() <= 3
    assert_close_outliers(pk.tensors['final_T'].cpu().numpy(), cr.final_T(), 1e-5, max_outlier_frac=1e-4, outlier_atol=0.02, what="final_T")


@pytest.mark.parametrize("path", ["exact", "fast"])
def test_near_plane_boundary(path):
    """Three Gaussians on the optical axis at z = float32(0.2), one step above and one step below: the near-plane test is z > 0.2 on
    the float32 value, so only the second is rendered -- radii (0, positive, 0) as the oracle's, the same image, the same markVisible."""
    from diff_gaussian_rasterization import GaussianRasterizer as Renderer
    W, H = 33, 17
    cam = R.make_camera(W, H, 40.0, 40.0, W / 2.0, H / 2.0)
    near = np.float32(0.2)
    zs = [float(near), float(np.nextafter(near, np.float32(1))), float(np.nextafter(near, np.float32(0)))]
    rv = dict(means3D=torch.tensor([[0.0, 0.0, z] for z in zs]), means2D=torch.zeros(3, 3), opacities=torch.full((3, 1), 0.7),
              colors_precomp=torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]), scales=torch.full((3, 3), 0.01),
              rotations=torch.tensor([[1.0, 0, 0, 0]] * 3))
    gc, gr, gd, _ = _gpu_render(cam, rv, path=path)
    oc, orad, od, _, _ = _c_oracle(cam, rv)
    assert orad[0] == 0 and orad[1] > 0 and orad[2] == 0, orad
    assert np.array_equal(gr, orad), (gr, orad)
    assert oc[2].max() > 0.5 and oc[0].max() == 0.0 and oc[1].max() == 0.0                  # (the image is the second Gaussian's alone)
    assert np.abs(gc - oc).max() <= 1e-6 and np.abs(gd - od).max() <= 1e-6, (np.abs(gc - oc).max(), np.abs(gd - od).max())
    m = Renderer(raster_settings=_to_cuda_settings(cam)).markVisible(rv['means3D'].cuda()).cpu()
    assert m.tolist() == R.mark_visible(rv['means3D'], cam).tolist() == [False, True, False]


# -------------------------------------------------------------------------------------------------------------------------------
# the fused engine on the same map, at the walk-through pose
# -------------------------------------------------------------------------------------------------------------------------------

ENGINE_KEYS = ("means3D", "rgb_colors", "logit_opacities", "log_scales", "unnorm_rotations")
TRACKING_KEYS = ("rgb_colors", "logit_opacities", "log_scales")


def _engine_groups(params, cam_args, c, monkeypatch):
    """The row groups of the engine case, from the float64 oracle of its colour render (float64 glue) and its float64 centres."""
    from splatam_amd import slam
    from oracle import c_ref
    monkeypatch.setattr(slam, "Renderer", c_ref.CRasterizer)
    W, H, k = cam_args
    pc = {k_: v.detach().cpu().double() for k_, v in params.items()}
    cam_c = slam.setup_camera(W, H, k, np.eye(4, dtype=np.float32), device="cpu")
    with torch.no_grad():
        tg = slam.transform_to_frame(pc, 1, gaussians_grad=False, camera_grad=False)
        _, radii, _ = slam.Renderer(raster_settings=cam_c)(**slam.transformed_params2rendervar(pc, tg))
    return radii.numpy(), cam_c


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
@pytest.mark.parametrize("tracking", [False, True], ids=["mapping", "tracking"])
def test_closeup_fused_engine_vs_oracle(cell, tracking, monkeypatch):
    """One iteration at the walk-through pose (REPLICA_MAPPING / REPLICA_TRACKING), staged (A)..(D) against the C oracle as in
    tests/test_gpu_configs.py, once on exact lists and once on learnt buckets with group binning (whose live-rectangle cull files
    the off-screen splats): the calibrated check per tensor and the group-wise bound (mapping: all five tensors; tracking: the
    pose gradient, then colours, opacities and scales of the tracking iteration that forms the map's gradients too); the bucketed
    iteration equals the exact one to the float-atomic spread of test_group_binning_changes_nothing_but_speed."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    n, W, H, f, seed, aniso = cell
    params, variables, frame, cam, k, c = cc.closeup_engine_case(*cell)
    cfg = slam.REPLICA_TRACKING if tracking else slam.REPLICA_MAPPING
    radii64, _ = _engine_groups(params, (W, H, k), c, monkeypatch)
    tv = cc.engine_view_centres(params)
    outs = []
    for buckets in (False, True):
        p = {k_: torch.nn.Parameter(v.detach().clone()) for k_, v in params.items()}
        eng = FusedEngine(p, cam)
        eng.allow_buckets = buckets
        for _ in range(4):
            eng.loss_backward(frame, 1, cfg, tracking=tracking)
            if not eng.check_overflow():
                break
        else:
            raise AssertionError("the lists could not be sized")
        assert (eng.tile_stride > 0) == buckets and eng.max_list_hint > 0
        eng.loss_backward(frame, 1, cfg, tracking=tracking)                  # the iteration under test: the second one
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        assert (eng._workspace(False, with_ssim=False).st.group_stride > 0) == buckets
        what = f"fused close-up {'aniso' if aniso else 'iso'} {'tracking' if tracking else 'mapping'} on {'buckets + group binning' if buckets else 'exact lists'}"
        g32, g64 = _fused_stages(eng, p, variables, frame, (W, H, k), c, cfg, tracking, what, monkeypatch)
        if tracking:
            _check_pose_gradient(eng, g32, g64, what)
            grads = eng.buf['d_cam'][:7].clone()
            # ... and the tracking iteration that also forms the map's gradients: same planes, hence the same oracle gradients (with
            # the Gaussians detached from the pose the oracle has them for colours, opacities and scales)
            out6, planes = eng.buf['out6'].clone(), eng.buf['dL_dout6'].clone()
            eng.loss_backward(frame, 1, cfg, tracking=True, map_grads=True)
            torch.cuda.synchronize()
            assert not eng.check_overflow(grow=False)
            assert torch.equal(eng.buf['out6'], out6) and torch.equal(eng.buf['dL_dout6'], planes)
            groups = cc.row_groups(tv, radii64, [g64[key] for key in TRACKING_KEYS], W, cam.tanfovx, cam.tanfovy)
            print(what, {g: int(m.sum()) for g, m in groups.items()})
            for key in TRACKING_KEYS:
                got = eng.grads[key].cpu().numpy()
                assert_grad_calibrated(got, g32[key], g64[key], what=f"{what} grad {key}")
                cc.assert_groupwise(got, g64[key], groups, what=f"{what} grad {key}")
                assert float(np.abs(got[groups['behind']]).max()) == 0.0, key
        else:
            groups = cc.row_groups(tv, radii64, [g64[key] for key in ENGINE_KEYS], W, cam.tanfovx, cam.tanfovy)
            print(what, {g: int(m.sum()) for g, m in groups.items()})
            for g, least in cc.MIN_ROWS.items():
                assert int(groups[g].sum()) >= least, (g, int(groups[g].sum()))
            tail = 2.0 if eng.depth_tie_pixels == 0 else 3.0
            for key in ENGINE_KEYS:
                got = eng.grads[key].cpu().numpy()
                if key == "unnorm_rotations" and not aniso:
                    assert float(np.abs(got).max()) == 0.0
                    continue
                assert_grad_calibrated(got, g32[key], g64[key], what=f"{what} grad {key}", tail_factor=tail)
                cc.assert_groupwise(got, g64[key], groups, what=f"{what} grad {key}")
                assert float(np.abs(got[groups['behind']]).max()) == 0.0, key
            assert not bool(eng.seen.cpu().numpy()[groups['behind']].any())
            grads = torch.cat([eng.grads[key].reshape(-1) for key in ENGINE_KEYS]).clone()
        outs.append((eng.buf['out6'].clone(), grads, eng.loss()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert abs(outs[0][2] - outs[1][2]) <= 1e-6 * abs(outs[0][2])
    if tracking:
        assert float((outs[0][1] - outs[1][1]).abs().max()) <= 2e-5 * float(outs[0][1].abs().max())
    else:
        o = 0
        for key in ENGINE_KEYS:
            m = p[key].numel()
            a, b = outs[0][1][o:o + m], outs[1][1][o:o + m]
            o += m
            assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-12, key
