"""The fused iteration and its callers at a NON-IDENTITY first-frame pose.

Two descriptions of "the world seen from the first frame" reach the kernels by separate routes: the camera's view / projection
matrices (FusedArgs.cam, column-major, into the projection and its adjoint) and curr_data['w2c'], whose row 2 makes the depth
channel of the depth / silhouette render (z = (w2c @ [Xc; 1])[2]) and whose adjoint w2c_row2 * dz joins dL/dXc and from there
every means3D and pose gradient.  At the identity -- where every other test of this chain runs -- row 2 equals column 2, the
translation is zero, the view matrix equals its transpose and first_frame_w2c @ pose_t collapses to pose_t.  Here the chain is
checked at a GENERAL rigid M (tests/util.py: general_w2c; tests/test_slam_mirror.py pins the mirror to the reference at the same
M), with the stages, tolerances and explained-outlier machinery of tests/test_gpu_configs.py (no new numbers):

  * configs A and D (fx != fy, off-centre principal point), isotropic and anisotropic, tracking and mapping, and the flagship
    config B (anisotropic) at M;
  * config A with curr_data['w2c'] = M2 while the camera is built from M (the post-optimisation scripts' usage);
  * config A at the matrix the frame loop really passes: inv(inv(P0) @ P0) in float32, an identity up to rounding only;
  * the depth term must MATTER in every comparison of a means3D / pose gradient: by the float64 oracle alone, the gradient
    without the depth plane's cotangent is further from the full one than 10x the tolerance applied.

Mutants tried against this module (arithmetic changes only, not committed): F1 reading column 2 of the matrix for row 2, and F6
doing the same, each fail the twelve cases at M / M2 below plus the multi-view and plugin cases (F1's also the add_new_gaussians
case), while every test that runs at the identity passes; the two cases at the frame loop's matrix pass, as they must (it is the
identity to rounding).  Dropping w2c_row2 * dz from the adjoint altogether fails all fourteen cases here, but ALSO the identity
cases of tests/test_gpu_fused.py and tests/test_gpu_configs.py (row 2 of the identity still carries dz into dL/dXc.z): the
identity suite already saw that the term exists, not which row it is.

Then every variant that reads the frame's matrix (the four forms of F1, the sharded and one-kernel tracking forms, the mapping
step in one call, the render-only call) through the tests that compare them at the identity, and the callers on top."""
import numpy as np
import pytest
import torch

from tests import test_gpu_configs as C
from tests.util import assert_close_outliers, assert_grad_calibrated, general_w2c, loop_first_w2c, other_w2c

pytestmark = pytest.mark.gpu

CONFIGS = dict(C.CONFIGS)
POSES = {
    'M': lambda: dict(first_w2c=general_w2c()),
    'M-camera-M2-depth': lambda: dict(first_w2c=general_w2c(), frame_w2c=other_w2c()),
    'loop': lambda: dict(first_w2c=loop_first_w2c()),
}
# (config, anisotropic, pose)
CASES = ([('A', aniso, 'M') for aniso in (False, True)] + [('D', aniso, 'M') for aniso in (False, True)] + [('B', True, 'M')]
         + [('A', False, 'M-camera-M2-depth'), ('A', False, 'loop')])
IDS = [f"{c}-{'aniso' if a else 'iso'}-{p}" for c, a, p in CASES]


def _without_depth_cotangent(eng, tracking, monkeypatch, pose):
    """The float64 oracle's gradients for the engine's gradient planes with the DEPTH plane's cotangent zeroed: what is left of the
    gradient when dz = 0, i.e. without w2c_row2 * dz (and the depth plane's share of dL/dalpha)."""
    cs = eng.case
    planes = eng.buf['dL_dout6'].detach().cpu().clone()
    assert float(planes[3].abs().max()) > 0.0
    planes[3] = 0.0
    return C._oracle_backward_from_planes(cs['params'], cs['frame'], cs['cam_args'], planes, tracking, torch.float64, monkeypatch, **pose)


@pytest.mark.parametrize("cfg_name,aniso,pose", CASES, ids=IDS)
def test_fused_mapping_vs_oracle_at_a_general_first_frame_pose(cfg_name, aniso, pose, monkeypatch):
    """Stages (A)..(D) of test_fused_mapping_vs_oracle with the camera built from M and curr_data['w2c'] = M (or M2)."""
    pose_name, pose = pose, POSES[pose]()
    eng, g32, g64, what = C._fused_case(cfg_name, aniso, False, monkeypatch, **pose)
    what += f" [{pose_name}]"
    keys = ["means3D", "rgb_colors", "logit_opacities", "log_scales"] + (["unnorm_rotations"] if aniso else [])
    tail = 2.0 if eng.depth_tie_pixels == 0 else 3.0
    for k in keys:
        assert_grad_calibrated(eng.grads[k].cpu().numpy(), g32[k], g64[k], what=f"{what} grad {k}", tail_factor=tail)
    if not aniso:
        assert float(eng.grads["unnorm_rotations"].abs().max()) == 0.0
    # the comparison of means3D cannot pass without the depth term: 10x the bound every element is held to (1e-3 of the maximum)
    nd = _without_depth_cotangent(eng, False, monkeypatch, pose)['means3D']
    full = g64['means3D']
    moved, scale = float(np.abs(full - nd).max()), float(np.abs(full).max())
    rows = float((np.abs(full - nd).max(axis=1) > 1e-2 * scale).mean())
    print(f"{what}: without the depth plane's cotangent dL/dmeans3D moves by {moved / scale:.3g} of its maximum ({100 * rows:.1f} % of the rows by "
          f"more than 10x the 1e-3 bound)")
    assert moved > 10.0 * 1e-3 * scale, (what, moved, scale)


@pytest.mark.parametrize("cfg_name,aniso,pose", CASES, ids=IDS)
def test_fused_tracking_vs_oracle_at_a_general_first_frame_pose(cfg_name, aniso, pose, monkeypatch):
    """Stages (A)..(D) of test_fused_tracking_vs_oracle (the shipped sil_thres = 0.99) with the camera built from M and
    curr_data['w2c'] = M (or M2)."""
    pose_name, pose = pose, POSES[pose]()
    eng, g32, g64, what = C._fused_case(cfg_name, aniso, True, monkeypatch, **pose)
    what += f" [{pose_name}]"
    tols = C._check_pose_gradient(eng, g32, g64, what)
    nd = _without_depth_cotangent(eng, True, monkeypatch, pose)
    for name, key, tol in (("rotation", 'cam_unnorm_rots', tols[0]), ("translation", 'cam_trans', tols[1])):
        moved = float(np.abs(g64[key][0, :, 1] - nd[key][0, :, 1]).max())
        print(f"{what}: without the depth plane's cotangent the {name} gradient moves by {moved:.4g} = {moved / tol:.3g}x the tolerance {tol:.3g}")
        assert moved > 10.0 * tol, (what, name, moved, tol)
    # ... and the one-kernel tracking forms (forward composite, loss and backward composite in ONE kernel, planes kept / in registers),
    # which the engine takes once it knows the lists: the same pose gradient against the oracle driven by THEIR gradient planes
    from splatam_amd import _capi
    cs = eng.case
    assert not eng.check_overflow() and eng.tile_stride > 0 and _capi.lists_sorted_by_composite(eng.max_list_hint), (eng.tile_stride, eng.max_list_hint)
    eng.begin_tracking(1)
    for form, keep in ((2, True), (1, False)):
        eng.loss_backward(cs['frame'], 1, cs['cfg'], tracking=True, keep_planes=keep)
        torch.cuda.synchronize()
        assert eng._lc_keep.fused_composite == form and eng._workspace(False, with_ssim=False).st.tile_stride > 0
        assert not eng.check_overflow(grow=False)
        if keep:
            planes = eng.buf['dL_dout6'].detach().cpu()
            g32, g64 = (C._oracle_backward_from_planes(cs['params'], cs['frame'], cs['cam_args'], planes, True, dt, monkeypatch, **pose)
                        for dt in (torch.float32, torch.float64))
        C._check_pose_gradient(eng, g32, g64, f"{what}, one-kernel form {form}")


# ---------------------------------------------------------------------------------------------------------------------
# every variant that reads the frame's matrix: the comparisons made at the identity, at M
# ---------------------------------------------------------------------------------------------------------------------
# frame.w2c is read by F1 (four forms: exact lists, per-tile buckets, aggregated bucket slots, group records; and the dense
# workgroup-histogram kernel) and by F6.  Each test below is the test of tests/test_gpu_fused.py that compares the forms at the
# identity (same helpers, same bounds, the same assertions on the engine's state about the form that ran), on a scene under M.

def test_learnt_lists_match_exact_lists_at_a_general_pose():
    from tests import test_gpu_fused as F
    for tracking in (True, False):
        F.test_bucketed_lists_match_exact_lists(tracking, first_w2c=general_w2c())


def test_aggregated_bucket_slots_change_nothing_at_a_general_pose():
    from tests import test_gpu_fused as F
    F.test_order_hint_changes_nothing_but_speed("random", first_w2c=general_w2c())


@pytest.mark.parametrize("case", ["random", "tracking"])
def test_group_binning_and_render_only_call_change_nothing_at_a_general_pose(case):
    """Group records against per-tile buckets, and FusedEngine.render (splat_iter_render) against the forward half of the full
    iteration: bit-identical planes."""
    from tests import test_gpu_fused as F
    F.test_group_binning_changes_nothing_but_speed(case, first_w2c=general_w2c())


def test_one_kernel_tracking_forms_equal_the_two_kernels_at_a_general_pose():
    from tests import test_gpu_fused as F
    F.test_tracking_composites_in_one_kernel_equal_the_two_kernels(20000, 328, 248, "one batch per tile, general pose", first_w2c=general_w2c())


def test_tile_row_sharded_tracking_equals_whole_frame_tracking_at_a_general_pose():
    from tests import test_gpu_fused as F
    F.test_tile_row_sharded_tracking_equals_whole_frame_tracking("learnt", 2, first_w2c=general_w2c())


def test_mapping_step_in_one_call_at_a_general_pose():
    from tests import test_gpu_fused as F
    F.test_mapping_step_in_one_call_equals_loss_backward_plus_adam(True, first_w2c=general_w2c())


def test_dense_preprocess_matches_exact_lists_at_a_general_pose():
    """fused_preprocess_dense_kernel (F1 with a workgroup-level tile histogram): launched for bucketed lists longer than the composite
    sorts itself, without an order hint or group records, on at least 32 768 Gaussians and at most 12 288 tiles.  Config D's camera
    (fx != fy, off-centre principal point) with 400 000 Gaussians -- D's own 150 000 leave the longest list at ~380, which the
    composite sorts itself -- under M, against the exact lists of a fresh engine, with the bounds of
    test_bucketed_lists_match_exact_lists."""
    from splatam_amd import _capi, slam
    from splatam_amd.fused import FusedEngine
    from tests import test_gpu_fused as F
    c = dict(CONFIGS['D'], n=400_000)
    M = general_w2c()
    params, variables = slam.synthetic_params(c['n'], c['W'], c['H'], c['fx'], c['fy'], c['cx'], c['cy'], num_frames=3, seed=3, device="cuda")
    c2w = torch.tensor(np.linalg.inv(M.astype(np.float64))).float().cuda()
    with torch.no_grad():
        params['means3D'].copy_(params['means3D'] @ c2w[:3, :3].T + c2w[:3, 3])
        params['cam_unnorm_rots'][0, :, 1] = torch.tensor([0.98, 0.01, -0.02, 0.015], device="cuda") * 1.1
        params['cam_trans'][0, :, 1] = torch.tensor([0.01, -0.02, 0.015], device="cuda")
    w2c = torch.tensor(M, device="cuda")
    cam = slam.setup_camera(c['W'], c['H'], [[c['fx'], 0, c['cx']], [0, c['fy'], c['cy']], [0, 0, 1]], M, device="cuda")
    im, depth = slam.synthetic_frame(params, cam, w2c, 1, rot_deg=0.4, trans_m=0.01)
    frame = {'cam': cam, 'im': im, 'depth': depth, 'id': 1, 'w2c': w2c}
    cfg = slam.REPLICA_MAPPING
    eng = FusedEngine(params, cam)
    for _ in range(3):                                  # (the default list capacity may be outgrown once)
        eng.loss_backward(frame, 1, cfg, tracking=False)
        torch.cuda.synchronize()
        ref = dict(out6=eng.buf['out6'].clone(), d=eng.buf['d_cam'][:8].clone(), g={k: v.clone() for k, v in eng.grads.items()})
        exact = eng.tile_stride == 0
        if not eng.check_overflow():
            break
    assert exact and eng.tile_stride > 0
    # the conditions of the dense launch, from the engine's state
    st = eng._workspace(False, with_ssim=False).st
    print(f"dense F1: longest list {eng.max_list_hint}, bucket stride {st.tile_stride}, {eng.num_tiles} tiles, {eng.P} Gaussians")
    assert st.tile_stride > 0 and st.group_stride == 0 and not st.order_hint
    assert not _capi.lists_sorted_by_composite(eng.max_list_hint) and eng.P >= 32768 and eng.num_tiles <= 12288
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    assert float(eng.buf['d_cam'][12]) == 0.0
    assert torch.equal(eng.buf['out6'], ref['out6'])    # the same sorted lists: the same planes, bit for bit
    assert (eng.buf['d_cam'][:8] - ref['d']).abs().max() <= 1e-4 * ref['d'].abs().max()
    for k in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
        assert (eng.grads[k] - ref['g'][k]).abs().max() <= 1e-4 * ref['g'][k].abs().max() + 1e-12, k
    assert int(eng.buf['tile_count'].abs().max()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# a frame matrix the kernels cannot read is refused before anything is launched
# ---------------------------------------------------------------------------------------------------------------------

def _small_engine(first_w2c):
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    from tests import test_gpu_fused as F
    params, variables, frame, cam = F._scene(6000, 160, 112, seed=5, first_w2c=first_w2c)
    return FusedEngine(params, cam), frame, slam.REPLICA_MAPPING


def _state(eng):
    keys = ('out6', 'dL_dout6', 'd_cam', 'status', 'tile_count', 'sums', 'accum')
    return {k: eng.buf[k].clone() for k in keys}, {k: v.clone() for k, v in eng.grads.items()}


@pytest.mark.parametrize("bad", ["float64", "cpu", "[3, 4]", "[1, 4, 4]", "numpy"])
def test_unreadable_frame_matrix_is_refused_before_any_launch(bad):
    """curr_data['w2c'] that is not 16 float32 values on the engine's device (float64: what an inverse taken in double gives; a CPU
    tensor: np.load + torch.tensor; a row short; a batch) raises a RuntimeError naming the field -- as the reference's own matmul
    does for a dtype / device mismatch -- from loss_backward and from render, and leaves the rendered planes, the gradients and
    the overflow / skip counters as they were."""
    M = general_w2c()
    eng, frame, cfg = _small_engine(M)
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    assert float(eng.buf['out6'].abs().max()) > 0.0
    before_buf, before_grads = _state(eng)
    good = frame['w2c']
    wrong = {"float64": good.double(), "cpu": good.cpu(), "[3, 4]": good[:3].contiguous(), "[1, 4, 4]": good[None].contiguous(),
             "numpy": M}[bad]
    for call in (lambda f: eng.loss_backward(f, 1, cfg, tracking=False), lambda f: eng.loss_backward(f, 1, cfg, tracking=True),
                 lambda f: eng.render(f, 1)):
        with pytest.raises(RuntimeError, match=r"curr_data\['w2c'\]"):
            call(dict(frame, w2c=wrong))
    torch.cuda.synchronize()
    after_buf, after_grads = _state(eng)
    for k in before_buf:
        assert torch.equal(before_buf[k], after_buf[k]), k
    for k in before_grads:
        assert torch.equal(before_grads[k], after_grads[k]), k
    eng.loss_backward(frame, 1, cfg, tracking=False)        # ... and the engine goes on as if nothing had been asked
    torch.cuda.synchronize()
    assert torch.equal(eng.buf['out6'], before_buf['out6'])
    assert not eng.check_overflow(grow=False) and eng.skipped_iterations == 0


def test_views_of_the_frame_matrix_give_the_contiguous_matrix_results():
    """A transposed view (M.T.contiguous().T) and a [4, 4] slice out of an [N, 4, 4] stack (a keyframe list's matrices) are the same
    16 numbers: bit-identical rendered planes, gradient planes, loss and gradients."""
    M = general_w2c()
    eng, frame, cfg = _small_engine(M)
    good = frame['w2c']
    transposed_view = good.T.contiguous().T
    stack = torch.stack([torch.eye(4, device="cuda"), good, 2.0 * good])
    assert not transposed_view.is_contiguous() and torch.equal(transposed_view, good) and stack[1].is_contiguous()
    results = []
    for w2c in (good, transposed_view, stack[1]):
        for tracking in (False, True):
            eng.loss_backward(dict(frame, w2c=w2c), 1, cfg, tracking=tracking)
            torch.cuda.synchronize()
            out = [eng.buf['out6'].clone(), eng.buf['dL_dout6'].clone()]
            eng.render(dict(frame, w2c=w2c), 1)
            torch.cuda.synchronize()
            results.append((tracking, out + [eng.buf['out6'].clone()]))
    for (tr, res), (tr0, res0) in zip(results[2:], results[:2] * 2):
        assert tr == tr0
        for a, b in zip(res, res0):
            assert torch.equal(a, b)
    assert not eng.check_overflow(grow=False)


# ---------------------------------------------------------------------------------------------------------------------
# the callers on top, one small case each at M, against what they are compared with at the identity
# ---------------------------------------------------------------------------------------------------------------------

def test_add_new_gaussians_on_a_real_render_at_a_general_pose():
    """FusedEngine.add_new_gaussians thresholds the silhouette and depth planes of its own render -- the depth plane is the one row 2
    of curr_data['w2c'] produced -- against slam._add_from_render fed with the same planes (as
    test_render_only_pass_matches_full_iteration_and_densification_full_size does at the identity and workload size)."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    from tests import test_gpu_fused as F
    from tests.test_gpu_mapedit import VAR_KEYS
    M = general_w2c()
    n, W, H = 12000, 256, 192
    params, variables, frame, cam = F._scene(n, W, H, seed=13, first_w2c=M)
    f = 0.5 * W
    frame['intrinsics'] = torch.tensor([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]])
    with torch.no_grad():
        frame['depth'][:, 40:70, 60:120] *= 0.5             # a new foreground object in front of the map
        Mt = frame['w2c']
        Xc = params['means3D'] @ Mt[:3, :3].T + Mt[:3, 3]
        params['logit_opacities'][Xc[:, 0] / Xc[:, 2] > 0.5] = -6.0          # thin the map on one side: low silhouette there
    ref_params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}
    ref_vars = {k: v.clone() for k, v in variables.items()}
    eng = FusedEngine(params, cam, gaussian_capacity=n + 40000, variables=variables)
    out = eng.render(frame, 1)
    torch.cuda.synchronize()
    assert not eng.check_overflow()
    depth_sil = torch.stack([out[1][0], out[2]]).clone()
    # the planes it thresholds are the reference's: its add_new_gaussians renders them itself (/root/reference/scripts/splatam.py:381-385),
    # here on the drop-in rasterizer; the figures of stage (A) of tests/test_gpu_configs.py (_fused_stages)
    with torch.no_grad():
        tg = slam.transform_to_frame(ref_params, 1, gaussians_grad=False, camera_grad=False)
        ds, _, _ = slam.Renderer(raster_settings=cam)(**slam.transformed_params2depthplussilhouette(ref_params, frame['w2c'], tg))
    assert_close_outliers(depth_sil.cpu().numpy(), ds[0:2].cpu().numpy(), 1e-4, rtol=1e-4, max_outlier_frac=2e-4,
                          what="depth / silhouette planes of the render add_new_gaussians thresholds")
    added = eng.add_new_gaussians(frame, 0.5, 1, "projective", "isotropic")
    ref_params, ref_vars = slam._add_from_render(ref_params, ref_vars, frame, depth_sil, 0.5, 1, "projective", "isotropic")
    n1 = ref_params['means3D'].shape[0]
    print(f"add_new_gaussians at a general first-frame pose: {added} rows added to {n}")
    assert added == n1 - n and added > 1000
    for k in slam.GAUSSIAN_KEYS:
        np.testing.assert_allclose(params[k].detach().cpu().numpy(), ref_params[k].detach().cpu().numpy(), rtol=3e-6, atol=3e-6, err_msg=k)
    for k in VAR_KEYS:
        assert torch.equal(variables[k], ref_vars[k]), k


def test_multiview_mapping_batch_at_a_general_pose():
    """The multi-view mapping step (8 keyframe views averaged + one Adam step against autograd on the drop-in rasterizer and
    torch.optim.Adam) on the small map, the map and all eight keyframes under M: every keyframe pose is conjugated by M
    (tests/util.py: conjugate_pose), so each view sees what it sees at the identity and the partition of the map is the same."""
    from tests import test_gpu_mapping_views as V
    V.test_mapping_batch_config3_vs_autograd_and_adam('small', first_w2c=general_w2c())


def test_plugin_statements_at_a_general_pose():
    """plugin.install: the reference-shaped tracking and mapping statements with curr_data['w2c'] = M against slam.get_loss on the
    drop-in rasterizer."""
    from tests import test_gpu_plugin as P
    P.test_tracking_statements_run_fused_and_match_the_dropin_path(first_w2c=general_w2c())
    P.test_mapping_statements_with_the_references_pruning_run_fused(first_w2c=general_w2c())
