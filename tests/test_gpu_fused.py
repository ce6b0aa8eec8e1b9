"""Parity of the fused SplaTAM iteration (splatam_amd/fused.py over the C ABI's splat_iter_* entry points)
against the reference-shaped path: splatam_amd.slam.get_loss (pinned to /root/reference's own get_loss by
tests/golden/) + torch.autograd + torch.optim.Adam, both running on the HIP rasterizer.  Tolerances: 1e-4
relative on the loss, 1e-3 of the tensor's max magnitude on gradients (north star), Adam updates to 1e-6."""
import copy

import numpy as np
import pytest
import torch

from tests.util import assert_close_outliers, grad_scale, track_loop_loss_rtol

pytestmark = pytest.mark.gpu


def _scene(n, W, H, aniso=False, seed=0, num_frames=3, first_w2c=None):
    """``first_w2c`` (default: the identity): the camera's matrix and curr_data['w2c']; the map, made at the identity, is moved by its
    inverse so that it fills the frame as before (tests/test_gpu_world_frame.py runs the variant comparisons below at a general one)."""
    from splatam_amd import slam
    f = 0.5 * W
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    params, variables = slam.synthetic_params(n, W, H, f, f, cx, cy, num_frames=num_frames, seed=seed, device="cuda",
                                              anisotropic=aniso)
    k = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    w2c = torch.eye(4, device="cuda")
    if first_w2c is not None:
        w2c = torch.tensor(np.ascontiguousarray(np.asarray(first_w2c, dtype=np.float32)), device="cuda")
        c2w = torch.tensor(np.linalg.inv(np.asarray(first_w2c, dtype=np.float64))).float().cuda()
        with torch.no_grad():
            params['means3D'].copy_(params['means3D'] @ c2w[:3, :3].T + c2w[:3, 3])
    cam = slam.setup_camera(W, H, k, w2c.cpu().numpy(), device="cuda")
    im, depth = slam.synthetic_frame(params, cam, w2c, 1, rot_deg=0.4, trans_m=0.01)
    g = torch.Generator().manual_seed(seed + 1)
    im = (im + 0.03 * torch.randn(im.shape, generator=g).cuda()).clamp(0, 1)
    depth = depth * (1 + 0.01 * torch.randn(depth.shape, generator=g).cuda())
    depth[:, : H // 8, : W // 8] = 0.0                      # a patch of invalid depth (mask path)
    frame = {'cam': cam, 'im': im.contiguous(), 'depth': depth.contiguous(), 'id': 1, 'w2c': w2c}
    with torch.no_grad():                                   # a pose that is not the identity and not unit length
        params['cam_unnorm_rots'][0, :, 1] = torch.tensor([0.98, 0.01, -0.02, 0.015], device="cuda") * 1.1
        params['cam_trans'][0, :, 1] = torch.tensor([0.01, -0.02, 0.015], device="cuda")
    return params, variables, frame, cam


def _reference_grads(params, variables, frame, cfg, tracking):
    from splatam_amd import slam
    for p in params.values():
        p.grad = None
    loss, _, _ = slam.get_loss(params, frame, dict(variables), 1, cfg['loss_weights'], cfg['use_sil_for_loss'], cfg['sil_thres'],
                               cfg['use_l1'], cfg['ignore_outlier_depth_loss'], tracking=tracking, mapping=not tracking)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in params.items()}


def _gap_threshold(params, frame, cam, cfg):
    """The tracking loss is a SUM over the pixels with silhouette > sil_thres: a pixel whose silhouette sits within
    float32 evaluation-order noise (~1e-5) of the threshold enters or leaves the sum -- and the pose gradient -- with
    its whole error.  One such pixel moved the loss by 1e-4 and a gradient component by 1 % in this scene, in two
    evaluations that agree to 1e-5 per pixel.  Parity of the two paths is therefore checked at a threshold with no
    pixel that close to it."""
    from splatam_amd import slam
    with torch.no_grad():
        tg = slam.transform_to_frame(params, 1, False, False)
        dv = slam.transformed_params2depthplussilhouette(params, frame['w2c'], tg)
        ds, _, _ = slam.Renderer(raster_settings=cam)(**dv)
    sil = ds[1].reshape(-1)
    v = torch.sort(sil[(sil > 0.9) & (sil < 0.9995)]).values
    gaps = v[1:] - v[:-1]
    k = int(torch.argmax(gaps))
    assert float(gaps[k]) > 4e-5, "no gap in the silhouette histogram"
    out = copy.deepcopy(cfg)
    out['sil_thres'] = float(0.5 * (v[k] + v[k + 1]))
    return out


def _cmp(got, ref, what, tol=1e-3):
    ref = ref.cpu().numpy()
    got = got.cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), what
    assert_close_outliers(got, ref, tol * grad_scale(ref), max_outlier_frac=2e-4, outlier_atol=0.05 * grad_scale(ref), what=what)


@pytest.mark.parametrize("aniso", [False, True])
def test_tracking_loss_and_pose_gradient(aniso):
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 320, 240, aniso=aniso, seed=3)
    cfg = _gap_threshold(params, frame, cam, slam.REPLICA_TRACKING)
    loss_ref, g_ref = _reference_grads(params, variables, frame, cfg, tracking=True)
    eng = FusedEngine(params, cam)
    eng.loss_backward(frame, 1, cfg, tracking=True)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    d = eng.buf['d_cam'].cpu().numpy()
    assert abs(d[7] - loss_ref) <= 1e-4 * abs(loss_ref), (d[7], loss_ref)
    gq = g_ref['cam_unnorm_rots'][0, :, 1].cpu().numpy()
    gt = g_ref['cam_trans'][0, :, 1].cpu().numpy()
    assert np.abs(d[0:4] - gq).max() <= 1e-3 * np.abs(gq).max(), (d[0:4], gq)
    assert np.abs(d[4:7] - gt).max() <= 1e-3 * np.abs(gt).max(), (d[4:7], gt)
    # the rendered planes are the two reference renders
    im, depth, sil, dsq = eng.rendered()
    tg = slam.transform_to_frame(params, 1, False, False)
    with torch.no_grad():
        rv = slam.transformed_params2rendervar(params, tg)
        im_ref, _, _ = slam.Renderer(raster_settings=cam)(**rv)
        dv = slam.transformed_params2depthplussilhouette(params, frame['w2c'], tg)
        ds_ref, _, _ = slam.Renderer(raster_settings=cam)(**dv)
    assert_close_outliers(im.cpu().numpy(), im_ref.cpu().numpy(), 1e-4, max_outlier_frac=1e-4, outlier_atol=0.03, what="im")
    assert_close_outliers(torch.cat([depth, sil[None], dsq]).cpu().numpy(), ds_ref.cpu().numpy(), 1e-4, rtol=1e-4,
                          max_outlier_frac=1e-4, outlier_atol=0.3, what="depth_sil")


@pytest.mark.parametrize("aniso", [False, True])
def test_mapping_loss_and_gaussian_gradients(aniso):
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 320, 240, aniso=aniso, seed=5)
    cfg = slam.REPLICA_MAPPING
    loss_ref, g_ref = _reference_grads(params, variables, frame, cfg, tracking=False)
    eng = FusedEngine(params, cam)
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    assert abs(eng.loss() - loss_ref) <= 1e-4 * abs(loss_ref), (eng.loss(), loss_ref)
    for k in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
        _cmp(eng.grads[k], g_ref[k], k)
    if aniso:
        _cmp(eng.grads["unnorm_rotations"], g_ref["unnorm_rotations"], "unnorm_rotations")
    else:
        # isotropic: Sigma = s^2 R R^T does not depend on the direction of the quaternion, both gradients are
        # rounding noise around zero (orders of magnitude below the scale gradient)
        assert float(eng.grads["unnorm_rotations"].abs().max()) <= 1e-3 * float(g_ref["log_scales"].abs().max())
    assert g_ref['cam_trans'] is None or float(g_ref['cam_trans'].abs().max()) == 0.0


def test_mapping_adam_steps_match_torch():
    """Three fused mapping iterations against get_loss + backward + torch.optim.Adam(eps=1e-15)."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(8000, 208, 160, aniso=True, seed=7)
    cfg = slam.REPLICA_MAPPING
    ref = {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}
    opt = slam.initialize_optimizer(ref, cfg['lrs'], tracking=False)
    eng = FusedEngine(params, cam)
    first_grads = None
    for it in range(3):
        _, g = _reference_grads(ref, variables, frame, cfg, tracking=False)
        if first_grads is None:
            first_grads = g
        with torch.no_grad():
            opt.step()
            opt.zero_grad(set_to_none=True)
        eng.mapping_iteration(frame, 1, cfg)
    torch.cuda.synchronize()
    for k in ("means3D", "rgb_colors", "logit_opacities", "log_scales", "unnorm_rotations"):
        lr = cfg['lrs'][k]
        a, b = params[k].detach(), ref[k].detach()
        # Adam with eps = 1e-15 moves every element by ~lr * sign(g): elements whose gradient is rounding noise may
        # step the other way; compare where the first gradient is significant
        sig = first_grads[k].abs() > 1e-4 * first_grads[k].abs().max()
        diff = (a - b).abs()[sig]
        assert float((diff > 0.05 * lr).float().mean()) < 5e-3, (k, float(diff.max()), lr)
    assert torch.equal(params['cam_trans'], ref['cam_trans'])


def test_tracking_loop_matches_reference_loop():
    """Six tracking iterations (Adam on the pose + best-candidate bookkeeping) against the reference-shaped loop."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(12000, 256, 192, aniso=False, seed=11)
    cfg = slam.REPLICA_TRACKING
    ref = {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}
    opt = slam.initialize_optimizer(ref, cfg['lrs'], tracking=True)
    state = slam.TrackingState(ref, 1)
    eng = FusedEngine(params, cam)
    eng.begin_tracking(1)
    losses = []
    for it in range(6):
        loss, _ = slam.tracking_iteration(ref, frame, dict(variables), 1, opt, state, cfg)
        losses.append(float(loss.detach()))
        eng.tracking_iteration(frame, cfg)
        # the render changes every iteration, so threshold pixels (see _gap_threshold) cannot be excluded here: allow
        # a few of them per iteration
        assert abs(eng.loss() - losses[-1]) <= track_loop_loss_rtol(it) * abs(losses[-1]), (it, eng.loss(), losses[-1])
    torch.cuda.synchronize()
    q_ref, t_ref = ref['cam_unnorm_rots'][0, :, 1], ref['cam_trans'][0, :, 1]
    # Adam normalises the gradient: a threshold pixel changes an update by a fraction of lr (0.0004 / 0.002); bound: a fifth of ONE
    # step's lr after six steps (observed 0.5e-4 .. 2.0e-4 on the translation over compiler-flag variants of the same kernels)
    assert (params['cam_unnorm_rots'][0, :, 1] - q_ref).abs().max() <= 1e-4
    assert (params['cam_trans'][0, :, 1] - t_ref).abs().max() <= 4e-4
    st = eng.buf['pose_state']
    assert abs(float(st[14]) - float(state.min_loss)) <= 1e-3 * float(state.min_loss)
    assert (st[15:19] - state.best_rot.reshape(-1)).abs().max() <= 1e-4
    assert (st[19:22] - state.best_tran.reshape(-1)).abs().max() <= 4e-4
    eng.end_tracking()
    state.commit(ref)
    assert (params['cam_trans'] - ref['cam_trans']).abs().max() <= 4e-4
    # Gaussians untouched by tracking (LR 0 in the reference)
    assert torch.equal(params['means3D'], ref['means3D']) and torch.equal(params['rgb_colors'], ref['rgb_colors'])


@pytest.mark.parametrize("tracking", [True, False])
def test_bucketed_lists_match_exact_lists(tracking, first_w2c=None):
    """check_overflow() teaches the engine the list statistics; from then on the per-tile lists are bucketed (no scan /
    scatter pass).  Same lists but for the entries that cannot blend, same results: only the order of float atomics differs."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 320, 240, aniso=not tracking, seed=21, first_w2c=first_w2c)
    cfg = slam.REPLICA_TRACKING if tracking else slam.REPLICA_MAPPING
    eng = FusedEngine(params, cam)
    eng.loss_backward(frame, 1, cfg, tracking=tracking)
    torch.cuda.synchronize()
    ref_cam = eng.buf['d_cam'][:8].clone()
    ref_grads = {k: v.clone() for k, v in eng.grads.items()}
    ref_lists = None
    assert eng.tile_stride == 0 and not eng.check_overflow()
    assert eng.tile_stride >= 256 and eng.tile_stride * eng.num_tiles <= eng.capacity
    assert 0 < eng.max_list_hint <= 800         # short lists: the composite kernel sorts them itself from here on
    n_exact = int(eng.buf['status'][0])
    for _ in range(2):                      # twice: the counters must come back to zero by themselves
        eng.loss_backward(frame, 1, cfg, tracking=tracking)
        torch.cuda.synchronize()
        assert float(eng.buf['d_cam'][12]) == 0.0
        # (group binning: the entries whose tile cannot hold a pixel with alpha >= 1/255 are not filed -- splat_math.h live_tile_rect)
        n_group = int(eng.buf['status'][0])
        assert 0.6 * n_exact <= n_group <= n_exact and (ref_lists is None or n_group == ref_lists)
        ref_lists = n_group
        got = eng.buf['d_cam'][:8]
        assert (got - ref_cam).abs().max() <= 1e-4 * ref_cam.abs().max()
        if not tracking:
            for k in ("means3D", "rgb_colors", "logit_opacities", "log_scales", "unnorm_rotations"):
                assert (eng.grads[k] - ref_grads[k]).abs().max() <= 1e-4 * ref_grads[k].abs().max() + 1e-12, k
    assert not eng.check_overflow()
    assert int(eng.buf['tile_count'].abs().max()) == 0


def test_bucket_overflow_falls_back_to_exact_lists():
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 96, 64, seed=23)          # dense: hundreds of instances per tile
    cfg = slam.REPLICA_TRACKING
    eng = FusedEngine(params, cam)
    eng.loss_backward(frame, 1, cfg, tracking=True)
    torch.cuda.synchronize()
    loss_exact = eng.loss()
    assert not eng.check_overflow()
    eng.tile_stride = 64                                                     # force buckets that are too small
    eng.loss_backward(frame, 1, cfg, tracking=True)
    torch.cuda.synchronize()
    assert eng.check_overflow()                                              # flagged; engine is back on exact lists
    assert eng.tile_stride == 0
    eng.loss_backward(frame, 1, cfg, tracking=True)
    torch.cuda.synchronize()
    assert abs(eng.loss() - loss_exact) <= 1e-5 * abs(loss_exact)
    assert not eng.check_overflow(grow=False)


def test_list_overflow_is_flagged_not_fatal():
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(5000, 160, 112, seed=13)
    eng = FusedEngine(params, cam, capacity=100)            # far too small
    eng.loss_backward(frame, 1, slam.REPLICA_TRACKING, tracking=True)
    torch.cuda.synchronize()
    assert eng.check_overflow(grow=True)                    # flagged, lists re-sized
    eng.loss_backward(frame, 1, slam.REPLICA_TRACKING, tracking=True)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    assert np.isfinite(eng.loss()) and eng.loss() > 0


def test_missing_outlier_scratch_is_an_invalid_argument():
    """ignore_outlier_depth_loss needs its two scratch arrays at the C ABI (the engine allocates them on first use)."""
    import ctypes as C
    from splatam_amd import _capi, slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(1000, 96, 64, seed=17)
    eng = FusedEngine(params, cam)
    cfg = copy.deepcopy(slam.REPLICA_TRACKING)
    cfg['ignore_outlier_depth_loss'] = True
    lc = eng.loss_config(cfg, True)
    ws = eng._workspace(False, with_ssim=False)            # no outlier scratch yet
    fr = _capi.SplatFrameData()
    fr.im, fr.depth, fr.w2c, fr.time_idx = frame['im'].data_ptr(), frame['depth'].data_ptr(), frame['w2c'].data_ptr(), 1
    m = eng._map_struct()
    rc = eng.L.splat_iter_loss_backward(C.byref(eng._cam), C.byref(m), C.byref(fr), C.byref(lc), C.byref(ws), eng._stream())
    assert rc == 1
    eng.loss_backward(frame, 1, cfg, tracking=True)        # the engine path allocates them
    torch.cuda.synchronize()
    assert np.isfinite(eng.loss())


def test_edge_shapes_and_empty_map():
    """Image not a multiple of the tile / SSIM block sizes, odd pixel count (F4 / F5 pixel by pixel; the tracking loss is formed in
    the composite's epilogue here -- the scalar form of the loss kernel is reached only with outlier rejection, in
    tests/test_gpu_loss_configs.py), and a map with no visible Gaussian: finite results, zero gradients where nothing is rendered."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(3000, 203, 117, aniso=True, seed=31)          # 203*117 is odd
    for tracking, cfg in ((True, slam.REPLICA_TRACKING), (False, slam.REPLICA_MAPPING)):
        cfg2 = _gap_threshold(params, frame, cam, cfg) if tracking else cfg
        loss_ref, g_ref = _reference_grads(params, variables, frame, cfg2, tracking=tracking)
        eng = FusedEngine(params, cam)
        eng.loss_backward(frame, 1, cfg2, tracking=tracking)
        torch.cuda.synchronize()
        assert abs(eng.loss() - loss_ref) <= 2e-4 * abs(loss_ref), (tracking, eng.loss(), loss_ref)
        if tracking:
            gq = g_ref['cam_unnorm_rots'][0, :, 1]
            assert (eng.buf['d_cam'][0:4] - gq).abs().max() <= 2e-3 * gq.abs().max()
        else:
            _cmp(eng.grads['means3D'], g_ref['means3D'], 'means3D')
            _cmp(eng.grads['rgb_colors'], g_ref['rgb_colors'], 'rgb_colors')
    # everything behind the camera: nothing rendered, loss = the empty-image loss, all gradients zero
    with torch.no_grad():
        params['means3D'][:, 2] = -1.0
    eng = FusedEngine(params, cam)
    eng.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False)
    torch.cuda.synchronize()
    assert int(eng.buf['status'][0]) == 0 and not eng.check_overflow()
    assert float(eng.grad_flat.abs().max()) == 0.0
    loss_ref, _ = _reference_grads(params, variables, frame, slam.REPLICA_MAPPING, tracking=False)
    assert abs(eng.loss() - loss_ref) <= 1e-5 * abs(loss_ref)


def test_stale_list_length_hint_is_flagged_and_memory_safe():
    """A list longer than the wave-sort limit meeting a stale host hint (which skipped the long-list sort launch) must be
    flagged for a re-run AND must not feed unwritten list slots to the composite kernels (found by running the frame loop
    on re-used allocator memory: garbage ids -> memory fault)."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(60000, 96, 64, seed=11)       # dense: several thousand instances per tile
    eng = FusedEngine(params, cam)
    eng.allow_buckets = False
    cfg = slam.REPLICA_MAPPING
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow()
    assert eng.max_list_hint > 1024
    good = eng.grads['means3D'].clone()
    good_loss = eng.loss()
    eng.buf['point_list'].fill_(0x7f7f7f7f)                              # what re-used allocator memory looks like
    eng.max_list_hint = 100                                              # stale: claims that no list needs the long-list sort
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()                                            # no memory fault
    assert eng.check_overflow()                                          # ... and the iteration is reported as invalid
    eng.loss_backward(frame, 1, cfg, tracking=False)                     # hint reset by check_overflow: sorted again
    torch.cuda.synchronize()
    assert not eng.check_overflow()
    assert abs(eng.loss() - good_loss) <= 1e-5 * abs(good_loss)
    _cmp(eng.grads['means3D'], good, "dL/dmeans3D after recovery", tol=1e-4)


@pytest.mark.parametrize("tracking", [True, False])
def test_ignore_outlier_depth_loss(tracking):
    """get_loss(ignore_outlier_depth_loss=True): mask = (depth_error < 10 * depth_error.median()) & (gt_depth > 0)
    (/root/reference/scripts/splatam.py:264-272).  The median is torch.median's, bit for bit (exact radix selection on the
    device); loss and gradients match the reference-shaped path."""
    import copy
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 320, 240, seed=13)
    frame['depth'] = frame['depth'].clone()
    frame['depth'][:, 100:140, 60:140] *= 4.0                  # regions of gross depth outliers
    frame['depth'][:, 10:20, 200:260] += 6.0
    base = slam.REPLICA_TRACKING if tracking else slam.REPLICA_MAPPING
    cfg = copy.deepcopy(_gap_threshold(params, frame, cam, base) if tracking else base)
    cfg['ignore_outlier_depth_loss'] = True
    loss_ref, g_ref = _reference_grads(params, variables, frame, cfg, tracking=tracking)
    cfg_off = copy.deepcopy(cfg)
    cfg_off['ignore_outlier_depth_loss'] = False
    loss_off, _ = _reference_grads(params, variables, frame, cfg_off, tracking=tracking)
    assert abs(loss_off - loss_ref) > 1e-2 * abs(loss_ref), (loss_off, loss_ref)    # the outliers matter in this scene
    eng = FusedEngine(params, cam)
    eng.loss_backward(frame, 1, cfg, tracking=tracking)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    _, depth, _, _ = eng.rendered()
    gt = frame['depth']
    med_ref = (torch.abs(gt - depth) * (gt > 0)).median()
    assert float(eng.buf['d_cam'][13]) == float(med_ref)      # bit-exact on the engine's own render
    assert abs(eng.loss() - loss_ref) <= 3e-4 * abs(loss_ref), (eng.loss(), loss_ref)
    if tracking:
        d = eng.buf['d_cam'].cpu().numpy()
        gq = g_ref['cam_unnorm_rots'][0, :, 1].cpu().numpy()
        gtr = g_ref['cam_trans'][0, :, 1].cpu().numpy()
        assert np.abs(d[0:4] - gq).max() <= 3e-3 * np.abs(gq).max(), (d[0:4], gq)
        assert np.abs(d[4:7] - gtr).max() <= 3e-3 * np.abs(gtr).max(), (d[4:7], gtr)
    else:
        for k in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
            _cmp(eng.grads[k], g_ref[k], k)


def test_view_sharded_exchange_keeps_replicas_identical():
    """The exchange step of view-sharded mapping on the fused path, emulated in one process: two replicas render different
    keyframe views, average the exchanged prefix of their flat gradient buffers (8 floats per isotropic Gaussian: the rotation
    gradient is exactly zero and stays out of the collective) and take the same Adam step."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(8000, 208, 160, seed=23, num_frames=4)
    frame2 = dict(frame)
    frame2['im'] = (frame['im'] * 0.9 + 0.03).contiguous()
    cfg = slam.REPLICA_MAPPING
    reps = []
    for fr, t in ((frame, 1), (frame2, 2)):
        p = {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}
        eng = FusedEngine(p, cam)
        eng.loss_backward(fr, t, cfg, tracking=False)
        reps.append((p, eng))
    torch.cuda.synchronize()
    (p1, e1), (p2, e2) = reps
    assert e1.reduce_flat.numel() == 8 * e1.P and e1.grad_flat.numel() == 12 * e1.P
    assert float(e1.grads['unnorm_rotations'].abs().max()) == 0.0
    assert e1.reduce_flat.data_ptr() == e1.grad_flat.data_ptr()
    mean = 0.5 * (e1.reduce_flat + e2.reduce_flat)
    assert float((e1.reduce_flat - e2.reduce_flat).abs().max()) > 0.0        # the views really differ
    for e in (e1, e2):
        e.reduce_flat.copy_(mean)
        e.adam_map(cfg['lrs'])
    torch.cuda.synchronize()
    for k in ('means3D', 'rgb_colors', 'logit_opacities', 'log_scales', 'unnorm_rotations'):
        assert torch.equal(p1[k].detach(), p2[k].detach()), k
    assert torch.equal(p1['unnorm_rotations'].detach(), params['unnorm_rotations'].detach())      # untouched
    assert not torch.equal(p1['means3D'].detach(), params['means3D'].detach())


def test_mapping_batch_equals_gradient_accumulation():
    """FusedEngine.mapping_batch (BASELINE config 3: several keyframe views per mapping step; the ranks' sums are exchanged by ONE
    all-reduce) against its definition: the mean of the per-view gradients, one Adam step.  Two 'ranks' are emulated in one
    process: each accumulates its own view, the exchange callback adds the other rank's sum."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(8000, 208, 160, seed=29, num_frames=4)
    views = [(frame, 1), (dict(frame, im=(frame['im'] * 0.9 + 0.03).contiguous()), 2), (dict(frame, im=(frame['im'] * 0.8 + 0.1).contiguous()), 3)]
    cfg = slam.REPLICA_MAPPING
    clone = lambda: {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}      # noqa: E731
    # definition: per-view gradients averaged, one Adam step
    p_ref = clone()
    e_ref = FusedEngine(p_ref, cam)
    acc = torch.zeros_like(e_ref.grad_flat)
    for fr, t in views:
        e_ref.loss_backward(fr, t, cfg, tracking=False)
        acc += e_ref.grad_flat
    e_ref.grad_flat.copy_(acc / len(views))
    e_ref.adam_map(cfg['lrs'])
    # one process, all three views in one batch
    p_one = clone()
    FusedEngine(p_one, cam).mapping_batch(views, cfg)
    # two ranks: views {0, 2} and {1}; the "all-reduce" adds the other rank's accumulated sum
    p_a, p_b = clone(), clone()
    e_a, e_b = FusedEngine(p_a, cam), FusedEngine(p_b, cam)
    other = {}
    e_b.loss_backward(*views[1], cfg, tracking=False)
    other['b'] = e_b.reduce_flat.clone()
    # (the exchanged buffer = a 16-float header -- slot 0 carries the rank's capacity flag, FusedEngine.exchange_gradients -- + the gradients)
    e_a.mapping_batch([views[0], views[2]], cfg, total_views=3, allreduce_sum=lambda red: red[red.numel() - other['b'].numel():].add_(other['b']))
    torch.cuda.synchronize()
    for k in ('means3D', 'rgb_colors', 'logit_opacities', 'log_scales'):
        ref = p_ref[k].detach()
        step = float((ref - params[k].detach()).abs().max())
        assert step > 0
        for got, name in ((p_one[k].detach(), "one process"), (p_a[k].detach(), "two ranks")):
            assert float((got - ref).abs().max()) <= 2e-3 * step, (k, name, float((got - ref).abs().max()), step)


@pytest.mark.parametrize("order", ["random", "scan"])
def test_order_hint_changes_nothing_but_speed(order, first_w2c=None):
    """SplatState.order_hint (bucket slots taken per (workgroup, tile) through an LDS table instead of one returning atomic per
    instance): same lists after the in-kernel sort, hence bit-identical renders, for a map in random order (most instances
    fall back to their own atomic) and for one in pixel-scan order (the case it is for)."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(30000, 320, 240, seed=31, first_w2c=first_w2c)
    if order == "scan":
        with torch.no_grad():
            z = params['means3D'][:, 2]
            key = torch.round(params['means3D'][:, 1] / z * 160.0 + 120.0) * 4096 + params['means3D'][:, 0] / z * 160.0
            perm = torch.argsort(key)
            for k in ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales'):
                params[k] = torch.nn.Parameter(params[k].detach()[perm].contiguous())
    cfg = slam.REPLICA_MAPPING
    outs = []
    for hint in (False, True):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.creation_order = hint
        eng.group_bins = False                                             # (group binning would take precedence over the hint)
        eng.loss_backward(frame, 1, cfg, tracking=False)
        assert not eng.check_overflow() and eng.tile_stride > 0           # learns the buckets
        eng.loss_backward(frame, 1, cfg, tracking=False)                  # bucketed lists: the hinted path
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        st = eng._workspace(False, with_ssim=False).st                    # the form of F1 the launch took: aggregated bucket slots or not
        assert bool(st.order_hint) == hint and st.tile_stride > 0 and st.group_stride == 0
        outs.append((eng.buf['out6'].clone(), eng.grads['means3D'].clone(), eng.loss()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert abs(outs[0][2] - outs[1][2]) <= 1e-6 * abs(outs[0][2])
    g0, g1 = outs
    assert float((g0[1] - g1[1]).abs().max()) <= 1e-5 * float(g0[1].abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("aniso", [False, True])
def test_mapping_step_without_gradient_stores_moves_the_map_the_same(aniso):
    """mapping_iteration(keep_grads=False): the fused Adam step takes the gradients from registers and nothing is written to
    ``eng.grads`` (the reference's loop discards them after the step, /root/reference/scripts/splatam.py:860-861).  Parameters and
    moments after three iterations equal those of the storing form to float-atomic summation order; the gradient buffers stay untouched."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 320, 240, aniso=aniso, seed=43)
    cfg = slam.REPLICA_MAPPING
    engs = []
    for keep in (True, False):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        for _ in range(3):
            eng.loss_backward(frame, 1, cfg, tracking=False)
            if not eng.check_overflow():
                break
        for g in eng.grads.values():
            g.fill_(123.0)
        for _ in range(3):
            eng.mapping_iteration(frame, 1, cfg, keep_grads=keep)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        engs.append(eng)
    a, b = engs
    assert all(float((g - 123.0).abs().max()) == 0.0 for g in b.grads.values())             # nothing was stored
    assert any(float((g - 123.0).abs().max()) > 0.0 for g in a.grads.values())
    for k in ('means3D', 'rgb_colors', 'logit_opacities', 'log_scales') + (('unnorm_rotations',) if aniso else ()):
        moved = float((a.params[k].detach() - params[k]).abs().max())
        assert moved > 0.0, k
        assert float((a.params[k].detach() - b.params[k].detach()).abs().max()) <= 2e-3 * moved + 1e-9, k
        assert float((a.exp_avg[k] - b.exp_avg[k]).abs().max()) <= 1e-4 * float(a.exp_avg[k].abs().max()) + 1e-12, k


def _bind_only(eng, only):
    """The engine's workspaces with only the map-gradient buffer ``only`` bound; a C caller may leave any of the five NULL
    (include/splat_hip.h: each is written when non-NULL)."""
    workspace = eng._workspace

    def bound(*args, **kw):
        ws = workspace(*args, **kw)
        for f in ('d_means3D', 'd_rgb_colors', 'd_unnorm_rotations', 'd_logit_opacities', 'd_log_scales'):
            if f != only:
                setattr(ws, f, None)
        return ws
    eng._workspace = bound


@pytest.mark.gpu
@pytest.mark.parametrize("mode,only", [("mapping", "d_means3D"), ("mapping", "d_log_scales"), ("one-kernel tracking", "d_means3D")])
def test_one_map_gradient_buffer_gives_what_all_five_give(mode, only):
    """splat_iter_loss_backward with ONE map-gradient buffer bound: the backward composite forms its sums in the form the per-Gaussian
    kernel reads them in (fused.hip: iter_sums), so the requested gradient and the report's pose gradient and loss equal those of the
    run with all five (anisotropic map: the scales' adjoint goes through the rotation)."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 320, 240, aniso=True, seed=57)
    out = {}
    for keep in (None, only):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False)
        assert not eng.check_overflow() and eng.tile_stride > 0
        if keep is not None:
            _bind_only(eng, keep)
        if mode == "mapping":
            eng.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False, do_ba=True)
        else:
            assert eng.track_fused and eng.track_fused_full and 0 < eng.max_list_hint <= 400     # (the one-kernel form with map gradients)
            eng.begin_tracking(1)
            eng.loss_backward(frame, 1, slam.REPLICA_TRACKING, tracking=True, map_grads=True)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        out[keep] = dict(d=eng.buf['d_cam'].clone(), grads={k: v.clone() for k, v in eng.grads.items()})
    a, b = out[only], out[None]
    assert abs(float(a['d'][7]) - float(b['d'][7])) <= 1e-6 * abs(float(b['d'][7]))
    assert float((a['d'][:7] - b['d'][:7]).abs().max()) <= 2e-5 * float(b['d'][:7].abs().max()), (a['d'][:7], b['d'][:7])
    if mode == "mapping":
        k = only[2:]
        sc = float(b['grads'][k].abs().max())
        assert sc > 0 and float((a['grads'][k] - b['grads'][k]).abs().max()) <= 5e-5 * sc, k


@pytest.mark.gpu
def test_mapping_step_without_colour_and_opacity_gradients_moves_the_rest_the_same():
    """splat_iter_mapping_step with SplatAdamMap.grad[1] and grad[3] NULL (torch skips parameters that have no gradient): means,
    rotations and scales and their moments move as in the step over all five groups; colours, opacities and their moments stay as
    they were, bit for bit."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 320, 240, aniso=True, seed=61)
    cfg = slam.REPLICA_MAPPING
    engs = []
    for skip in (False, True):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        for _ in range(3):
            eng.loss_backward(frame, 1, cfg, tracking=False)
            if not eng.check_overflow():
                break
        o = eng._adam_map_args(cfg['lrs'])
        if skip:
            o.grad[1] = o.grad[3] = None
        eng.loss_backward(frame, 1, cfg, tracking=False, map_adam=o, map_grads="step only")
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        engs.append(eng)
    a, b = engs
    for k in ('means3D', 'unnorm_rotations', 'log_scales'):
        moved = float((a.params[k].detach() - params[k]).abs().max())
        assert moved > 0.0, k
        assert float((a.params[k].detach() - b.params[k].detach()).abs().max()) <= 2e-3 * moved + 1e-9, k
        assert float((a.exp_avg[k] - b.exp_avg[k]).abs().max()) <= 1e-4 * float(a.exp_avg[k].abs().max()) + 1e-12, k
    for k in ('rgb_colors', 'logit_opacities'):
        assert float((a.params[k].detach() - params[k]).abs().max()) > 0.0, k
        assert torch.equal(b.params[k].detach(), params[k].detach().cuda()), k
        assert float(b.exp_avg[k].abs().max()) == 0.0 and float(b.exp_avg_sq[k].abs().max()) == 0.0, k


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one batch", "several batches", "exact lists"])
def test_staged_records_handed_to_the_backward_composite_change_nothing_but_speed(case):
    """SplatState.tile_recs: the forward composite leaves the staged 48-byte record of every list entry (pre-scaled conic, opacity,
    colours, centre, id, quadrant mask) and the backward composite re-stages its batches from them instead of gathering through the id
    and culling again.  Same records, same visit order: the planes are untouched and the gradients equal to float-atomic summation
    order, for lists of one 255-entry batch, of several, and on the exact (unbucketed) lists of an engine's first iteration."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    n = 15000 if case != "several batches" else 150000
    params, variables, frame, cam = _scene(n, 320, 240, seed=41)
    cfg = slam.REPLICA_MAPPING
    outs = []
    for recs in (0, 1):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.use_recs = recs
        if case != "exact lists":
            for _ in range(4):
                eng.loss_backward(frame, 1, cfg, tracking=False)
                if not eng.check_overflow():
                    break
            assert eng.tile_stride > 0
            assert (eng.max_list_hint > 400) == (case == "several batches"), eng.max_list_hint
        eng.loss_backward(frame, 1, cfg, tracking=False)
        torch.cuda.synchronize()
        ws = eng._workspace(False, with_ssim=False)
        assert bool(ws.st.tile_recs) == bool(recs)
        outs.append((eng.buf['out6'].clone(), {k: v.clone() for k, v in eng.grads.items()}, eng.loss()))
        # ... and the colour pass' own means2D gradient (one more backward composite over the same lists: it gathers) is the same too
        outs[-1][1]['means2D'] = eng.means2d_gradient().clone()
    assert torch.equal(outs[0][0], outs[1][0]) and abs(outs[0][2] - outs[1][2]) <= 1e-6 * abs(outs[0][2])
    for k in outs[0][1]:
        a, b = outs[0][1][k], outs[1][1][k]
        assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-12, k


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["random", "large", "odd_grid", "tracking"])
def test_group_binning_changes_nothing_but_speed(case, first_w2c=None):
    """SplatState.group_count (one record per (Gaussian, 2 x 2-tile group), slots through an LDS histogram; the forward composite
    filters its group's records by tile rectangle): the per-tile lists after the composite's sort are those of the per-tile
    buckets WITHOUT the entries whose tile cannot hold a pixel with alpha >= 1/255 (splat_math.h live_tile_rect: 12-13 % of the
    reference's instances at the SplaTAM workloads), hence bit-identical renders and list statistics that can only shrink.  "large": splats
    wide enough to touch more than four groups (a lane's further records take their own atomics); "odd_grid": an odd number of
    tile columns / rows (edge groups of one tile); "tracking": the composite with the loss epilogue, and the render-only call."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    W, H = (328, 232) if case == "odd_grid" else (320, 240)
    params, variables, frame, cam = _scene(30000 if case != "large" else 6000, W, H, seed=37, first_w2c=first_w2c)
    if case == "large":
        with torch.no_grad():
            params['log_scales'] += 1.5
    tracking = case == "tracking"
    cfg = slam.REPLICA_TRACKING if tracking else slam.REPLICA_MAPPING
    outs = []
    for groups in (False, True):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.group_bins = groups
        for attempt in range(4):                                          # (the wide splats outgrow the default list capacity once)
            eng.loss_backward(frame, 1, cfg, tracking=tracking)
            if not eng.check_overflow():
                break
        assert eng.tile_stride > 0                                         # learnt the buckets (and, with them, the groups)
        eng.loss_backward(frame, 1, cfg, tracking=tracking)
        torch.cuda.synchronize()
        stat = eng.buf['status'].tolist()
        assert not eng.check_overflow(grow=False)
        ws = eng._workspace(False, with_ssim=False)
        assert (ws.st.group_stride > 0) == groups
        grads = eng.grads['means3D'].clone() if not tracking else eng.buf['d_cam'][:7].clone()
        out6, loss = eng.buf['out6'].clone(), eng.loss()
        eng.render(frame, 1)                                               # forward half only: same lists, same planes
        torch.cuda.synchronize()
        assert torch.equal(eng.buf['out6'], out6)
        # counters consumed and reset (word 0 of each 128-byte counter line; word 1 of a group's line keeps its record count for a
        # later pass over the same records: splat_iter_time_kernel fn 2)
        from splatam_amd import _capi
        gc = eng.buf['group_count'].view(-1, _capi.SPLAT_COUNTER_STRIDE)
        assert float(eng.buf['tile_count'].abs().max()) == 0.0 and float(gc[:, 0].abs().max()) == 0.0 and float(gc[:, 2:].abs().max()) == 0.0
        outs.append((out6, grads, loss, stat[0], stat[2]))
    assert torch.equal(outs[0][0], outs[1][0])
    # list entries, longest list: group binning drops the instances that cannot blend -- some, never most of them
    assert 0.6 * outs[0][3] <= outs[1][3] <= outs[0][3] and 0.6 * outs[0][4] <= outs[1][4] <= outs[0][4], (outs[0][3:], outs[1][3:])
    assert outs[1][3] < outs[0][3]
    assert abs(outs[0][2] - outs[1][2]) <= 1e-6 * abs(outs[0][2])
    assert float((outs[0][1] - outs[1][1]).abs().max()) <= 2e-5 * float(outs[0][1].abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("aniso", [False, True])
def test_mapping_step_in_one_call_equals_loss_backward_plus_adam(aniso, first_w2c=None):
    """splat_iter_mapping_step (the Adam step of the map folded into the iteration's last kernel) against the two calls it replaces
    (splat_iter_loss_backward, splat_iter_adam_map), three iterations: same parameters and moments up to the summation order of
    the backward composite's float atomics (Adam with eps = 1e-15 turns a gradient that is rounding noise into a +-lr step, so
    elements are compared where the gradient is significant), and the loss / pose outputs of the folded F7."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine, PARAM_ORDER
    params, variables, frame, cam = _scene(8000, 208, 160, aniso=aniso, seed=11, first_w2c=first_w2c)
    cfg = slam.REPLICA_MAPPING
    e1 = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
    e2 = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
    g_first = None
    for it in range(3):
        e1.mapping_iteration(frame, 1, cfg)
        e2.loss_backward(frame, 1, cfg, tracking=False)
        if g_first is None:
            g_first = {k: e2.grads[k].clone() for k in PARAM_ORDER}
        e2.adam_map(cfg['lrs'])
        torch.cuda.synchronize()
        assert abs(e1.loss() - e2.loss()) <= 1e-6 * abs(e2.loss())
    assert not e1.check_overflow() and not e2.check_overflow()
    for k in PARAM_ORDER:
        assert float((e1.grads[k] - e2.grads[k]).abs().max()) <= 1e-3 * float(e2.grads[k].abs().max()) + 1e-12, k   # still written
        if k == 'unnorm_rotations' and not aniso:
            assert torch.equal(e1.params[k].detach(), params[k].detach()) and float(e1.exp_avg[k].abs().max()) == 0.0
            continue
        lr = cfg['lrs'][k]
        sig = g_first[k].abs() > 1e-4 * g_first[k].abs().max()
        diff = (e1.params[k].detach() - e2.params[k].detach()).abs()[sig]
        assert float((diff > 0.05 * lr).float().mean()) < 5e-3, (k, float(diff.max()), lr)
        dm = (e1.exp_avg[k] - e2.exp_avg[k]).abs()
        assert float(dm.max()) <= 1e-3 * float(e2.exp_avg[k].abs().max()), k
        dv = (e1.exp_avg_sq[k] - e2.exp_avg_sq[k]).abs()
        assert float(dv.max()) <= 2e-3 * float(e2.exp_avg_sq[k].abs().max()), k
    assert torch.equal(e1.params['cam_trans'], e2.params['cam_trans'])


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [False, True])
def test_stale_hint_with_bucketed_lists_is_flagged_and_memory_safe(groups):
    """Bucketed lists (and group records) whose host statistics have gone stale: tiles with more instances than the composite can
    sort itself (1 024) while the hint still says "short".  The composite truncates, flags the iteration for a re-run, and publishes
    the CLAMPED count -- the backward composite must never walk into list slots nobody wrote (poisoned here, as re-used allocator
    memory would be)."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(60000, 96, 64, seed=11)       # dense: several thousand instances per tile
    eng = FusedEngine(params, cam)
    eng.group_bins = groups
    cfg = slam.REPLICA_MAPPING
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow()
    assert eng.max_list_hint > 1024
    good, good_loss = eng.grads['means3D'].clone(), eng.loss()
    # stale statistics: "no list is longer than 100", buckets of 1 536 slots
    eng.max_list_hint, eng.tile_stride = 100, 1536
    if eng.tile_stride * eng.num_tiles > eng.capacity:
        eng._alloc_lists(eng.tile_stride * eng.num_tiles)
    eng.buf['point_list'].fill_(0x7f7f7f7f)
    eng.buf['keys'].fill_(0x7f7f7f7f7f7f7f7f)
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()                                            # no memory fault
    ws = eng._workspace(False, with_ssim=False)
    assert (ws.st.group_stride > 0) == groups
    assert eng.check_overflow()                                          # ... and the iteration is reported as invalid
    for _ in range(2):
        eng.loss_backward(frame, 1, cfg, tracking=False)                 # statistics reset by check_overflow: exact lists again
        torch.cuda.synchronize()
        assert not eng.check_overflow()
    assert abs(eng.loss() - good_loss) <= 1e-5 * abs(good_loss)
    _cmp(eng.grads['means3D'], good, "dL/dmeans3D after recovery", tol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("lists", ["exact", "learnt"])
@pytest.mark.parametrize("world", [2, 3])
def test_tile_row_sharded_tracking_equals_whole_frame_tracking(lists, world, first_w2c=None):
    """Tracking sharded over tile rows (SplatState.tile_row_begin / _end, splat_iter_finish): ``world`` engines holding the same map and
    pose each composite their band of the frame; their partial sums, added (what the all-reduce does), give the whole frame's loss
    and pose gradient; every rank then takes the same Adam step.  Against the whole-frame tracking loop over four iterations, with the
    exact lists of a fresh engine and with learnt bucketed lists / group records."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 328, 248, seed=53, first_w2c=first_w2c)        # 21 x 16 tiles: bands of 8 + 8 or 5 + 5 + 6 rows
    cfg = slam.REPLICA_TRACKING

    def engine():
        e = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        if lists == "learnt":
            e.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False)
            assert not e.check_overflow() and e.tile_stride > 0
        e.begin_tracking(1)
        return e
    full = engine()
    ranks = [engine() for _ in range(world)]
    bands = [e.tile_row_band(r, world) for r, e in enumerate(ranks)]
    assert bands[0][0] == 0 and bands[-1][1] == 16 and all(bands[r][1] == bands[r + 1][0] for r in range(world - 1))
    for it in range(4):
        # the whole-frame engine starts every iteration from the shards' pose and Adam state: the pose optimisation amplifies
        # rounding-level differences of the gradient (float-atomic summation order) ~10x per iteration on this scene (L1 kinks, mask
        # edges), which is a property of the objective, not of the sharding under test
        with torch.no_grad():
            full.params['cam_unnorm_rots'].copy_(ranks[0].params['cam_unnorm_rots'])
            full.params['cam_trans'].copy_(ranks[0].params['cam_trans'])
            full.buf['pose_state'].copy_(ranks[0].buf['pose_state'])
        full.tracking_iteration(frame, cfg)
        for r, e in enumerate(ranks):
            e.loss_backward(frame, e.track_time_idx, cfg, tracking=True, tile_rows=bands[r])
        total = sum(e.buf['sums'] for e in ranks)                          # the all-reduce
        for e in ranks:
            e.buf['sums'].copy_(total)
            e.finish_iteration(e._pose_adam_args(cfg))
        torch.cuda.synchronize()
        assert abs(ranks[0].loss() - full.loss()) <= 2e-6 * abs(full.loss()), (it, ranks[0].loss(), full.loss())
        g_full, g_shard = full.buf['d_cam'][:7], ranks[0].buf['d_cam'][:7]
        assert float((g_full - g_shard).abs().max()) <= 2e-5 * float(g_full.abs().max()), it
        for e in ranks[1:]:                                                # same sums -> the same step, bit for bit
            assert torch.equal(e.params['cam_unnorm_rots'], ranks[0].params['cam_unnorm_rots'])
            assert torch.equal(e.params['cam_trans'], ranks[0].params['cam_trans'])
        assert not full.check_overflow(grow=False) and all(not e.check_overflow(grow=False) for e in ranks)
    # a band's list statistics are not the frame's: check_overflow() learns nothing from them, a whole-frame render re-arms it
    e = ranks[0]
    hint, stride = e.max_list_hint, e.tile_stride
    assert e._stats_partial and not e.check_overflow() and (e.max_list_hint, e.tile_stride) == (hint, stride)
    e.relearn_lists(frame, 1)
    assert not e._stats_partial and e.tile_stride > 0 and e.max_list_hint > 0
    # Adam normalises the gradient: rounding-level differences of the sums stay rounding-level in the pose
    assert float((ranks[0].params["cam_trans"].detach() - full.params["cam_trans"].detach()).abs().max()) <= 2e-5
    assert float((ranks[0].params["cam_unnorm_rots"].detach() - full.params["cam_unnorm_rots"].detach()).abs().max()) <= 2e-5
    assert float(ranks[0].buf['tile_count'].abs().max()) == 0.0 and float(ranks[0].buf['accum'].abs().max()) == 0.0


def test_flagged_iterations_take_no_adam_step_and_are_counted():
    """A capacity flag raised on the device (per-tile lists that did not fit) holds back every Adam step until the host has dealt
    with it (include/splat_hip.h, d_cam[12]): the map, the pose, the moments and the best-candidate record stay as they were, d_cam[21]
    counts the iterations, settle() reports them (skipped_iterations), re-sizes the lists and takes the host-side step count back to
    where it stood before them; the loop then goes on."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(12000, 256, 192, seed=21)
    p = {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}
    eng = FusedEngine(p, cam)
    mcfg, tcfg = slam.REPLICA_MAPPING, slam.REPLICA_TRACKING
    for _ in range(2):
        eng.mapping_iteration(frame, 1, mcfg)
        assert not eng.check_overflow()
    assert eng.tile_stride > 0 and eng.skipped_iterations == 0
    good = (eng.tile_stride, eng.max_list_hint)
    snap = {k: v.detach().clone() for k, v in p.items()}
    m_snap = {k: eng.exp_avg[k].clone() for k in eng.exp_avg}
    steps_before = eng.map_step
    assert steps_before == 2
    eng.tile_stride, eng.max_list_hint = 64, 40                     # buckets far too small: every list overflows
    for _ in range(3):
        eng.mapping_iteration(frame, 1, mcfg)                       # Adam inside the per-Gaussian backward kernel: gated
    eng.loss_backward(frame, 1, mcfg, tracking=False)
    eng.adam_map(mcfg['lrs'])                                       # Adam as its own kernel: gated
    torch.cuda.synchronize()
    rep = eng.buf['d_cam'].cpu()
    assert float(rep[12]) == 1.0 and int(rep.view(torch.int32)[20]) == 1 and int(rep.view(torch.int32)[21]) == 4
    assert int(rep.view(torch.int32)[17]) == 1                      # the status snapshot: overflow
    for k in snap:
        assert torch.equal(p[k].detach(), snap[k]), k
    for k in m_snap:
        assert torch.equal(eng.exp_avg[k], m_snap[k]), k
    assert eng.map_step == steps_before + 4
    assert eng.settle("map") == 4 and eng.skipped_iterations == 4 and eng.tile_stride == 0
    assert eng.map_step == steps_before
    eng.mapping_iteration(frame, 1, mcfg)                           # exact lists: valid again, steps again
    assert eng.settle("map") == 0 and eng.map_step == steps_before + 1          # a clean phase: nothing is taken back
    assert eng.skipped_iterations == 0 and eng.tile_stride > 0
    assert not torch.equal(p['means3D'].detach(), snap['means3D'])
    # tracking: the pose's step rides in the last kernel of the iteration (and as a kernel of its own)
    eng.begin_tracking(1)
    eng.tracking_iteration(frame, tcfg)
    torch.cuda.synchronize()
    pose = (p['cam_unnorm_rots'].detach().clone(), p['cam_trans'].detach().clone(), eng.buf['pose_state'].clone())
    steps_before = eng.pose_step
    assert steps_before == 1
    eng.tile_stride, eng.max_list_hint = 64, 40
    eng.tracking_iteration(frame, tcfg)
    eng.loss_backward(frame, 1, tcfg, tracking=True)
    eng.adam_pose(tcfg['lrs']['cam_unnorm_rots'], tcfg['lrs']['cam_trans'])
    torch.cuda.synchronize()
    assert torch.equal(p['cam_unnorm_rots'].detach(), pose[0]) and torch.equal(p['cam_trans'].detach(), pose[1])
    assert torch.equal(eng.buf['pose_state'], pose[2])
    assert eng.settle("pose") == 2 and eng.skipped_iterations == 2
    assert eng.pose_step == steps_before
    eng.tracking_iteration(frame, tcfg)
    torch.cuda.synchronize()
    assert not torch.equal(p['cam_trans'].detach(), pose[1])
    assert eng.settle("pose") == 0 and eng.pose_step == steps_before + 1
    assert (eng.tile_stride, eng.max_list_hint)[0] > 0 and good[0] > 0


def test_sharded_tracking_flag_travels_with_the_sums_and_folded_sums_are_the_sums():
    """Tile-row-sharded tracking: a rank whose band overflowed adds to sums[31] (all-reduced with the partial sums), so that EVERY
    rank skips the Adam step of that iteration; and splat_iter_fold_sums leaves the totals of the 64 copies in copy 0."""
    from splatam_amd import _capi, slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(20000, 328, 248, seed=53)
    cfg = slam.REPLICA_TRACKING
    ranks = []
    for r in range(2):
        e = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        e.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False)
        assert not e.check_overflow() and e.tile_stride > 0
        e.begin_tracking(1)
        ranks.append(e)
    bands = [e.tile_row_band(r, 2) for r, e in enumerate(ranks)]
    ranks[1].tile_stride, ranks[1].max_list_hint = 64, 40           # rank 1's lists will not fit
    pose0 = ranks[0].params['cam_trans'].detach().clone()
    for r, e in enumerate(ranks):
        e.loss_backward(frame, 1, cfg, tracking=True, tile_rows=bands[r])
    # folded: copy 0 holds the totals, the others are zero
    raw = ranks[0].buf['sums'].clone().view(_capi.SPLAT_ITER_SUM_COPIES, _capi.SPLAT_ITER_SUMS)
    _capi.check(ranks[0].L.splat_iter_fold_sums(ranks[0].buf['sums'].data_ptr(), ranks[0]._stream()), "splat_iter_fold_sums")
    folded = ranks[0].buf['sums'].view(_capi.SPLAT_ITER_SUM_COPIES, _capi.SPLAT_ITER_SUMS)
    torch.cuda.synchronize()
    assert float(folded[1:].abs().max()) == 0.0
    assert float((folded[0] - raw.sum(0)).abs().max()) <= 1e-12 * float(raw.sum(0).abs().max())
    total = sum(e.buf['sums'] for e in ranks)                          # the all-reduce
    assert float(total[_capi.SPLAT_ITER_SUMS - 1]) == 1.0           # rank 1's flag
    for e in ranks:
        e.buf['sums'].copy_(total)
        e.finish_iteration(e._pose_adam_args(cfg))
    torch.cuda.synchronize()
    for e in ranks:                                                 # BOTH ranks held their step back
        assert torch.equal(e.params['cam_trans'].detach(), pose0)
        assert float(e.buf['d_cam'][12]) == 1.0


def test_tile_launch_order_changes_nothing_but_speed():
    """SplatState.tile_work / tile_order: the composites start the heaviest tiles of every XCD band first.  The order is a permutation
    of each band's tiles (the forward composite's own work estimates, descending), and a schedule only: the rendered planes are
    bit-identical with and without it, the gradients equal to float-atomic summation order."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(30000, 424, 312, seed=77)       # 27 x 20 = 540 tiles: bands of 68, the last one short
    cfg = slam.REPLICA_MAPPING
    res = {}
    for on in (True, False):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.tile_order_on = on
        for _ in range(3):                                          # exact lists, then learnt lists in the learnt order
            eng.loss_backward(frame, 1, cfg, tracking=False)
            assert not eng.check_overflow()
        torch.cuda.synchronize()
        res[on] = (eng.buf['out6'].clone(), {k: v.clone() for k, v in eng.grads.items()}, eng.loss(),
                   eng.buf['tile_order'].cpu().numpy().astype(np.int64) & 0xFFFFFFFF, eng.buf['tile_work'].cpu().numpy())
    T, per = 540, 68
    order, work = res[True][3], res[True][4]
    assert work.max() > 0
    for band in range(8):
        seg = order[band * per:(band + 1) * per]
        tiles = seg[seg != 0xFFFFFFFF] - 1                                      # (an entry holds tile + 1: zero = not written yet)
        lo, hi = band * per, min(T, (band + 1) * per)
        assert sorted(tiles.tolist()) == list(range(lo, hi)), band             # a permutation of the band's tiles
        assert (seg[len(tiles):] == 0xFFFFFFFF).all()
        w = work[tiles].astype(np.float64)
        bins = np.floor(w * 255.0 / max(work[lo:hi].max(), 1)).astype(int)
        assert (np.diff(bins) <= 0).all(), band                                 # heaviest first (to the sort's 256 bins)
    assert (res[False][3] == 0).all()                               # off: never touched (the zeroed buffer is the natural order)
    assert torch.equal(res[True][0], res[False][0])
    assert abs(res[True][2] - res[False][2]) <= 1e-6 * abs(res[False][2])
    for k in res[True][1]:
        a, b = res[True][1][k], res[False][1][k]
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-12, k


def test_every_view_keeps_its_own_launch_order():
    """Mapping draws another keyframe view every iteration: the order an iteration leaves is kept for the NEXT visit of ITS view (keyed
    by the frame's time index; the last 64 views), not handed to whichever view comes next.  Each view's buffer is a permutation built
    from that view's own work estimates; the planes do not depend on it."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(30000, 424, 312, seed=78)
    with torch.no_grad():                                           # a second view: the pose of time index 2 looks elsewhere
        params['cam_unnorm_rots'][0, :, 2] = torch.tensor([0.99, -0.03, 0.05, 0.01], device="cuda")
        params['cam_trans'][0, :, 2] = torch.tensor([-0.05, 0.04, 0.02], device="cuda")
    cfg = slam.REPLICA_MAPPING
    eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
    assert eng.order_per_view and eng.tile_order_on
    natural = eng._natural_order.clone()
    planes = {}
    for it in range(6):
        view = 1 + it % 2
        eng.loss_backward(frame, view, cfg, tracking=False)
        assert not eng.check_overflow()
        assert eng.buf['tile_order'] is eng._orders[view]
        planes[view] = eng.buf['out6'].clone()
    torch.cuda.synchronize()
    o1, o2 = eng._orders[1], eng._orders[2]
    assert o1.data_ptr() != o2.data_ptr() and len(eng._orders) == 2
    assert torch.equal(eng._natural_order, natural)                 # the natural order itself is never written
    assert not torch.equal(o1, natural) and not torch.equal(o2, natural) and not torch.equal(o1, o2)
    T_, per_ = 27 * 20, (27 * 20 + 7) // 8
    nat = torch.arange(8 * per_)
    want = torch.sort(torch.where(nat < T_, nat + 1, torch.full_like(nat, 0xFFFFFFFF))).values      # (entries hold tile + 1; 0xFFFFFFFF = no tile)
    assert int(natural.abs().max()) == 0                            # the natural order is the zeroed buffer
    for o in (o1, o2):
        assert torch.equal(torch.sort(o.view(torch.int32).long().cpu() & 0xFFFFFFFF).values, want)
    single = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
    single.order_per_view = False
    for it in range(6):
        view = 1 + it % 2
        single.loss_backward(frame, view, cfg, tracking=False)
        assert not single.check_overflow()
        if it >= 4:
            assert torch.equal(single.buf['out6'], planes[view]), view
    assert len(single._orders) == 0
    # bounded: the 65th view evicts the one visited longest ago
    for v in range(3, 3 + 64):
        eng._select_order(v)
    assert len(eng._orders) == 64 and 1 not in eng._orders and 2 not in eng._orders


@pytest.mark.parametrize("n,W,H,label", [(20000, 328, 248, "one batch per tile"), (64000, 328, 248, "two to three batches per tile"),
                                         (4000, 200, 120, "sparse: empty tiles, pixels outside the image")])
def test_tracking_composites_in_one_kernel_equal_the_two_kernels(n, W, H, label, first_w2c=None):
    """SplatLossConfig.fused_composite: the tracking iteration's forward composite, loss and backward composite as ONE kernel (the
    backward pass walks the batch the forward pass left in LDS; planes in registers) against the two-kernel form: rendered planes,
    gradient planes, final_T / n_contrib bit for bit (the forward pass is the same code), loss and pose gradient to float-atomic
    summation order; and, without the planes, the same tracking LOOP."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(n, W, H, seed=91, first_w2c=first_w2c)
    cfg = slam.REPLICA_TRACKING
    out = {}
    for fused in (True, False):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.track_fused = fused
        eng.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False)       # learn the lists (the composite sorts them itself)
        assert not eng.check_overflow() and eng.tile_stride > 0 and eng.max_list_hint * 5 // 4 <= 1024
        eng.begin_tracking(1)
        eng.loss_backward(frame, 1, cfg, tracking=True)                         # planes kept
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        assert eng._lc_keep.fused_composite == (2 if fused else 0)              # the form the launch took
        out[fused] = dict(out6=eng.buf['out6'].clone(), dplanes=eng.buf['dL_dout6'].clone(), T=eng.buf['final_T'].clone(),
                          nc=eng.buf['n_contrib'].clone(), d=eng.buf['d_cam'].clone(), longest=eng.max_list_hint)
        for _ in range(4):                                                      # the loop's own iterations: no planes
            eng.tracking_iteration(frame, cfg)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        assert eng._lc_keep.fused_composite == (1 if fused else 0)
        out[fused].update(rot=eng.params['cam_unnorm_rots'].detach().clone(), trans=eng.params['cam_trans'].detach().clone(), loss=eng.loss())
    a, b = out[True], out[False]
    print(label, "longest list", a['longest'])
    for k in ('out6', 'dplanes', 'T', 'nc'):
        assert torch.equal(a[k], b[k]), (label, k)
    assert abs(float(a['d'][7]) - float(b['d'][7])) <= 1e-6 * abs(float(b['d'][7]))
    assert float((a['d'][:7] - b['d'][:7]).abs().max()) <= 2e-5 * float(b['d'][:7].abs().max()), (a['d'][:7], b['d'][:7])
    assert float((a['d'][8:12] - b['d'][8:12]).abs().max()) <= 1e-5 * float(b['d'][8:12].abs().max())
    assert float((a['trans'] - b['trans']).abs().max()) <= 2e-5 and float((a['rot'] - b['rot']).abs().max()) <= 2e-5
    assert abs(a['loss'] - b['loss']) <= 1e-3 * abs(b['loss'])


@pytest.mark.parametrize("n,label", [(20000, "one batch per tile"), (64000, "two to three batches per tile")])
def test_full_gradient_tracking_in_one_kernel_equals_the_two_kernels(n, label):
    """The tracking iteration with EVERY gradient the reference's backward() forms (dL/d rgb, opacity, scale too: learning rate 0 in
    /root/reference/configs/replica/splatam.py:71-79): forward composite, loss and the backward composite's MAPPING form as one
    kernel (render_track_fused_full_kernel) against K6 + K7: planes bit for bit, loss, pose gradient and the map's gradients to
    float-atomic summation order."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(n, 328, 248, seed=92)
    cfg = slam.REPLICA_TRACKING
    out = {}
    for full in (True, False):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.track_fused_full = full
        eng.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False)
        assert not eng.check_overflow() and eng.tile_stride > 0
        eng.begin_tracking(1)
        eng.loss_backward(frame, 1, cfg, tracking=True, map_grads=True)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        out[full] = dict(out6=eng.buf['out6'].clone(), dplanes=eng.buf['dL_dout6'].clone(), d=eng.buf['d_cam'].clone(),
                         grads={k: v.clone() for k, v in eng.grads.items()})
        # ... and with the pose's Adam step riding along, no planes (bench.py's tracking_full_gradients figure)
        for _ in range(3):
            eng.loss_backward(frame, 1, cfg, tracking=True, map_grads=True, pose_adam=eng._pose_adam_args(cfg))
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        out[full].update(trans=eng.params['cam_trans'].detach().clone(), g2={k: v.clone() for k, v in eng.grads.items()})
    a, b = out[True], out[False]
    assert torch.equal(a['out6'], b['out6']) and torch.equal(a['dplanes'], b['dplanes']), label
    assert abs(float(a['d'][7]) - float(b['d'][7])) <= 1e-6 * abs(float(b['d'][7]))
    assert float((a['d'][:7] - b['d'][:7]).abs().max()) <= 2e-5 * float(b['d'][:7].abs().max())
    for key in ('grads', 'g2'):
        for k in ('rgb_colors', 'logit_opacities', 'log_scales'):
            sc = float(b[key][k].abs().max())
            assert sc > 0 and float((a[key][k] - b[key][k]).abs().max()) <= 5e-5 * sc, (label, key, k)
    assert float((a['trans'] - b['trans']).abs().max()) <= 2e-5


def _offset_view(t):
    """The same values in a contiguous tensor whose first element is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("W,H", [(320, 240), (64, 48), (44, 20)])
def test_mapping_loss_planes_do_not_depend_on_the_alignment_of_the_frame(W, H):
    """F4 / F5 move a thread's four pixels as one float4 when the width is a multiple of 4 and every plane is 16-byte aligned, and
    pixel by pixel otherwise (a caller's frame may be any contiguous view).  Same arithmetic either way: the gradient planes
    are bit-identical, the loss agrees to the order of its float64 partial sums."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(4000, W, H, seed=71)
    cfg = slam.REPLICA_MAPPING
    out = []
    for shifted in (False, True):
        fr = dict(frame)
        if shifted:
            fr['im'], fr['depth'] = _offset_view(frame['im']), _offset_view(frame['depth'])
        eng = FusedEngine(params, cam)
        eng.loss_backward(fr, 1, cfg, tracking=False)
        torch.cuda.synchronize()
        out.append((eng.loss(), eng.buf['dL_dout6'].clone(), eng.grad_flat.clone()))
    assert abs(out[0][0] - out[1][0]) <= 1e-6 * abs(out[0][0])
    assert torch.equal(out[0][1], out[1][1])
    scale = float(out[0][2].abs().max())
    assert float((out[0][2] - out[1][2]).abs().max()) <= 1e-5 * scale          # (float atomics of the backward composite)


@pytest.mark.parametrize("W,H", [(1200, 680), (203, 117), (40, 24), (33, 25), (9, 7)])
def test_ssim_loss_and_gradient_planes_against_torch(W, H):
    """F4 + F5 against the reference-shaped loss (slam.get_loss on torch: conv2d with the 11x11 window, zero padding) as seen at the
    rasterizer boundary: dL/d(rendered image), dL/d(rendered depth).  Sizes: the bench frame; not a multiple of the 32x24 SSIM tile
    nor of 4; one tile exactly; one pixel past a tile in both directions; smaller than the window."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    n = 20000 if W >= 1000 else 1500
    params, variables, frame, cam = _scene(n, W, H, seed=83)
    cfg = slam.REPLICA_MAPPING
    eng = FusedEngine(params, cam)
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    planes = eng.rendered()                     # what the fused forward composite produced: (im, depth, silhouette, depth_sq)
    im = planes[0].detach().clone().requires_grad_(True)
    depth = planes[1].detach().clone().requires_grad_(True)
    mask = (frame['depth'] > 0)                 # ignore_outlier_depth_loss is off in REPLICA_MAPPING; nan_mask is all-true here
    l_depth = torch.abs(frame['depth'] - depth)[mask].mean()
    l_im = 0.8 * torch.abs(im - frame['im']).mean() + 0.2 * (1.0 - slam.calc_ssim(im, frame['im']))
    loss = cfg['loss_weights']['im'] * l_im + cfg['loss_weights']['depth'] * l_depth
    loss.backward()
    assert abs(eng.loss() - float(loss)) <= 1e-5 * abs(float(loss)), (eng.loss(), float(loss))
    g = eng.buf['dL_dout6'].view(6, H, W)
    for got, ref, what in ((g[0:3], im.grad, "dL/dim"), (g[3:4], depth.grad, "dL/ddepth")):
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        # |x - y| has a kink at x == y: where the rendered colour equals the frame's to the last bit the two sides may pick
        # different subgradients; nowhere else may the planes differ by more than float32 evaluation order
        kink = (got - ref).abs() > 1e-4 * scale
        assert err <= 1e-4 * scale or int(kink.sum()) <= 2, (what, err, scale, int(kink.sum()))
