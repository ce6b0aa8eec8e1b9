"""The five places where the device turns get_loss' flags into a loss and gradient planes -- the forward composite's TRACK epilogue
(K6), the one-kernel tracking composites (pose-only and full-gradient), F3 track_loss_kernel<4 / 1>, F4 / F5 (mapping) and F7
(pose_finish_kernel, which combines the sums) -- at EVERY configuration get_loss accepts, not the shipped three.

How: the loss is checked on THE ENGINE'S OWN rendered planes against tests/loss_ref.py (pinned to slam.get_loss by
tests/test_loss_ref_cpu.py), where every mask decision is a float32 comparison both sides take identically: tracking gradient
planes match exactly, the report to the order of its sums.  Everything behind the gradient planes (backward composite, F6, the pose
sums) is linear in them and does not read the configuration: it is checked by feeding the engine's own planes as cotangents to the
reference-shaped path on the drop-in rasterizer.  No loss threshold can flip there: the masks are already inside the planes.

Scenes: tests/test_gpu_fused._scene with the frame edited so that every flag changes the mask (``edit_scene``).  NaN ground-truth
depth is left out: with outlier rejection it makes torch.median NaN (a rendered NaN stays with tests/test_loss_ref_cpu.py and
tests/test_host_math.py: these scenes cannot produce one).  In tracking the device forms no mask count (nothing divides by it):
SPLAT_REPORT_SUMS[2] is compared in mapping and is 0 in tracking.

Every test prints "LOSSCFG <site> | <configuration> | worst report ratio" (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from tests import loss_ref as LR

pytestmark = pytest.mark.gpu

SPARSE = (4000, 200, 120)           # silhouette holes, empty tiles; HW % 4 == 0, 16-byte rows: F3 <4>, F4 / F5 with float4
ONE_BATCH = (20000, 328, 248)       # the one-kernel forms' own size (learnt lists, max_list_hint * 5 / 4 <= 1024)
ODD = (3000, 203, 117)              # HW odd: F3 <1>, F4 / F5 pixel by pixel
ROW_ENDS = (3000, 70, 46)           # HW % 4 == 0, W % 4 != 0: F3 <4> with float4s that straddle row ends
SEED = 57
REPORT_RTOL = 1e-5                  # a device loss against a torch restatement (test_ssim_loss_and_gradient_planes_against_torch)
SENTINEL = 7.0                      # what the gradient planes hold before the iteration: a pixel no kernel wrote shows


def edit_scene(params, frame, W, H):
    """In place, on any device.  The frame: _scene's H/8 x W/8 patch of zero depth stays (but for pixel 0, valid again: the first
    element of every plane takes part); a few pixels of NEGATIVE depth; the two gross-outlier patches of
    test_ignore_outlier_depth_loss scaled to the frame.  The map: the Gaussians that project into a window of the lower right
    quadrant turn transparent AFTER the frame was rendered from them, so that the engine's silhouette has a hole where the frame
    has valid depth (synthetic_frame gives depth 0 wherever the frame's own silhouette is <= 0.5: without the window, valid depth
    under a silhouette <= 0.5 is a few edge pixels)."""
    d = frame['depth'] = frame['depth'].clone()
    d[:, 100 * H // 240:140 * H // 240, 60 * W // 320:140 * W // 320] *= 4.0
    d[:, 10 * H // 240:20 * H // 240, 200 * W // 320:260 * W // 320] += 6.0
    d[0, 3 * H // 10, W // 2:W // 2 + 6] = -1.5
    d[0, 3 * H // 10 + 2, W // 2:W // 2 + 6] *= -1.0
    d[0, 0, 0] = 2.0
    with torch.no_grad():
        m = params['means3D']
        u, v = 0.5 * W * m[:, 0] / m[:, 2] + W / 2 - 0.5, 0.5 * W * m[:, 1] / m[:, 2] + H / 2 - 0.5
        inside = (u >= 0.55 * W) & (u < 0.78 * W) & (v >= 0.62 * H) & (v < 0.88 * H)
        params['logit_opacities'][inside] = -12.0
    return int(inside.sum())


@functools.lru_cache(maxsize=None)
def _loss_scene(n, W, H):
    """One scene per size for the whole file: no test steps or edits it."""
    from tests.test_gpu_fused import _scene
    params, variables, frame, cam = _scene(n, W, H, seed=SEED)
    assert edit_scene(params, frame, W, H) > 0
    return params, variables, frame, cam


def assert_guards(out6, depth, cfg):
    """No comparison passes on an empty set: on the ENGINE'S planes at least 1 % of the pixels have gt <= 0, at least 1 % valid depth
    under a silhouette <= the threshold, and with outlier rejection at least 0.5 % are rejected as outliers."""
    gt, rd, sil = depth.reshape(-1).float().cpu(), out6[3].reshape(-1).float().cpu(), out6[4].reshape(-1).float().cpu()
    n = gt.numel()
    assert int((gt <= 0).sum()) >= 0.01 * n and int((gt < 0).sum()) >= 6, (int((gt <= 0).sum()), n)
    below = (gt > 0) & ~(sil > torch.tensor(cfg['sil_thres'], dtype=torch.float32))
    assert int(below.sum()) >= 0.01 * n, (int(below.sum()), n, cfg['sil_thres'])
    assert not torch.isnan(out6.float().cpu()).any() and not torch.isnan(gt).any()
    if cfg['ignore_outlier_depth_loss']:
        err = (gt - rd).abs() * (gt > 0)
        rejected = (gt > 0) & ~(err < 10 * err.median())
        assert int(rejected.sum()) >= 0.005 * n, (int(rejected.sum()), n)


def _report(eng):
    from splatam_amd import _capi as A
    d = eng.buf['d_cam'].detach().cpu().numpy().copy()
    return dict(d=d, sums=d[A.SPLAT_REPORT_SUMS:A.SPLAT_REPORT_SUMS + 4], loss=d[A.SPLAT_REPORT_LOSS], depth_term=d[A.SPLAT_REPORT_DEPTH_TERM],
                im_term=d[A.SPLAT_REPORT_IM_TERM], median=d[A.SPLAT_REPORT_MEDIAN], pose=d[0:7])


def check_report(rep, ref, cfg, tracking, site):
    """SPLAT_REPORT_SUMS[0..2], LOSS, DEPTH_TERM, IM_TERM against the float64 restatement; returns the worst ratio."""
    ratios = dict(depth_l1=LR.rel(rep['sums'][0], ref['depth_l1']), im_l1=LR.rel(rep['sums'][1], ref['im_l1']),
                  loss=LR.rel(rep['loss'], ref['loss']), im_term=LR.rel(rep['im_term'], ref['im_term']))
    if tracking:
        assert rep['sums'][2] == 0.0                          # (no count is formed in tracking: see the module docstring)
    else:
        assert rep['sums'][2] == float(ref['count']), (site, rep['sums'][2], ref['count'])       # an integer below 2^24: exact
    if cfg['use_l1']:
        ratios['depth_term'] = LR.rel(rep['depth_term'], ref['depth_term'])
    else:
        assert rep['depth_term'] == 0.0 and rep['loss'] == rep['im_term'], (site, rep['depth_term'], rep['loss'], rep['im_term'])
    worst = max(ratios.values())
    print(f"LOSSCFG {site} | {'tracking' if tracking else 'mapping'} {LR.cfg_id(cfg)} | worst report ratio {worst:.2e} "
          f"({max(ratios, key=ratios.get)})")
    assert ref['depth_l1'] > 0 and ref['im_l1'] > 0 and ref['count'] > 0
    assert worst <= REPORT_RTOL, (site, LR.cfg_id(cfg), ratios)
    return worst


def check_tracking_planes(planes, ref, cfg, site):
    """dL_dout6 planes 0..3 == the restatement's cast to float32, elementwise (both sides give 0 where the argument of abs is exactly
    zero); planes 4 and 5 all zero; without the depth term plane 3 all zero."""
    got, want = planes.detach().cpu().numpy(), LR.tracking_planes_f32(ref)
    assert not (got[4:] != 0).any(), site
    bad = np.argwhere(got[0:4] != want[0:4])
    assert bad.shape[0] == 0, (site, LR.cfg_id(cfg), bad.shape[0], bad[:5], [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])
    if not cfg['use_l1']:
        assert not (got[3] != 0).any(), site
    else:
        assert (np.abs(got[3]) == np.float32(LR.W_DEPTH)).any()
    assert (np.abs(got[0:3]) == np.float32(LR.W_IM)).any()


def dropin_backward(params, frame, cam, g, tracking, do_ba=False):
    """The reference-shaped path behind the gradient planes, on the drop-in rasterizer: transform_to_frame with get_loss' grad flags,
    the two render-variable dicts, two Renderer calls, and the planes ``g`` as cotangents of (im, depth)."""
    from splatam_amd import slam
    for p in params.values():
        p.grad = None
    gg, cg = LR.grad_flags(tracking, do_ba)
    tg = slam.transform_to_frame(params, 1, gaussians_grad=gg, camera_grad=cg)
    rv = slam.transformed_params2rendervar(params, tg)
    dv = slam.transformed_params2depthplussilhouette(params, frame['w2c'], tg)
    im, _, _ = slam.Renderer(raster_settings=cam)(**rv)
    depth_sil, _, _ = slam.Renderer(raster_settings=cam)(**dv)
    g = g.detach()
    ((im * g[0:3]).sum() + (depth_sil[0] * g[3]).sum()).backward()
    torch.cuda.synchronize()
    out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in params.items()}
    for p in params.values():
        p.grad = None
    return out


def check_pose(pose, g_ref, site):
    """d_cam[0:7] against the pose gradients: 1e-3 of the larger component, rotation and translation apart (test_tracking_loss_and_pose_gradient)."""
    gq, gt = g_ref['cam_unnorm_rots'][0, :, 1].cpu().numpy(), g_ref['cam_trans'][0, :, 1].cpu().numpy()
    assert np.abs(gq).max() > 0 and np.abs(gt).max() > 0 and np.isfinite(pose).all(), site
    assert np.abs(pose[0:4] - gq).max() <= 1e-3 * np.abs(gq).max(), (site, pose[0:4], gq)
    assert np.abs(pose[4:7] - gt).max() <= 1e-3 * np.abs(gt).max(), (site, pose[4:7], gt)


def check_map(eng, g_ref, site):
    """eng.grads against the map gradients through test_gpu_fused._cmp: 1e-3 of the tensor's maximum, 2e-4 outliers."""
    from tests.test_gpu_fused import _cmp
    for k in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
        assert float(g_ref[k].abs().max()) > 0, (site, k)
        _cmp(eng.grads[k], g_ref[k], f"{site} {k}")


def _tracking_engine(params, cam, frame, learn, **flags):
    """A fresh engine, its gradient planes at the sentinel; ``learn``: one mapping iteration first, so that the composite sorts its
    (bucketed) lists itself -- what the one-kernel forms need."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    eng = FusedEngine(params, cam)
    for k, v in flags.items():
        assert hasattr(eng, k)
        setattr(eng, k, v)
    if learn:
        eng.loss_backward(frame, 1, slam.REPLICA_MAPPING, tracking=False)
        assert not eng.check_overflow() and eng.tile_stride > 0 and eng.max_list_hint * 5 // 4 <= 1024
    eng.begin_tracking(1)
    eng.buf['dL_dout6'][0:4].fill_(SENTINEL)
    return eng


NO_REJECTION = [c for c in LR.TRACKING_CONFIGS if not c['ignore_outlier_depth_loss']]
REJECTION = [c for c in LR.TRACKING_CONFIGS if c['ignore_outlier_depth_loss']]


@pytest.mark.parametrize("size", [SPARSE, ONE_BATCH], ids=lambda s: f"{s[1]}x{s[2]}")
@pytest.mark.parametrize("cfg", NO_REJECTION, ids=LR.cfg_id)
def test_tracking_without_rejection_in_every_form(cfg, size):
    """use_sil_for_loss x use_l1 at weights 0.37 / 1.9 through (a) the K6 epilogue on exact and on learnt lists, (b) the one-kernel
    composite with planes, (c) the full-gradient one-kernel composite, (d) the one-kernel composite without planes (its report and
    pose gradient against (a)'s at the bounds of test_tracking_composites_in_one_kernel_equal_the_two_kernels)."""
    n, W, H = size
    params, variables, frame, cam = _loss_scene(n, W, H)
    forms = (("K6 epilogue, exact lists", False, dict(track_fused=False), {}),
             ("K6 epilogue, learnt lists", True, dict(track_fused=False), {}),
             ("one-kernel", True, dict(track_fused=True), {}),
             ("one-kernel full-gradient", True, dict(track_fused=True, track_fused_full=True), dict(map_grads=True)))
    g_ref, first = None, None
    for site, learn, flags, kw in forms:
        eng = _tracking_engine(params, cam, frame, learn, **flags)
        eng.loss_backward(frame, 1, cfg, tracking=True, **kw)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        assert eng._lc_keep.fused_composite == (2 if flags['track_fused'] else 0), site
        if kw:
            assert 0 < eng.max_list_hint <= 400                # (the full-gradient form is taken, not K6 + K7)
        out6, planes = eng.buf['out6'].clone(), eng.buf['dL_dout6'].clone()
        assert_guards(out6, frame['depth'], cfg)
        ref = LR.loss_from_planes(out6, frame['im'], frame['depth'], cfg, tracking=True)
        check_tracking_planes(planes, ref, cfg, site)
        rep = _report(eng)
        check_report(rep, ref, cfg, True, site)
        if g_ref is None:                                       # (the planes are the restatement's in every form: one reference)
            g_ref, first = dropin_backward(params, frame, cam, planes, tracking=True), rep
        check_pose(rep['pose'], g_ref, site)
        if kw:      # ... and the gradients the reference's backward() forms for the map in tracking too (rgb, opacity, scale: no transform_to_frame between)
            from tests.test_gpu_fused import _cmp
            for k in ("rgb_colors", "logit_opacities", "log_scales"):
                assert float(g_ref[k].abs().max()) > 0
                _cmp(eng.grads[k], g_ref[k], f"{site} {k}")
    # (d) no planes: fused_composite 1
    eng = _tracking_engine(params, cam, frame, True, track_fused=True)
    eng.loss_backward(frame, 1, cfg, tracking=True, keep_planes=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False) and eng._lc_keep.fused_composite == 1
    rep = _report(eng)
    assert abs(float(rep['loss']) - float(first['loss'])) <= 1e-6 * abs(float(first['loss']))
    assert float(np.abs(rep['pose'] - first['pose']).max()) <= 2e-5 * float(np.abs(first['pose']).max()), (rep['pose'], first['pose'])
    for k in ('depth_term', 'im_term'):
        assert abs(float(rep[k]) - float(first[k])) <= 1e-6 * abs(float(first[k])), k
    assert abs(float(rep['sums'][0]) - float(first['sums'][0])) <= 1e-6 * abs(float(first['sums'][0]))
    assert abs(float(rep['sums'][1]) - float(first['sums'][1])) <= 1e-6 * abs(float(first['sums'][1]))
    if not cfg['use_l1']:
        assert rep['depth_term'] == 0.0 and rep['loss'] == rep['im_term']
    assert (eng.buf['dL_dout6'][0:4] == SENTINEL).all()         # (really no planes)


def _f3_run(params, cam, fr, cfg):
    eng = _tracking_engine(params, cam, fr, False)
    eng.loss_backward(fr, 1, cfg, tracking=True)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    return eng


@pytest.mark.parametrize("size", [SPARSE, ODD, ROW_ENDS], ids=lambda s: f"{s[1]}x{s[2]}")
@pytest.mark.parametrize("cfg", REJECTION, ids=LR.cfg_id)
def test_tracking_with_rejection_through_the_loss_kernel(cfg, size):
    """Outlier rejection sends tracking through F3: track_loss_kernel<4> at 200x120, <1> at 203x117 (HW odd), <4> across row ends at
    70x46.  With use_sil_for_loss off the colour is masked by the outlier mask alone.  SPLAT_REPORT_MEDIAN is torch.median on the
    engine's own plane, bit for bit."""
    n, W, H = size
    params, variables, frame, cam = _loss_scene(n, W, H)
    eng = _f3_run(params, cam, frame, cfg)
    vec = (H * W) % 4 == 0
    for t in (eng.buf['out6'], eng.buf['dL_dout6'], frame['im'], frame['depth']):
        assert t.data_ptr() % 16 == 0                           # (with HW % 4 == 0: the float4 form)
    site = f"F3 V={4 if vec else 1}" + (" across row ends" if vec and W % 4 else "")
    out6, planes = eng.buf['out6'].clone(), eng.buf['dL_dout6'].clone()
    assert_guards(out6, frame['depth'], cfg)
    ref = LR.loss_from_planes(out6, frame['im'], frame['depth'], cfg, tracking=True)
    rep = _report(eng)
    gt = frame['depth']
    med = (torch.abs(gt - out6[3:4]) * (gt > 0)).median()
    assert float(rep['median']) == float(med) == float(ref['median'])
    check_tracking_planes(planes, ref, cfg, site)
    check_report(rep, ref, cfg, True, site)
    check_pose(rep['pose'], dropin_backward(params, frame, cam, planes, tracking=True), site)


@pytest.mark.parametrize("cfg", [c for c in REJECTION if c['use_l1']], ids=LR.cfg_id)
def test_loss_kernel_planes_do_not_depend_on_the_alignment_of_the_frame(cfg):
    """F3 takes its float4 form only when HW % 4 == 0 AND the rendered planes, the gradient planes and the frame's im and depth all
    start on 16 bytes (a caller's frame may be any contiguous view), its scalar form otherwise.  Same arithmetic either way: the
    gradient planes are bit-identical, sums and loss agree to the order of the float64 partial sums."""
    from tests.test_gpu_fused import _offset_view
    n, W, H = SPARSE
    params, variables, frame, cam = _loss_scene(n, W, H)
    out = []
    for shifted in (False, True):
        fr = dict(frame)
        if shifted:
            fr['im'], fr['depth'] = _offset_view(frame['im']), _offset_view(frame['depth'])
            assert fr['im'].data_ptr() % 16 == 4 and fr['depth'].data_ptr() % 16 == 4
        eng = _f3_run(params, cam, fr, cfg)
        out.append((_report(eng), eng.buf['dL_dout6'].clone(), eng.buf['out6'].clone()))
    (ra, pa, oa), (rb, pb, ob) = out
    assert torch.equal(oa, ob) and torch.equal(pa, pb)
    assert not (pb[0:4] == SENTINEL).any()
    assert ra['median'] == rb['median']
    for k in ('loss', 'depth_term', 'im_term'):
        assert abs(float(ra[k]) - float(rb[k])) <= 1e-6 * abs(float(ra[k])), k
    for k in (0, 1):
        assert abs(float(ra['sums'][k]) - float(rb['sums'][k])) <= 1e-6 * abs(float(ra['sums'][k])), k
    assert float(np.abs(ra['pose'] - rb['pose']).max()) <= 2e-5 * float(np.abs(ra['pose']).max())
    # ... and the shifted run is right, not merely the same
    ref = LR.loss_from_planes(ob, frame['im'], frame['depth'], cfg, tracking=True)
    check_tracking_planes(pb, ref, cfg, "F3 V=1 (frame 4 bytes past a 16-byte boundary)")
    check_report(rb, ref, cfg, True, "F3 V=1 (frame 4 bytes past a 16-byte boundary)")


def _mapping_run(params, cam, frame, cfg, do_ba=False):
    from splatam_amd.fused import FusedEngine
    eng = FusedEngine(params, cam)
    eng.buf['dL_dout6'][0:4].fill_(SENTINEL)
    eng.loss_backward(frame, 1, cfg, tracking=False, do_ba=do_ba)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    return eng


def check_mapping_planes(planes, ref, cfg, site):
    """Depth plane: one float32 division, within 1e-6 relative (HIP's default divide: 2.5 ulp, 3e-7) and zero exactly where the
    restatement's is; colour planes: 1e-4 of the plane's maximum with at most two kink pixels; planes 4 and 5 all zero."""
    got, want = planes.detach().cpu().numpy().astype(np.float64), ref['g'].numpy()
    assert not (got[4:] != 0).any() and np.isfinite(got).all(), site
    assert ((got[3] == 0) == (want[3] == 0)).all(), site
    assert (np.abs(got[3] - want[3]) <= 1e-6 * np.abs(want[3])).all(), (site, float(np.abs(got[3] - want[3]).max()))
    if cfg['use_l1']:
        assert (want[3] != 0).any()
    else:
        assert not (got[3] != 0).any(), site
    LR.colour_planes_close(got[0:3], want[0:3], site)


@pytest.mark.parametrize("size", [SPARSE, ODD], ids=lambda s: f"{s[1]}x{s[2]}")
@pytest.mark.parametrize("cfg", LR.MAPPING_CONFIGS, ids=LR.cfg_id)
def test_mapping_configs(cfg, size):
    """use_l1 x ignore_outlier_depth_loss through F4 / F5 (float4 form at 200x120, pixel by pixel at 203x117) and F7's mapping
    branch; and once more with use_sil_for_loss set, which is read only when tracking: planes and report bit-equal."""
    n, W, H = size
    params, variables, frame, cam = _loss_scene(n, W, H)
    site = "F4/F5 " + ("float4" if W % 4 == 0 else "scalar")
    eng = _mapping_run(params, cam, frame, cfg)
    out6, planes = eng.buf['out6'].clone(), eng.buf['dL_dout6'].clone()
    assert_guards(out6, frame['depth'], cfg)
    ref = LR.loss_from_planes(out6, frame['im'], frame['depth'], cfg, tracking=False)
    rep = _report(eng)
    if cfg['ignore_outlier_depth_loss']:
        assert float(rep['median']) == float(ref['median'])
    check_mapping_planes(planes, ref, cfg, site)
    check_report(rep, ref, cfg, False, site)
    assert not rep['pose'].any()                                # (no camera gradient without do_ba)
    check_map(eng, dropin_backward(params, frame, cam, planes, tracking=False), site)
    # the silhouette flag (at a threshold that would cut: the guard above holds for it) changes nothing in mapping
    cfg_sil = dict(cfg, use_sil_for_loss=True)
    eng2 = _mapping_run(params, cam, frame, cfg_sil)
    assert torch.equal(eng2.buf['out6'], out6) and torch.equal(eng2.buf['dL_dout6'], planes)
    rep2 = _report(eng2)
    for k in ('loss', 'depth_term', 'im_term', 'median'):
        assert rep2[k] == rep[k] or (np.isnan(rep2[k]) and np.isnan(rep[k])), k
    assert (rep2['sums'][0:3] == rep['sums'][0:3]).all()


def test_mapping_with_do_ba_forms_pose_and_map_gradients():
    """do_ba: get_loss lets gradient through BOTH sides of transform_to_frame.  The loss and its planes are the mapping ones; the
    pose gradient and the map's gradients are both non-zero and both match the reference-shaped path on the engine's planes."""
    n, W, H = SPARSE
    params, variables, frame, cam = _loss_scene(n, W, H)
    cfg = LR.MAPPING_CONFIGS[0]
    assert cfg['use_l1'] and not cfg['ignore_outlier_depth_loss']
    plain = _mapping_run(params, cam, frame, cfg)
    eng = _mapping_run(params, cam, frame, cfg, do_ba=True)
    out6, planes = eng.buf['out6'].clone(), eng.buf['dL_dout6'].clone()
    assert_guards(out6, frame['depth'], cfg)
    assert torch.equal(planes, plain.buf['dL_dout6']) and torch.equal(out6, plain.buf['out6'])
    ref = LR.loss_from_planes(out6, frame['im'], frame['depth'], cfg, tracking=False, do_ba=True)
    check_mapping_planes(planes, ref, cfg, "F4/F5 do_ba")
    rep = _report(eng)
    check_report(rep, ref, cfg, False, "F4/F5 do_ba")
    g_ref = dropin_backward(params, frame, cam, planes, tracking=False, do_ba=True)
    check_pose(rep['pose'], g_ref, "do_ba")
    check_map(eng, g_ref, "do_ba")
    assert not _report(plain)['pose'].any() and rep['pose'].any()
