"""tests/loss_ref.py (the restatement of get_loss from rendered planes that tests/test_gpu_loss_configs.py holds the loss kernels to)
pinned to slam.get_loss itself -- which tests/golden/ pins to the reference -- with the two renders replaced by given planes: the
hand-placed pixels of tests/util.track_pixel_planes (NaN render, silhouette at / either side of the threshold, kinks, either side of
10 x median), at every configuration the GPU file runs.  CPU only."""
import numpy as np
import pytest
import torch

from tests import loss_ref as LR
from tests.util import PlanesRenderer, track_pixel_planes

H, W = 16, 32


def _get_loss_on_planes(monkeypatch, out6, gt_im, gt, cfg, tracking, do_ba):
    """slam.get_loss (float32 torch) with the planes as its two renders: loss, weighted terms, dL/d(im), dL/d(depth_sil)."""
    from splatam_amd import slam
    params, variables = slam.synthetic_params(4, W, H, 30.0, 30.0, W / 2, H / 2, num_frames=2, seed=0, device="cpu")
    cam = slam.setup_camera(W, H, [[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]], np.eye(4), device="cpu")
    monkeypatch.setattr(slam, 'Renderer', PlanesRenderer)
    frame = {'cam': cam, 'im': gt_im.reshape(3, H, W), 'depth': gt.reshape(1, H, W), 'id': 1, 'w2c': torch.eye(4)}
    im = out6[:3].reshape(3, H, W).clone().requires_grad_(True)
    depth_sil = out6[3:].reshape(3, H, W).clone().requires_grad_(True)
    PlanesRenderer.planes = [im, depth_sil]
    loss, _, wl = slam.get_loss(params, frame, dict(variables), 1, cfg['loss_weights'], cfg['use_sil_for_loss'], cfg['sil_thres'],
                                cfg['use_l1'], cfg['ignore_outlier_depth_loss'], tracking=tracking, mapping=not tracking, do_ba=do_ba)
    loss.backward()
    ds_grad = depth_sil.grad if depth_sil.grad is not None else torch.zeros(3, H, W)    # (without the depth term the render takes no part)
    return float(loss.detach()), {k: float(v.detach()) for k, v in wl.items()}, im.grad, ds_grad


def _check(monkeypatch, cfg, tracking, do_ba=False):
    outliers = cfg['ignore_outlier_depth_loss']
    # (a NaN rendered depth not together with outlier rejection: torch.median of the frame's errors would be NaN)
    _, _, out6, gt_im, gt, median, at = track_pixel_planes(nan_depth=not outliers)
    loss, wl, g_im, g_ds = _get_loss_on_planes(monkeypatch, out6, gt_im, gt, cfg, tracking, do_ba)
    ref = LR.loss_from_planes(out6.reshape(6, H, W), gt_im.reshape(3, H, W), gt.reshape(1, H, W), cfg, tracking, do_ba)
    what = (LR.cfg_id(cfg), tracking, do_ba)
    assert LR.rel(ref['loss'], loss) <= 1e-6, (what, ref['loss'], loss)
    assert LR.rel(ref['im_term'], wl['im']) <= 1e-6, (what, ref['im_term'], wl['im'])
    if cfg['use_l1']:
        assert LR.rel(ref['depth_term'], wl['depth']) <= 1e-6, (what, ref['depth_term'], wl['depth'])
    else:
        assert 'depth' not in wl and ref['depth_term'] == 0.0 and ref['loss'] == ref['im_term'] and not ref['g'][3].any()
    if outliers:
        assert float(ref['median']) == float(median)                               # torch.median of the float32 errors, the lower one
    g = ref['g']
    assert not g[4:].any() and not g_ds[1:].any()                                   # silhouette and depth^2 carry no gradient
    assert not torch.isnan(g).any() and not torch.isnan(g_im).any() and not torch.isnan(g_ds).any()
    if tracking:
        # exact: +-weight, or 0 of either sign (outside the mask and at the kinks)
        assert (g[0:3].to(torch.float32) == g_im).all(), (what, torch.nonzero(g[0:3].to(torch.float32) != g_im))
        assert (g[3].to(torch.float32) == g_ds[0]).all(), (what, torch.nonzero(g[3].to(torch.float32) != g_ds[0]))
        assert set(np.unique(np.abs(LR.tracking_planes_f32(ref)[0:3]))) <= {np.float32(0), np.float32(LR.W_IM)}
        assert set(np.unique(np.abs(LR.tracking_planes_f32(ref)[3]))) <= {np.float32(0), np.float32(LR.W_DEPTH)}
    else:
        # the depth plane is one float32 division on either side; the colour planes go through SSIM in float32 there, float64 here
        d64 = g_ds[0].to(torch.float64)
        assert ((g[3] - d64).abs() <= 1e-6 * d64.abs()).all(), what
        assert ((g[3] == 0) == (d64 == 0)).all(), what
        LR.colour_planes_close(g_im.numpy(), g[0:3].numpy(), what)
    # ... and the hand-placed pixels decide what they are there for, in the restatement's own mask
    m = ref['mask'].reshape(-1)
    use_sil = tracking and cfg['use_sil_for_loss']
    thr = np.float32(cfg['sil_thres'])
    assert not m[at['gt_zero']] and not m[at['nan_unc']] and (outliers or not m[at['nan_depth']])
    for name in ('sil_at', 'sil_below', 'sil_above'):
        assert bool(m[at[name]]) == (not use_sil or bool(out6[4, at[name]].numpy() > thr)), (what, name)
    assert m[at['outlier_in']] and bool(m[at['outlier_out']]) == (not outliers), what
    assert m[at['depth_equal']] and g[3].reshape(-1)[at['depth_equal']] == 0
    return ref


@pytest.mark.parametrize("cfg", LR.TRACKING_CONFIGS, ids=LR.cfg_id)
def test_tracking_restatement_against_get_loss(monkeypatch, cfg):
    ref = _check(monkeypatch, cfg, tracking=True)
    if not (cfg['use_sil_for_loss'] or cfg['ignore_outlier_depth_loss']):
        # the unmasked colour sum: pixels outside the depth mask take part
        assert ref['im_l1'] > LR.loss_from_planes(*_planes(), dict(cfg, use_sil_for_loss=True), True)['im_l1']
        assert ref['g'][0:3].reshape(3, -1)[:, ~ref['mask'].reshape(-1)].any()


def _planes():
    _, _, out6, gt_im, gt, _, _ = track_pixel_planes(nan_depth=True)
    return out6.reshape(6, H, W), gt_im.reshape(3, H, W), gt.reshape(1, H, W)


@pytest.mark.parametrize("do_ba", [False, True])
@pytest.mark.parametrize("cfg", LR.MAPPING_CONFIGS, ids=LR.cfg_id)
def test_mapping_restatement_against_get_loss(monkeypatch, cfg, do_ba):
    ref = _check(monkeypatch, cfg, tracking=False, do_ba=do_ba)
    # use_sil_for_loss is read only when tracking: the same mapping loss with it set
    ref_sil = _check(monkeypatch, dict(cfg, use_sil_for_loss=True, sil_thres=0.99), tracking=False, do_ba=do_ba)
    assert ref_sil['loss'] == ref['loss'] and torch.equal(ref_sil['g'], ref['g']) and torch.equal(ref_sil['mask'], ref['mask'])


def test_grad_flags_are_get_loss_own():
    """The three branches at the top of get_loss (tracking / mapping with do_ba / mapping)."""
    assert LR.grad_flags(True) == (False, True) and LR.grad_flags(True, do_ba=True) == (False, True)
    assert LR.grad_flags(False) == (True, False) and LR.grad_flags(False, do_ba=True) == (True, True)


def test_every_flag_changes_the_restatement_on_these_planes():
    """No configuration is a copy of another on the hand-placed planes: all eight tracking losses differ pairwise; so do the four
    mapping (loss, mask count) pairs -- without the depth term outlier rejection shows in the mask alone."""
    for cfgs, tracking in ((LR.TRACKING_CONFIGS, True), (LR.MAPPING_CONFIGS, False)):
        _, _, out6, gt_im, gt, _, _ = track_pixel_planes(nan_depth=False)
        refs = [LR.loss_from_planes(out6.reshape(6, H, W), gt_im.reshape(3, H, W), gt.reshape(1, H, W), c, tracking) for c in cfgs]
        losses = [r['loss'] if tracking else (r['loss'], r['count']) for r in refs]
        assert len(set(losses)) == len(losses), losses
