"""Plain restatement of get_loss (splatam_amd/slam.py, itself pinned to /root/reference/scripts/splatam.py:214-347 by tests/golden/)
FROM THE RENDERED PLANES: what the fused iteration's loss kernels compute between the forward and the backward composite, for every
configuration get_loss accepts.  Shared by tests/test_loss_ref_cpu.py (which pins it to slam.get_loss) and tests/test_gpu_loss_configs.py.

TEST INFRASTRUCTURE.  Two rules:
  decisions  are taken in float32, exactly as torch's float32 get_loss takes them: gt > 0, the two isnan tests, silhouette >
             float32(sil_thres), |gt - depth| < 10 * median (difference and product in float32), the signs of gt - depth and of
             im - colour.  The median is torch.median (the LOWER median) of the float32 |gt - depth| * (gt > 0);
  sums and terms are formed in float64, from the per-pixel float32 differences get_loss itself forms.
So two sides that hold the same planes take the same mask, bit for bit, and differ in the order of their sums alone."""
import numpy as np
import torch


W_IM, W_DEPTH = 0.37, 1.9         # neither weight is 1.0: a dropped multiplication shows


def _cfg(use_sil, use_l1, outliers, sil_thres):
    return dict(use_sil_for_loss=use_sil, sil_thres=sil_thres, use_l1=use_l1, ignore_outlier_depth_loss=outliers,
                loss_weights=dict(im=W_IM, depth=W_DEPTH))


# tracking: use_sil_for_loss x use_l1 x ignore_outlier_depth_loss, all eight; the threshold 0.99 for half of them and 0.5 for the other
# half (either value with and without the silhouette, the depth term and outlier rejection)
TRACKING_CONFIGS = [_cfg(s, l, o, 0.99 if l != o else 0.5) for s in (True, False) for l in (True, False) for o in (False, True)]
# mapping: use_l1 x ignore_outlier_depth_loss (use_sil_for_loss is read only when tracking; do_ba is an argument of its own)
MAPPING_CONFIGS = [_cfg(False, l, o, 0.5) for l in (True, False) for o in (False, True)]


def cfg_id(cfg):
    return "-".join(f"{k}{int(cfg[v])}" for k, v in (("sil", "use_sil_for_loss"), ("l1", "use_l1"), ("out", "ignore_outlier_depth_loss"))) + \
        f"-thr{cfg['sil_thres']}"


def grad_flags(tracking, do_ba=False):
    """(gaussians_grad, camera_grad) of transform_to_frame as get_loss chooses them (/root/reference/scripts/splatam.py:219-231)."""
    if tracking:
        return False, True
    return True, bool(do_ba)


def loss_from_planes(out6, im, depth, cfg, tracking, do_ba=False):
    """out6 [6, H, W]: rendered r, g, b, depth, silhouette, depth^2; im [3, H, W], depth [1, H, W]: the frame; cfg: use_sil_for_loss,
    sil_thres, use_l1, ignore_outlier_depth_loss, loss_weights (the keys of slam.REPLICA_TRACKING); ``do_ba`` changes which
    parameters receive gradient (grad_flags), not the loss.  Returns a dict:
      mask        bool [H, W], the depth loss mask (tracking with the silhouette or outlier rejection: the colour mask too)
      median      float32 scalar tensor (outlier rejection) or None
      depth_l1, im_l1, count   the raw sums (float64): masked sum of |gt - depth|, (masked) sum of |im - colour|, mask.sum()
      ssim_sum    mapping: the sum of the SSIM map over 3 H W (float64)
      depth_term, im_term, loss   the two WEIGHTED terms and their sum (float64); depth_term is 0.0 without use_l1
      g           float64 [6, H, W]: dL/dout6"""
    o = torch.as_tensor(out6).detach().cpu().to(torch.float32)
    col, rd, sil, dsq = o[0:3], o[3], o[4], o[5]
    H, W = rd.shape
    gt_im = torch.as_tensor(im).detach().cpu().to(torch.float32).reshape(3, H, W)
    gt = torch.as_tensor(depth).detach().cpu().to(torch.float32).reshape(H, W)
    w_im, w_depth = float(cfg['loss_weights']['im']), float(cfg['loss_weights']['depth'])
    use_sil = bool(tracking and cfg['use_sil_for_loss'])
    outliers, use_l1 = bool(cfg['ignore_outlier_depth_loss']), bool(cfg['use_l1'])

    # ---- decisions, float32
    valid = gt > 0
    unc = dsq - rd * rd
    diff = gt - rd                                              # float32, as get_loss forms it
    median = None
    mask = valid
    if outliers:
        err = diff.abs() * valid
        median = err.median()
        mask = (err < 10 * median) & valid
    mask = mask & ~torch.isnan(rd) & ~torch.isnan(unc)
    if use_sil:
        mask = mask & (sil > torch.tensor(cfg['sil_thres'], dtype=torch.float32))
    d_sign = (diff < 0).to(torch.float64) - (diff > 0).to(torch.float64)       # d|gt - d| / dd; 0 at the kink (and for NaN)
    dcol = gt_im - col
    c_sign = (dcol < 0).to(torch.float64) - (dcol > 0).to(torch.float64)       # d|im - c| / dc

    # ---- sums, float64
    zero = torch.zeros((), dtype=torch.float64)
    d_abs = torch.where(mask, diff.abs().to(torch.float64), zero)
    depth_l1, count = float(d_abs.sum()), int(mask.sum())
    colour_mask = mask if (tracking and (use_sil or outliers)) else torch.ones_like(mask)
    im_l1 = float(torch.where(colour_mask[None].expand(3, -1, -1), dcol.abs().to(torch.float64), zero).sum())
    g = torch.zeros(6, H, W, dtype=torch.float64)
    ssim_sum = None
    if tracking:
        l_depth, l_im = depth_l1, im_l1
        g[0:3] = w_im * c_sign * colour_mask[None]
        if use_l1:
            g[3] = w_depth * d_sign * mask
    else:
        from splatam_amd import slam
        l_depth = depth_l1 / count if count else float('nan')
        x = col.to(torch.float64).clone().requires_grad_(True)
        y = gt_im.to(torch.float64)
        ssim = slam.calc_ssim(x, y)
        term = 0.8 * (x - y).abs().mean() + 0.2 * (1.0 - ssim)
        (w_im * term).backward()
        l_im = float(term.detach())
        ssim_sum = float(ssim.detach()) * 3 * H * W
        g[0:3] = x.grad
        if use_l1:
            g[3] = w_depth * d_sign * mask / count
    depth_term = w_depth * l_depth if use_l1 else 0.0
    im_term = w_im * l_im
    return dict(mask=mask, median=median, depth_l1=depth_l1, im_l1=im_l1, count=count, ssim_sum=ssim_sum, depth_term=depth_term,
                im_term=im_term, loss=depth_term + im_term, g=g)


def tracking_planes_f32(ref):
    """The tracking gradient planes as float32 numpy: every value is +-float32(w) or 0."""
    return ref['g'].to(torch.float32).numpy()


def rel(got, want):
    """|got - want| / |want| (0 / 0 = 0): the ratio the report checks print."""
    got, want = float(got), float(want)
    if want == 0.0:
        return 0.0 if got == 0.0 else float('inf')
    return abs(got - want) / abs(want)


def colour_planes_close(got, ref, what=""):
    """Mapping colour planes under the bound of test_ssim_loss_and_gradient_planes_against_torch: 1e-4 of the plane's maximum, with at
    most two pixels beyond it (|x - y| has a kink where the rendered colour equals the frame's to the last bit)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    err = np.abs(got - ref)
    kink = int((err > 1e-4 * scale).sum())
    assert float(err.max()) <= 1e-4 * scale or kink <= 2, (what, float(err.max()), scale, kink)
    return float(err.max()) / scale
