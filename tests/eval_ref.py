"""The evaluation metrics restated for the tests (tests/test_eval_cpu.py, tests/test_gpu_eval.py): the float64 torch form the
kernels and ``splatam_amd.slam`` are held to, with the per-level means exposed, and the seeded planes the comparisons run on.
Written from the published definitions (PSNR over all pixels, per-pixel |d| depth error, MS-SSIM with an unpadded 11-tap window
and 2x2 pooling that zero-pads odd sizes); it shares no code with the package."""
import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def level_sizes(n):
    out = [n]
    for _ in range(4):
        out.append(out[-1] // 2 + out[-1] % 2)
    return out


def ms_ssim_levels(X, Y):
    """[1,3,H,W] x 2 in any float dtype -> (cs means [5,3], ssim means [5,3], ms_ssim scalar), all in that dtype."""
    c = torch.arange(11, dtype=X.dtype) - 5
    g = torch.exp(-c ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()

    def blur(x):
        x = F.conv2d(x, g.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3)
        return F.conv2d(x, g.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)

    cs_means, ss_means, vals = [], [], []
    for level in range(5):
        mu1, mu2 = blur(X), blur(Y)
        s1, s2, s12 = blur(X * X) - mu1 * mu1, blur(Y * Y) - mu2 * mu2, blur(X * Y) - mu1 * mu2
        cs = (2 * s12 + 0.03 ** 2) / (s1 + s2 + 0.03 ** 2)
        ss = (2 * mu1 * mu2 + 0.01 ** 2) / (mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * cs
        cs_means.append(cs.flatten(2).mean(-1)[0])
        ss_means.append(ss.flatten(2).mean(-1)[0])
        vals.append(torch.relu(cs_means[-1] if level < 4 else ss_means[-1]))
        if level < 4:
            pad = [d % 2 for d in X.shape[2:]]
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    w = torch.tensor(WEIGHTS, dtype=X.dtype).view(-1, 1)
    return torch.stack(cs_means), torch.stack(ss_means), torch.prod(torch.stack(vals) ** w, 0).mean()


def frame_metrics(rgb, depth, sil, gt_im, gt_depth, sil_thres, sil_mask, dtype=torch.float64, with_ms_ssim=True):
    """CPU planes (float32) -> dict: psnr, depth_l1, valid, and with MS-SSIM cs [5,3], ss [5,3], ms_ssim; arithmetic in ``dtype``.
    The masks are decided on the float32 inputs (they are decisions, not arithmetic)."""
    valid = (gt_depth.reshape(1, *rgb.shape[-2:]) > 0)
    presence = (sil.reshape(1, *rgb.shape[-2:]) > np.float32(sil_thres))
    v, p = valid.to(dtype), presence.to(dtype)
    im, gt, d, gd = rgb.to(dtype), gt_im.to(dtype), depth.reshape(1, *rgb.shape[-2:]).to(dtype), gt_depth.reshape(1, *rgb.shape[-2:]).to(dtype)
    if sil_mask:
        wim, wgt = im * p * v, gt * p * v
        diff = (d * v - gd) * p
    else:
        wim, wgt = im * v, gt * v
        diff = d * v - gd
    mse = ((wim - wgt) ** 2).reshape(3, -1).mean(1)
    out = {'psnr': (20 * torch.log10(1.0 / torch.sqrt(mse))).mean(), 'depth_l1': (diff.abs() * v).sum() / v.sum(), 'valid': int(valid.sum())}
    if with_ms_ssim:
        out['cs'], out['ss'], out['ms_ssim'] = ms_ssim_levels(wim.unsqueeze(0), wgt.unsqueeze(0))
    return out


def seeded_planes(W, H, seed, sil_thres=0.5):
    """A rendered frame and its RGB-D frame as CPU float32 planes: a textured image, the ground truth = that image + noise, ~10 % of
    the depth pixels invalid at random plus an invalid rectangle, a silhouette on both sides of the threshold.  No silhouette lies
    within 1e-4 of the threshold and no ground-truth depth in (0, 1e-6): both masks are then the same decision in any arithmetic
    (asserted here, on the inputs)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.3 * torch.sin(xx / 7.0 + k) * torch.cos(yy / (5.0 + k)) + 0.1 * torch.sin((xx + 2 * yy) / (23.0 + 3 * k)) for k in range(3)])
    tex = (base + 0.08 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
    gt_im = tex.contiguous()
    rgb = (tex + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1).contiguous()
    gt_depth = 1.0 + 2.0 * torch.rand(1, H, W, generator=g) + 0.5 * torch.sin(xx / 40.0)[None]
    gt_depth[torch.rand(1, H, W, generator=g) < 0.1] = 0.0
    gt_depth[:, H // 5:H // 3, W // 4:W // 2] = 0.0
    depth = (gt_depth + 0.02 * torch.randn(1, H, W, generator=g)).clamp_min(0.0) + 1.5 * (gt_depth == 0)
    sil = torch.rand(H, W, generator=g)
    sil = torch.where(sil < 0.85, 0.6 + 0.4 * sil, 0.45 * sil)         # ~85 % present; the rest well below the threshold
    sil[H // 2:H // 2 + H // 8, W // 8:W // 3] = 0.1
    near = (sil - sil_thres).abs() < 1e-4
    sil[near] = sil_thres + 0.01
    assert float((sil - sil_thres).abs().min()) >= 1e-4
    assert not bool(((gt_depth > 0) & (gt_depth < 1e-6)).any())
    assert 0.02 < float((gt_depth == 0).float().mean()) < 0.5 and 0.05 < float((sil < sil_thres).float().mean()) < 0.5
    return rgb, depth.contiguous(), sil.contiguous(), gt_im, gt_depth.contiguous()


def f32_ulps(value, n=16):
    """n float32 units in the last place at |value|."""
    return n * float(np.spacing(np.float32(abs(float(value)))))


# ---- the case behind tests/golden/eval_reference.npz (regenerated from its seeds by the generator and by the tests) ----------------
GOLDEN_SCENE = dict(n_gaussians=14000, W=240, H=176, f=200.0, frames=12, seed=5, step_m=0.012, step_deg=0.4)
GOLDEN_NAN_POSE_FRAME = 7
GOLDEN_SIL_THRES = 0.5
# (mapping_iters, add_new_gaussians) of the two mask variants, and the two cadences
GOLDEN_VARIANTS = {"valid": (60, True), "sil": (0, False)}
GOLDEN_EVERY = (1, 5)


class EvalSequence:
    """The synthetic sequence with what an evaluation has to cope with: a rectangle of invalid depth in every frame and one frame
    whose ground-truth pose is NaN.  Items as the reference's datasets hand them over."""

    def __init__(self, ds):
        self.items = []
        for t in range(len(ds)):
            color, depth, k, pose = ds[t]
            depth = depth.clone()
            H, W = depth.shape[:2]
            depth[H // 6:H // 3, W // 2:W // 2 + W // 4] = 0.0
            if t == GOLDEN_NAN_POSE_FRAME:
                pose = torch.full_like(pose, float("nan"))
            self.items.append((color, depth, k, pose))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, t):
        return self.items[t]


def golden_case(device="cpu"):
    """(dataset, final params) of the golden evaluation: the scene's own Gaussians without those of one region (a hole in the
    silhouette), poses perturbed from a seed (frame 0 kept), so that the trajectory error is not zero.  ``slam.Renderer`` must
    already be the renderer the caller wants the frames made with."""
    from splatam_amd import pipeline
    s = GOLDEN_SCENE
    ds = pipeline.SyntheticRGBDSequence(s['n_gaussians'], s['W'], s['H'], s['f'], s['f'], s['W'] / 2 - 0.5, s['H'] / 2 - 0.5, num_frames=s['frames'],
                                        seed=s['seed'], device=device, step_m=s['step_m'], step_deg=s['step_deg'])
    scene = ds._scene
    m = scene['means3D']
    keep = ~((m[:, 0] > 0.2) & (m[:, 0] < 0.7) & (m[:, 1] > -0.1) & (m[:, 1] < 0.35))
    params = {k: (v[keep] if v.shape[0] == m.shape[0] else v).clone().contiguous() for k, v in scene.items()}
    g = torch.Generator().manual_seed(1234)
    dq = 0.003 * torch.randn(1, 4, s['frames'], generator=g)
    dt = 0.01 * torch.randn(1, 3, s['frames'], generator=g)
    dq[..., 0] = 0
    dt[..., 0] = 0
    params['cam_unnorm_rots'] = (params['cam_unnorm_rots'] + dq.to(device)).contiguous()
    params['cam_trans'] = (params['cam_trans'] + dt.to(device)).contiguous()
    return EvalSequence(ds), params
