"""The per-frame SplaTAM loop on the HIP engine: what ``rgbd_slam`` does between loading a frame and
storing a keyframe (/root/reference/scripts/splatam.py:654-905), without the reference's I/O, logging and evaluation.

=============================================  =============================================
here                                           reference
=============================================  =============================================
``keyframe_selection_overlap``                 utils/keyframe_selection.py:44-103 (+ its get_pointcloud :10-41)
``replica_config`` / ``splatam_s_config``      configs/replica/splatam.py / splatam_s.py (the values the loop reads)
``rgbd_slam`` (over ``session.SlamSession``)   scripts/splatam.py:455-905 (frame loop: pose initialisation, tracking with
                                               best-candidate bookkeeping and the depth-loss retry, densification,
                                               keyframe selection, mapping with pruning, keyframe list)
``save_params`` / ``load_params``              utils/common_utils.py:25-52 (``params.npz``)
``SyntheticRGBDSequence``                      stands in for datasets/gradslam_datasets/* (no datasets offline)
=============================================  =============================================

``engine="fused"`` runs every iteration through ``FusedEngine`` (C ABI ``splat_iter_*`` / ``splat_map_*``: ~8 kernel
launches per iteration, map edits in place on the device); ``engine="dropin"`` runs the reference-shaped PyTorch loop
(``splatam_amd.slam``) on the drop-in rasterizer.  Both follow the reference's control flow line by line, including the
places where it is surprising: pruning happens between ``backward()`` and ``optimizer.step()``, and ``remove_points``
re-creates the parameters, so the iterations on the pruning schedule take NO Adam step
(scripts/splatam.py:857-868, utils/slam_external.py:139-162).
"""
from __future__ import annotations

import contextlib
import copy
import math
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import _capi, slam


# --------------------------------------------------------------------------
# keyframe selection
# --------------------------------------------------------------------------

def _sampled_cloud(z, intrinsics, w2c, sampled_indices):
    """World-frame points of the sampled pixels (``z``: their depths); points that coincide after rounding to 1e-4 (duplicated
    samples, or the camera origin) are dropped, all copies of them, as the reference's unique/isin construction does."""
    fx, fy, cx, cy = intrinsics[0][0], intrinsics[1][1], intrinsics[0][2], intrinsics[1][2]
    v, u = sampled_indices[:, 0], sampled_indices[:, 1]
    pts_cam = torch.stack(((u - cx) / fx * z, (v - cy) / fy * z, z), dim=-1)
    c2w = torch.inverse(w2c)
    pts = pts_cam @ c2w[:3, :3].t() + c2w[:3, 3]
    # |round(p, 4)| as integers: round(p, 4) is round(p * 1e4) / 1e4, and distinct integers below 2^24 give distinct float32 quotients, so
    # two points coincide after rounding exactly when their integer triples do.  Three 21-bit fields make ONE int64 key per point:
    # a 1-d unique instead of unique(dim=0) (3 ms -> 0.1 ms for the 1600 samples on the host)
    q = torch.abs(torch.round(pts * 1e4)).to(torch.int64)
    if pts.dtype == torch.float32 and int(q.max()) < (1 << 21):
        key = torch.cat(((q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2], torch.zeros(1, dtype=torch.int64, device=pts.device)))
        _, inverse, counts = key.unique(return_inverse=True, return_counts=True)
    else:
        key = torch.cat((torch.abs(torch.round(pts, decimals=4)), torch.zeros(1, 3, device=pts.device, dtype=pts.dtype)), dim=0)
        _, inverse, counts = key.unique(dim=0, return_inverse=True, return_counts=True)
    keep = (counts[inverse] == 1)[:pts.shape[0]]
    return pts[keep]


def keyframe_selection_overlap(gt_depth, w2c, intrinsics, keyframe_list, k, pixels=1600):
    """Indices (into ``keyframe_list``) of up to ``k`` keyframes that see part of the current frame: 1600 valid-depth
    pixels are back-projected and re-projected into every keyframe (one batched product over all keyframes); keyframes with
    a non-zero share of points inside the image (20 px border) are kept, ordered by that share, then shuffled."""
    # The frame stays where it is: the valid-pixel list (one nonzero: row-major order, as torch.where gives it) and the gather of the
    # 1600 sampled depths run on the depth image's device, and only those samples travel to the host -- copying the frame and scanning
    # it there cost ~5 ms per 1200x680 frame.  The few thousand points against a few dozen keyframes that follow are host-side work
    # (on the GPU the unique(dim=0) / tolist chain cost 86 ms per frame in synchronisations and tiny launches).  Random numbers are
    # drawn where the reference draws them: torch.randint on the CPU generator, then numpy's permutation.
    H, W = gt_depth.shape[1], gt_depth.shape[2]
    valid = torch.nonzero(gt_depth[0] > 0)
    pick = torch.randint(valid.shape[0], (pixels,))
    sampled = valid[pick.to(valid.device)]
    z = gt_depth[0, sampled[:, 0], sampled[:, 1]].cpu()
    sampled, w2c, intrinsics = sampled.cpu(), w2c.cpu(), intrinsics.cpu()
    # (a few thousand floats per operation: on a 256-core host every one of these CPU operators otherwise wakes the whole thread pool)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _select_from_samples(z, sampled, w2c, intrinsics, keyframe_list, k, H, W)
    finally:
        torch.set_num_threads(threads)


def _select_from_samples(z, sampled, w2c, intrinsics, keyframe_list, k, H, W):
    pts = _sampled_cloud(z, intrinsics, w2c, sampled)
    if len(keyframe_list) == 0:
        return []
    est = torch.stack([kf['est_w2c'] for kf in keyframe_list]).cpu()               # [K,4,4]
    cam = torch.einsum('kij,nj->kni', est[:, :3, :3], pts) + est[:, None, :3, 3]     # [K,N,3]
    proj = torch.einsum('ij,knj->kni', intrinsics.to(cam.dtype), cam)
    zc = proj[..., 2] + 1e-5
    px, py = proj[..., 0] / zc, proj[..., 1] / zc
    edge = 20
    inside = (px < W - edge) & (px > edge) & (py < H - edge) & (py > edge) & (zc > 0)
    share = (inside.sum(dim=1) / max(pts.shape[0], 1)).tolist()
    order = sorted(range(len(keyframe_list)), key=lambda i: share[i], reverse=True)      # stable, like the reference's sorted()
    chosen = [i for i in order if share[i] > 0.0]
    return list(np.random.permutation(np.array(chosen))[:k])


# --------------------------------------------------------------------------
# configuration, I/O
# --------------------------------------------------------------------------

def replica_config(tracking_iters=40, mapping_iters=60, map_every=1, keyframe_every=5, mapping_window_size=24):
    """The entries of /root/reference/configs/replica/splatam.py that the frame loop reads."""
    return dict(
        seed=0, map_every=map_every, keyframe_every=keyframe_every, mapping_window_size=mapping_window_size,
        scene_radius_depth_ratio=3, mean_sq_dist_method="projective", gaussian_distribution="isotropic",
        tracking=dict(use_gt_poses=False, forward_prop=True, num_iters=tracking_iters, use_sil_for_loss=True, sil_thres=0.99,
                      use_l1=True, ignore_outlier_depth_loss=False, use_depth_loss_thres=False, depth_loss_thres=100000,
                      loss_weights=dict(im=0.5, depth=1.0), lrs=dict(slam.REPLICA_TRACKING['lrs'])),
        mapping=dict(num_iters=mapping_iters, add_new_gaussians=True, sil_thres=0.5, use_l1=True, use_sil_for_loss=False,
                     ignore_outlier_depth_loss=False, loss_weights=dict(im=0.5, depth=1.0), lrs=dict(slam.REPLICA_MAPPING['lrs']),
                     prune_gaussians=True, pruning_dict=dict(slam.REPLICA_PRUNE), use_gaussian_splatting_densification=False))


def splatam_s_config(width=1200, height=680, **kw):
    """The entries of /root/reference/configs/replica/splatam_s.py (SplaTAM-S) that the frame loop reads: 10 tracking and 15
    mapping iterations, a mapping window of 32, tracking at the frame's own size and densification at half of it (600 x 340 under
    the 1200 x 680 map), everything else as ``replica_config``.  ``width`` / ``height``: the dataset's frame size, i.e.
    ``desired_image_width`` / ``_height``."""
    cfg = replica_config(**dict(dict(tracking_iters=10, mapping_iters=15, mapping_window_size=32), **kw))
    cfg['data'] = dict(desired_image_height=int(height), desired_image_width=int(width),
                       tracking_image_height=int(height), tracking_image_width=int(width),
                       densification_image_height=int(height) // 2, densification_image_width=int(width) // 2)
    return cfg


def save_params(output_params, output_dir, time_idx=None):
    """``params.npz`` (or ``params<time_idx>.npz``): one array per entry of the params dict."""
    os.makedirs(output_dir, exist_ok=True)
    name = "params.npz" if time_idx is None else f"params{time_idx}.npz"
    path = os.path.join(output_dir, name)
    np.savez(path, **{k: (v.detach().cpu().contiguous().numpy() if isinstance(v, torch.Tensor) else v) for k, v in output_params.items()})
    return path


def load_params(path, device="cuda"):
    """Inverse of ``save_params`` the way the reference's checkpoint loader reads it (scripts/splatam.py:611-613)."""
    raw = dict(np.load(path, allow_pickle=True))
    return {k: torch.tensor(v).to(device).float().requires_grad_(True) for k, v in raw.items()}


class SyntheticRGBDSequence:
    """RGB-D frames rendered from a seeded synthetic scene along a smooth trajectory (no datasets offline).  Items look like
    the reference's gradslam datasets: ``(color[H,W,3] in 0..255, depth[H,W,1], intrinsics[4,4], pose[4,4])`` with the pose
    (camera-to-world) relative to the first frame.  The scene is a smooth, opaque, textured surface (``n_gaussians`` splats
    on z = z0 + ripples, colours a sum of low- and mid-frequency waves) so that frame-to-model tracking is well posed --
    the random per-pixel depth layers of the kernel workloads (bench.build_scene) are not."""

    def __init__(self, n_gaussians, width, height, fx, fy, cx, cy, num_frames, seed=0, device="cuda", step_m=0.01, step_deg=0.3):
        self.W, self.H, self.num_frames, self.device = width, height, num_frames, device
        self.k = torch.tensor([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32, device=device)
        g = torch.Generator().manual_seed(seed)
        n = int(n_gaussians)
        m = 0.15                                            # the surface extends past the first view: later frames see new parts
        u = (torch.rand(n, generator=g, dtype=torch.float64) * (1 + 2 * m) - m) * width - 0.5
        v = (torch.rand(n, generator=g, dtype=torch.float64) * (1 + 2 * m) - m) * height - 0.5
        su, sv = u / width * 2 * math.pi, v / height * 2 * math.pi
        z = 2.5 + 0.35 * torch.sin(1.3 * su + 0.4) * torch.cos(0.9 * sv) + 0.15 * torch.sin(2.7 * sv + 1.0)
        means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], dim=-1)
        rgb = torch.stack([0.5 + 0.25 * torch.sin(3 * su) * torch.cos(2 * sv) + 0.2 * torch.sin(17 * su + 0.3) * torch.sin(13 * sv),
                           0.5 + 0.25 * torch.cos(2 * su + 1.0) * torch.sin(3 * sv) + 0.2 * torch.sin(11 * su) * torch.cos(19 * sv + 0.7),
                           0.5 + 0.25 * torch.sin(4 * su + 2.0) + 0.2 * torch.cos(15 * su + 9 * sv)], dim=-1).clamp(0.02, 0.98)
        spacing = math.sqrt((1 + 2 * m) ** 2 * width * height / n)        # mean distance between neighbouring splats in pixels
        log_scales = torch.log(1.1 * spacing * z / ((fx + fy) / 2))[:, None]
        rots = torch.zeros(n, 4, dtype=torch.float64)
        rots[:, 0] = 1.0
        cam_rots = torch.zeros(1, 4, num_frames)
        cam_trans = torch.zeros(1, 3, num_frames)
        for t in range(num_frames):
            ang = math.radians(step_deg * t)
            cam_rots[0, :, t] = torch.tensor([math.cos(ang / 2), 0.0, math.sin(ang / 2), 0.0])
            cam_trans[0, :, t] = torch.tensor([step_m * t, -0.3 * step_m * t, 0.5 * step_m * t])
        raw = dict(means3D=means, rgb_colors=rgb, unnorm_rotations=rots, logit_opacities=torch.full((n, 1), 4.0, dtype=torch.float64),
                   log_scales=log_scales, cam_unnorm_rots=cam_rots, cam_trans=cam_trans)
        self._scene = {k: t.to(device=device, dtype=torch.float32).contiguous() for k, t in raw.items()}
        self._cam = slam.setup_camera(width, height, self.k[:3, :3].cpu().numpy(), np.eye(4, dtype=np.float32), device=device)
        self._w2c0 = torch.eye(4, device=device)

    def __len__(self):
        return self.num_frames

    def preload(self):
        """Render every frame once and keep it (a real dataset hands over loaded images; without this every ``dataset[t]`` renders)."""
        self._cache = {t: self._item(t) for t in range(self.num_frames)}
        return self

    def gt_w2c(self, t):
        q = F.normalize(self._scene['cam_unnorm_rots'][..., t].detach())
        w2c = torch.eye(4, device=self.device)
        w2c[:3, :3] = slam.build_rotation(q)[0]
        w2c[:3, 3] = self._scene['cam_trans'][0, :, t].detach()
        return w2c

    def __getitem__(self, t):
        cache = getattr(self, "_cache", None)
        return cache[t] if cache is not None and t in cache else self._item(t)

    def _item(self, t):
        im, depth = self._render(t)
        pose = torch.inverse(self.gt_w2c(t))
        return (im.permute(1, 2, 0) * 255.0).contiguous(), depth.permute(1, 2, 0).contiguous(), self.k, pose

    def _render(self, t):
        with torch.no_grad():
            p = self._scene
            tg = slam.transform_to_frame(p, t, gaussians_grad=False, camera_grad=False)
            rv = slam.transformed_params2rendervar(p, tg)
            im, _, _ = slam.Renderer(raster_settings=self._cam)(**{k: v.detach() for k, v in rv.items()})
            dv = slam.transformed_params2depthplussilhouette(p, self._w2c0, tg)
            ds, _, _ = slam.Renderer(raster_settings=self._cam)(**{k: v.detach() for k, v in dv.items()})
            sil = ds[1:2]
            depth = torch.where(sil > 0.5, ds[0:1] / sil.clamp_min(1e-6), torch.zeros_like(sil))
        return im.clamp(0, 1).contiguous(), depth.contiguous()


# --------------------------------------------------------------------------
# the frame loop
# --------------------------------------------------------------------------

def _est_w2c(params, time_idx):
    q = F.normalize(params['cam_unnorm_rots'][..., time_idx].detach())
    w2c = torch.eye(4, device=q.device)
    w2c[:3, :3] = slam.build_rotation(q)[0]
    w2c[:3, 3] = params['cam_trans'][0, :, time_idx].detach()
    return w2c


def initialize_first_timestep(dataset, num_frames, scene_radius_depth_ratio, mean_sq_dist_method, gaussian_distribution, device="cuda",
                              densify_frame=None, first=None, planes=None):
    """Map, variables, intrinsics, first-frame world-to-camera and camera from frame 0.  ``densify_frame`` = (im, depth,
    intrinsics[3, 3]) of the first densification frame when densification has a size of its own: the point cloud, its mean squared
    distances and the scene radius then come from IT, camera and w2c from the full frame (scripts/splatam.py:185-206).  ``first``:
    ``dataset[0]`` when the caller has read it already; ``planes`` = (im [3, H, W] in 0..1, depth [1, H, W]) when it has the frame
    in the loop's layout already (the item's colour and depth are then not read)."""
    color, depth, intrinsics, pose = dataset[0] if first is None else first
    if planes is not None:
        color, depth = planes
    else:
        color = color.permute(2, 0, 1) / 255
        depth = depth.permute(2, 0, 1)
    intrinsics = intrinsics[:3, :3]
    w2c = torch.linalg.inv(pose)
    cam = slam.setup_camera(color.shape[2], color.shape[1], intrinsics.cpu().numpy(), w2c.detach().cpu().numpy(), device=device)
    cloud_intrinsics = intrinsics
    if densify_frame is not None:
        color, depth, cloud_intrinsics = densify_frame
    mask = (depth > 0).reshape(-1)
    cloud, msd = slam.get_pointcloud(color, depth, cloud_intrinsics, w2c, mask=mask, compute_mean_sq_dist=True,
                                     mean_sq_dist_method=mean_sq_dist_method)
    params, variables = slam.initialize_params(cloud, num_frames, msd, gaussian_distribution)
    variables['scene_radius'] = torch.max(depth) / scene_radius_depth_ratio
    return params, variables, intrinsics, w2c, cam


class _ReducedFrames:
    """The frames of one of the loop's reduced resolutions (tracking, densification): items of a dataset of that size, as the
    reference keeps one (scripts/splatam.py:537-587; ``first_item``: its first, which fixes size and intrinsics), or derived from the
    full-size frame -- ``prepare_frame`` (the HIP kernel for frames on the device, the torch mirror on the CPU) and
    ``scale_intrinsics``, i.e. what such a dataset does to every frame it loads.  ``intrinsics``: the caller's own for the derived
    frames (a live session scales those of the raw image)."""

    def __init__(self, first_item, size, full_size, full_k, intrinsics=None):
        self.from_items, self.size = first_item is not None, (int(size[0]), int(size[1]))
        self._planes = None
        if first_item is not None:
            color, _, k, _ = first_item
            self.size = (int(color.shape[0]), int(color.shape[1]))
            self.intrinsics = k[:3, :3]
        elif intrinsics is not None:
            self.intrinsics = intrinsics[:3, :3]
        else:
            self.intrinsics = slam.scale_intrinsics(full_k, self.size[0] / full_size[0], self.size[1] / full_size[1])[:3, :3]
        self.cam = None

    def frame(self, time_idx, full_color, full_depth, item=None):
        """(im [3, h, w], depth [1, h, w]); ``full_*``: the full-size frame as the dataset hands it over; ``item``: this time
        index's item of the dataset of this size.  Derived frames on the device are written into ONE pair of planes kept for this
        resolution (a reduced frame is used within its own time index only: the keyframe list keeps full-size frames)."""
        if self.from_items:
            if item is None:
                raise ValueError(f"frame {time_idx}: this resolution takes its frames from a dataset of its own, and no item of it was passed")
            color, depth = item[0], item[1]
            return (color.permute(2, 0, 1) / 255).contiguous(), depth.permute(2, 0, 1).contiguous()
        if full_color.device.type == "cuda":
            from . import fused
            if self._planes is None:
                h, w = self.size
                self._planes = (torch.empty(3, h, w, dtype=torch.float32, device=full_color.device),
                                torch.empty(1, h, w, dtype=torch.float32, device=full_color.device))
            return fused.prepare_frame(full_color, full_depth, self.size, out=self._planes)
        return slam.prepare_frame(full_color, full_depth, self.size)

    def curr_data(self, time_idx, full_color, full_depth, w2c, item=None):
        im, depth = self.frame(time_idx, full_color, full_depth, item)
        return {'cam': self.cam, 'im': im, 'depth': depth, 'id': time_idx, 'intrinsics': self.intrinsics, 'w2c': w2c}


def _reduced_frames(which, first_item, config, full_size, full_k):
    """The tracking / densification frames of a run, or None when that step runs on the full frame: the first item of a dataset the
    caller passed, or ``config['data'][<which>_image_height / _width]`` that differ from the dataset's size (equal sizes mean "not
    separate": scripts/splatam.py:498-517)."""
    if first_item is not None:
        return _ReducedFrames(first_item, (0, 0), full_size, full_k)
    data = config.get('data') or {}
    if f"{which}_image_height" not in data:
        return None
    size = (int(data[f"{which}_image_height"]), int(data[f"{which}_image_width"]))
    return None if size == tuple(full_size) else _ReducedFrames(None, size, full_size, full_k)


class _PhaseTimer:
    """Wall time per named phase of the frame being processed (a device synchronisation on either side: ~10 per frame; ``sync=False``:
    host time only, for a phase whose device work the next synchronised phase waits for anyway).  ``on=False``: every phase is the
    same empty context -- nothing is timed and nothing synchronised."""
    _off = contextlib.nullcontext()

    def __init__(self, dev, on=True):
        self.dev, self.on, self.frame, self._open = dev, on, {}, []

    def _sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def __call__(self, name, sync=True):
        if not self.on:
            return self._off
        self._name, self._sync_next = name, sync
        return self

    def __enter__(self):
        if self._sync_next:
            self._sync()
        self._open.append((self._name, time.perf_counter(), self._sync_next))

    def __exit__(self, *exc):
        name, t0, sync = self._open.pop()
        if sync:
            self._sync()
        self.frame[name] = self.frame.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)

    def next_frame(self):
        done, self.frame = self.frame, {}
        return {k: round(v, 3) for k, v in done.items()}


def rgbd_slam(dataset, config, engine="fused", num_frames=None, gaussian_capacity=None, verbose=False, evaluate=None,
              tracking_dataset=None, densify_dataset=None, checkpoint_dir=None, resume_exact=None, exact_checkpoints=False):
    """Runs the SplaTAM frame loop over ``dataset`` -- the driver over ``session.SlamSession``, which holds the loop's set-up and its
    per-frame body: every frame is one ``add_frame(*dataset[i])`` -- and returns ``(params, variables, stats)`` with
    ``stats = {keyframe_time_indices, tracking_iters, mapping_iters, tracking_s, mapping_s, mapping_loop_s, num_gaussians,
    redone_iterations, phase_ms}`` (``mapping_loop_s``: the iterations alone, where the reference's own mapping timer runs,
    scripts/splatam.py:825-891; ``mapping_s`` also holds densification, keyframe selection and list re-learning; ``phase_ms``: one
    dict per frame -- prepare_frames, tracking, add_new_gaussians, keyframe_selection, relearn_lists, mapping_iterations, prune,
    keyframe_store).

    Resolutions of their own (SplaTAM-S, the iPhone configurations: scripts/splatam.py:498-517, 537-587): tracking runs on
    ``tracking_dataset``'s frames and camera, ``add_new_gaussians`` and the first frame's point cloud on ``densify_dataset``'s;
    keyframe selection, mapping, the keyframe list and the evaluation stay on ``dataset``'s full-size frames.  Without such a dataset
    the sizes are read from ``config['data']`` (``tracking_image_height / _width``, ``densification_image_height / _width``; sizes
    equal to the dataset's mean "not separate") and the reduced frames are derived from the full frame by ``prepare_frame`` +
    ``slam.scale_intrinsics`` -- on the device for a dataset on the device.  The fused engine holds ONE map and one camera per
    resolution (FusedEngine.add_camera).  Not with several ranks.

    ``engine``: "fused" (FusedEngine: every iteration one C call, the map edited in place on the device), "dropin" (the
    reference-shaped PyTorch loop of splatam_amd.slam on the drop-in rasterizer), or "plugin": the SAME reference-shaped loop -- its
    ``add_new_gaussians`` / ``prune_gaussians`` / ``remove_points`` re-create every tensor, its statements are get_loss -> backward ->
    prune -> step -- with ``splatam_amd.plugin`` installed into the module that holds it, i.e. what
    /root/reference/scripts/splatam.py:654-905 executes after ``plugin.install``; "plugin_map_edits": the same with
    ``plugin.install(map_edits=True)`` (the two map edits are adapters too: the engine owns the map and edits it in place).

    Per-tile list overflow (fused): a flagged iteration and every iteration after it take NO Adam step on the device
    (include/splat_hip.h, SPLAT_REPORT_FLAG); at the end of a phase ``check_overflow()`` says how many, the lists are re-sized and exactly
    that many iterations are run again -- the pose / the map never saw a bad gradient, so nothing has to be restored.

    With ``torch.distributed`` initialised (one process per GPU, splatam_amd.dist.init_from_env) the loop runs on every rank
    over the REPLICATED map:
      * tracking: the frame's tile rows are sharded over the ranks (every rank takes the same Adam step); with the outlier-rejecting
        loss every rank tracks the whole frame and rank 0's pose is then broadcast (7 floats), because the float
        atomics of the backward composite leave the replicas' poses different in the last bits and the densification that follows
        thresholds a render at that pose;
      * mapping: every iteration draws ``world`` keyframe views instead of one (the same random stream on every rank, the
        reference's one-random-keyframe-per-iteration rule /root/reference/scripts/splatam.py:831-845 applied ``world`` times),
        rank r renders the r-th, ONE gradient all-reduce (mean) follows, and every rank takes the identical Adam step;
      * after every edit of the map (densification, pruning) the row counts of the replicas are compared (all-reduce of min / max).

    ``evaluate``: ``None`` (default) -- the loop ends where it always did; a dict with any of ``eval_every`` (1), ``eval_dir`` (None),
    ``ms_ssim`` (True), ``save_frames``, ``lpips_weights`` (None; default ``config['lpips_weights']`` where the config has it) -- the run's last act is the reference's (scripts/splatam.py:961-971): ``evaluation.evaluate`` on the final
    parameters with the mapping configuration's ``sil_thres`` / ``num_iters`` / ``add_new_gaussians``, returned as ``stats['eval']``
    (PSNR, depth L1, MS-SSIM per evaluated frame, ATE; LPIPS with ``lpips_weights``: ``evaluation.evaluate``).  The fused engine evaluates on its own map, the other
    engines' parameters get a throw-away ``FusedEngine``; with several ranks rank 0 evaluates and the dict is broadcast.

    Checkpoints (splatam_amd/checkpoint.py; engines "fused" and "dropin", one rank).  With ``checkpoint_dir`` -- default
    ``workdir/run_name`` where the config has both -- the reference's four keys are honoured as it honours them:
    ``save_checkpoints`` writes ``params<t>.npz`` and ``keyframe_time_indices<t>.npy`` after every frame with
    ``t % checkpoint_interval == 0`` (scripts/splatam.py:927-931); ``load_checkpoint`` with ``checkpoint_time_idx = t`` does what
    :604-640 do (``SlamSession.load_reference_checkpoint``): the loop restarts AT ``t``, so that frame is tracked and mapped again.
    Without a directory and with the keys off nothing changes.  ``resume_exact=t``: ``SlamSession.restore`` of the exact checkpoint
    ``SlamSession.save_checkpoint`` wrote after frame ``t`` in that directory, continued at ``t + 1`` as if the run had never
    stopped (``stats`` cover the whole run).  ``exact_checkpoints=True``: the frames on which ``save_checkpoints`` writes the pair get
    the exact checkpoint (the pair plus ``session<t>.npz``; keyframe planes are read from ``dataset`` again).
    ``config['load_checkpoint']`` always means the reference's form."""
    from . import checkpoint
    from . import dist as sdist
    from .session import SlamSession
    world, rank = sdist.world_size(), sdist.get_rank()
    num_frames = len(dataset) if num_frames is None else min(num_frames, len(dataset))
    if checkpoint_dir is None:
        checkpoint_dir = checkpoint.default_directory(config)
    saves = bool(config.get('save_checkpoints')) and checkpoint_dir is not None
    loads = bool(config.get('load_checkpoint')) and checkpoint_dir is not None
    start = 0
    if resume_exact is not None:
        if checkpoint_dir is None:
            raise ValueError("resume_exact needs checkpoint_dir (or config['workdir'] and config['run_name'])")
        if loads:
            raise ValueError("resume_exact and config['load_checkpoint'] are two different ways to resume: choose one")
        session = SlamSession.restore(config, checkpoint_dir, int(resume_exact), num_frames=num_frames, dataset=dataset, engine=engine,
                                      gaussian_capacity=gaussian_capacity, verbose=verbose, return_pose=False, reference_division=True)
        start = session.frames_seen
    else:
        session = SlamSession(config, num_frames, engine=engine, gaussian_capacity=gaussian_capacity, verbose=verbose, return_pose=False,
                              reference_division=True)
    # the loop body and its set-up live in session.SlamSession: this is the driver over a finished sequence
    with session:
        if loads:
            start = int(config['checkpoint_time_idx'])
            session.load_reference_checkpoint(checkpoint_dir, start, dataset,
                                              tracking_item=None if tracking_dataset is None else tracking_dataset[0],
                                              densify_item=None if densify_dataset is None else densify_dataset[0])
        elif saves:
            session._refuse_checkpoints("save_checkpoints")
        # (the keyframe rule asks whether a pose is finite: answered once, from the dataset's host copy of the poses where it keeps one)
        host_poses = getattr(dataset, 'poses', None)
        finite = torch.isfinite(host_poses[:num_frames]).flatten(1).all(dim=1).tolist() \
            if isinstance(host_poses, torch.Tensor) and host_poses.device.type == "cpu" and host_poses.shape[0] >= num_frames else None
        for time_idx in range(start, num_frames):
            session._begin_frame()               # (reading the frame counts towards its prepare_frames phase and its frame_s)
            item = dataset[time_idx]
            tracking_item = tracking_dataset[time_idx] if tracking_dataset is not None else None
            densify_item = densify_dataset[time_idx] if densify_dataset is not None and session._densifies(time_idx) else None
            session.add_frame(*item, tracking_item=tracking_item, densify_item=densify_item,
                              _pose_finite=None if finite is None else bool(finite[time_idx]))
            if saves and time_idx % config['checkpoint_interval'] == 0:
                if exact_checkpoints:
                    session.save_checkpoint(checkpoint_dir, keyframes=False)
                else:
                    session.save_reference_checkpoint(checkpoint_dir, time_idx)
        params, variables, stats = session.finish()
    fused, eng, cam, mcfg = engine == "fused", session.engine, session.cam, config['mapping']
    if evaluate is not None:
        from . import evaluation
        opts = dict(evaluate)
        unknown = set(opts) - {'eval_every', 'eval_dir', 'ms_ssim', 'save_frames', 'lpips_weights'}
        if unknown:
            raise ValueError(f"evaluate: unknown keys {sorted(unknown)} (eval_every, eval_dir, ms_ssim, save_frames, lpips_weights)")
        if opts.get('lpips_weights') is None and config.get('lpips_weights') is not None:
            opts['lpips_weights'] = config['lpips_weights']
        box = [None]
        if rank == 0:
            with torch.no_grad():
                if fused:
                    eng.select_camera(cam)          # the evaluation renders the full-size frames
                box[0] = evaluation.evaluate(dataset, params, num_frames, mcfg['sil_thres'], mcfg['num_iters'], mcfg['add_new_gaussians'],
                                             engine=eng if fused else None, **opts)
        if world > 1:
            import torch.distributed as tdist
            tdist.broadcast_object_list(box, src=0)
        stats['eval'] = box[0]
    return params, variables, stats


def _track_frame(params, variables, curr_data, time_idx, tcfg, eng, stats):
    """Tracking iterations of one frame incl. the reference's doubling of the budget when the depth loss stays above
    ``depth_loss_thres`` (scripts/splatam.py:727-735).  Returns the number of iterations run."""
    num_iters = tcfg['num_iters']
    if eng is not None:
        eng.begin_tracking(time_idx)
    else:
        optimizer = slam.initialize_optimizer(params, tcfg['lrs'], tracking=True)
        state = slam.TrackingState(params, time_idx)
    # several ranks (replicated map and pose): each composites its band of tile rows, the partial sums are all-reduced, every rank
    # takes the same Adam step on the pose (FusedEngine.tracking_iteration); the outlier-rejecting loss needs the whole render
    from . import dist as sdist
    world, rank = sdist.world_size(), sdist.get_rank()
    shard = (rank, world) if (eng is not None and world > 1 and not tcfg['ignore_outlier_depth_loss']) else None
    it, todo, doubled, rounds = 0, num_iters, False, 0
    while todo:
        for _ in range(todo):
            if eng is not None:
                eng.tracking_iteration(curr_data, tcfg, shard=shard, allreduce_sums=sdist.all_reduce_sum_flat)
            else:
                loss, _ = slam.tracking_iteration(params, curr_data, variables, time_idx, optimizer, state, tcfg)
        it += todo
        todo = 0
        if eng is not None:
            lost = eng.settle("pose", sdist)       # (flagged iterations took no Adam step: the lists are re-sized, they are run again)
            if lost:
                stats['redone_iterations'] += lost
                if stats['redone_iterations'] > 100000:
                    raise RuntimeError(f"frame {time_idx} tracking: the per-tile lists keep overflowing")
                rounds += 1
                if rounds > 3:
                    raise RuntimeError(f"frame {time_idx}: the per-tile lists overflowed three times in a row")
                it -= lost
                todo = lost
                continue
        if it == num_iters and tcfg.get('use_depth_loss_thres', False) and not doubled:
            # the value the reference compares is the LAST iteration's weighted depth loss (scripts/splatam.py:728): no extra evaluation
            depth_loss = float(eng.buf['d_cam'][_capi.SPLAT_REPORT_DEPTH_TERM]) if eng is not None else float(state.last_losses['depth'].detach())
            if depth_loss >= tcfg['depth_loss_thres']:
                doubled, todo = True, num_iters
    if eng is not None:
        eng.end_tracking()
    else:
        state.commit(params)
    return it


def _track_frame_statements(params, variables, curr_data, time_idx, tcfg):
    """The tracking phase in the reference's own statements (scripts/splatam.py:680-744: optimizer per frame, get_loss -> backward ->
    step -> zero_grad, the host-side `if loss < current_min_loss`, the doubled budget) -- every name resolved in ``slam`` at call
    time, so that ``plugin.install(slam)`` is what runs."""
    optimizer = slam.initialize_optimizer(params, tcfg['lrs'], tracking=True)
    candidate_rot = params['cam_unnorm_rots'][..., time_idx].detach().clone()
    candidate_tran = params['cam_trans'][..., time_idx].detach().clone()
    current_min_loss = float(1e20)
    it, extended, budget = 0, False, tcfg['num_iters']
    while True:
        loss, variables, losses = slam.get_loss(params, curr_data, variables, time_idx, tcfg['loss_weights'], tcfg['use_sil_for_loss'],
                                                tcfg['sil_thres'], tcfg['use_l1'], tcfg['ignore_outlier_depth_loss'], tracking=True)
        loss.backward()
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        with torch.no_grad():
            if loss < current_min_loss:
                current_min_loss = loss
                candidate_rot = params['cam_unnorm_rots'][..., time_idx].detach().clone()
                candidate_tran = params['cam_trans'][..., time_idx].detach().clone()
        it += 1
        if it == budget:
            use_thres = tcfg.get('use_depth_loss_thres', False)
            if use_thres and losses['depth'] < tcfg['depth_loss_thres']:
                break
            if use_thres and not extended:
                extended, budget = True, 2 * budget
            else:
                break
    with torch.no_grad():
        params['cam_unnorm_rots'][..., time_idx] = candidate_rot
        params['cam_trans'][..., time_idx] = candidate_tran
    return it, variables


def _map_frame(params, variables, curr_data, time_idx, selected, keyframe_list, mcfg, eng, scene_radius, stats, phase, decided):
    """The mapping iterations of one frame over the selected keyframes + the current frame.  With ``world`` ranks every
    iteration draws ``world`` views from the SAME random stream on every rank; this rank renders its own one, the gradients are
    averaged by one all-reduce, every rank takes the same Adam step and the same pruning decisions.
    (Gradient-based densification accumulates the screen-space gradient of every iteration it sees, a flagged one included: its
    statistic is then one truncated-list sample short -- the map itself never moves on a flagged iteration.)"""
    from . import dist as sdist
    world, rank = sdist.world_size(), sdist.get_rank()
    cam, intrinsics, w2c0 = curr_data['cam'], curr_data['intrinsics'], curr_data['w2c']
    prune, pd = mcfg['prune_gaussians'], mcfg['pruning_dict']
    dev = params['means3D'].device
    if world > 1 and mcfg.get('use_gaussian_splatting_densification'):
        # every rank renders another view: means2D_gradient_accum / denom / max_2D_radius would differ between the replicas and
        # so would the clone / split selection -- the replicated-map invariant of the multi-rank loop does not hold
        raise NotImplementedError("gradient-based densification is not supported in the multi-rank frame loop")
    bucket = None                   # drop-in path: flat gradient bucket, re-made when an edit changes the number of rows
    if eng is not None:
        eng.reset_map_optimizer()
    else:
        optimizer = slam.initialize_optimizer(params, mcfg['lrs'], tracking=False)

    def iteration(it):
        nonlocal bucket
        if world == 1:
            sel = selected[np.random.randint(0, len(selected))]
        else:
            sel = selected[int(np.random.randint(0, len(selected), size=world)[rank])]
        if sel == -1:
            iter_time_idx, iter_color, iter_depth = time_idx, curr_data['im'], curr_data['depth']
        else:
            kf = keyframe_list[sel]
            iter_time_idx, iter_color, iter_depth = kf['id'], kf['color'], kf['depth']
        iter_data = {'cam': cam, 'im': iter_color, 'depth': iter_depth, 'id': iter_time_idx, 'intrinsics': intrinsics, 'w2c': w2c0}
        decided['views'].append(int(iter_time_idx))
        # the reference prunes between backward() and step(); remove_points re-creates the parameters without their
        # gradients, so an iteration on the pruning schedule takes no Adam step
        # (prune_gaussians also resets the opacities on its own schedule: utils/slam_external.py:186-190)
        sched = slam.edit_schedule(it, pd, 'prune_every') if prune else None
        on_schedule, resets = prune and sched.edits, prune and sched.resets
        if eng is not None and world == 1 and not on_schedule and not resets and not mcfg.get('use_gaussian_splatting_densification'):
            # nothing between backward() and step() in this iteration: one call, the Adam step rides in the last kernel
            eng.mapping_iteration(iter_data, iter_time_idx, mcfg)
        elif eng is not None:
            eng.loss_backward(iter_data, iter_time_idx, mcfg, tracking=False)
            if world > 1 and not on_schedule:                   # (an iteration on the pruning schedule takes no Adam step)
                # (with every rank's capacity flag in the bucket's header: a rank whose lists overflowed stops ALL replicas' steps)
                eng.exchange_gradients(sdist.all_reduce_mean_flat)
            edited = False
            dens = slam.edit_schedule(it, mcfg['densify_dict'], 'densify_every') if mcfg.get('use_gaussian_splatting_densification') else None
            if dens is not None and dens.active:
                # the colour pass' screen-space gradient is accumulated from THIS iteration's workspace (lists, radii, features
                # indexed by the rows the render saw): before any row is removed
                eng.accumulate_mean2d_gradient()
            if prune and (on_schedule or resets):
                rows = eng.P
                with phase("prune"):
                    edited = bool(eng.prune_gaussians(it, pd, scene_radius))
                if on_schedule:
                    decided['prunes'].append((it, rows, eng.P))
            if dens is not None:                                         # scripts/splatam.py:864-867
                edited = bool(eng.densify(it, mcfg['densify_dict'], scene_radius, accumulate=False)) or edited
                on_schedule = on_schedule or dens.edits                   # re-created parameters carry no gradient: no Adam step
            if edited:
                sdist.assert_replicated_count(eng.P, f"map edit (frame {time_idx}, iteration {it})", dev)
                if not eng.lists_known():
                    with phase("relearn_lists"):
                        eng.relearn_lists(curr_data, time_idx)
            if not on_schedule:
                eng.adam_map(mcfg['lrs'])
        else:
            loss, _, _ = slam.get_loss(params, iter_data, variables, iter_time_idx, mcfg['loss_weights'], mcfg['use_sil_for_loss'],
                                       mcfg['sil_thres'], mcfg['use_l1'], mcfg['ignore_outlier_depth_loss'], mapping=True)
            loss.backward()
            if world > 1 and not on_schedule:
                if bucket is None or bucket.sizes != [params[k].numel() for k in bucket.keys]:
                    bucket = sdist.GradBucket(params)
                bucket.all_reduce_mean(params)
            with torch.no_grad():
                if prune:
                    n_before = params['means3D'].shape[0]
                    if on_schedule or resets:
                        with phase("prune"):
                            slam.prune_gaussians(params, variables, optimizer, it, pd)
                    else:                                       # (the reference calls it every iteration; off schedule it does nothing)
                        slam.prune_gaussians(params, variables, optimizer, it, pd)
                    if on_schedule:
                        decided['prunes'].append((it, n_before, int(params['means3D'].shape[0])))
                    if params['means3D'].shape[0] != n_before:
                        sdist.assert_replicated_count(int(params['means3D'].shape[0]), f"prune_gaussians (frame {time_idx}, iteration {it})", dev)
                optimizer.step()
                optimizer.zero_grad(set_to_none=True)

    it, todo, rounds = 0, mcfg['num_iters'], 0
    while todo:
        for _ in range(todo):
            iteration(it)
            it += 1
        todo = 0
        if eng is not None:
            todo = eng.settle("map", sdist)
            if todo:
                stats['redone_iterations'] += todo
                if stats['redone_iterations'] > 100000:
                    raise RuntimeError(f"frame {time_idx} mapping: the per-tile lists keep overflowing")
                rounds += 1
                if rounds > 3:
                    raise RuntimeError(f"frame {time_idx}: the per-tile lists overflowed three times in a row")


def _matrix_to_quaternion(R):
    """``slam.matrix_to_quaternion`` in double, as the [1, 4] float32 row of ``cam_unnorm_rots`` that ``use_gt_poses`` writes
    (scripts/splatam.py:745-754)."""
    return slam.matrix_to_quaternion(R.reshape(3, 3).double()).float().reshape(1, 4)
