"""Evaluation of a finished run: what the reference's ``eval`` (utils/eval_helpers.py:408-623) reports -- PSNR, depth "RMSE",
depth L1 and MS-SSIM of the evaluated frames rendered from the final map, and the trajectory error -- without a host read per
frame: every frame is one ``FusedEngine.evaluate_frame`` (render + metric kernels, csrc/evalmetrics.hip) that writes a row of a
device table, and the table is read ONCE.

Kept from the reference, quirks included (each is pinned by tests/golden/eval_reference.npz):
  * frame selection: frame 0 and every frame with ``(t + 1) % eval_every == 0``;
  * mask variant: with ``mapping_iters == 0 and not add_new_gaussians`` images are weighted by presence * valid and the depth
    difference by presence, otherwise images by valid (``slam.eval_frame_metrics``);
  * "depth RMSE" takes its square root per pixel and therefore equals depth L1;
  * the trajectory error aligns the translation columns of the world-to-camera matrices, skips frames whose ground-truth pose
    holds a NaN, and is a MEAN distance reported as "ATE RMSE" (``slam.evaluate_ate``).
``save_frames=True`` writes the reference's four picture directories (``rendered_rgb/gs_%04d.png``, ``rendered_depth/gs_%04d.png``,
``rgb/gt_%04d.png``, ``depth/gt_%04d.png``: eval_helpers.py:418-426, 509-528) from the planes the evaluation render left, through
splat_view_finish (csrc/view.hip); the depth pictures carry matplotlib's jet, not ``cv2.COLORMAP_JET`` (``splatam_amd.view``).
Not kept: the plots.  LPIPS is computed when the caller supplies the AlexNet weights (``lpips_weights``: a path or an
``lpips.LpipsWeights``; csrc/lpips.hip writes slot 7 of the frame's row, still without a host read) -- this package carries none and
downloads none, and without them the result says ``lpips: None`` instead of a made-up number.  A failure in the trajectory error is
raised, not replaced by 100.0.

``evaluate_novel_views`` is the reference's ``eval_nvs`` (utils/eval_helpers.py:626-825) in the same manner: the finished map scored
at HELD-OUT poses (a dataset's test split, whose item 0 is the first training frame), one ``FusedEngine.evaluate_view`` per frame,
the table read once; frames with holes -- pixels that have depth where the map shows nothing -- stay out of the averages.  Both are
thin callers of ``_evaluate``, which enqueues, reads and repeats through ``map_pass.run_pass``.
"""
from __future__ import annotations

import contextlib
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import _capi, slam


def eval_frame_indices(num_frames, eval_every=1):
    """Frames the reference evaluates: 0 and every t with (t + 1) % eval_every == 0."""
    return [t for t in range(int(num_frames)) if t == 0 or (t + 1) % int(eval_every) == 0]


def uses_silhouette_mask(mapping_iters, add_new_gaussians):
    """The reference's choice of mask variant: a run that never mapped and never densified is judged where it has a map."""
    return int(mapping_iters) == 0 and not add_new_gaussians


def trajectory_error(params, first_frame_w2c, gt_poses, num_frames=None):
    """``ate_rmse`` of the reference's ``eval``: estimated poses = the first frame's world-to-camera, then for every later frame the
    pose in ``params`` RELATIVE to the first frame (as stored); ground truth = inverses of the dataset poses ``gt_poses`` [n,4,4];
    frames after the first whose ground-truth pose holds a NaN are skipped on both sides.  Host work (inverses check their status
    on the host): call it after the metric table has been read."""
    gt_poses = torch.as_tensor(gt_poses)
    n = min(int(params['cam_unnorm_rots'].shape[-1]), int(gt_poses.shape[0]))
    if num_frames is not None:
        n = min(n, int(num_frames))
    bad = torch.isnan(gt_poses.reshape(gt_poses.shape[0], -1)).any(dim=1).cpu().tolist()
    dev = first_frame_w2c.device
    est, gt = [first_frame_w2c.detach().float()], [torch.linalg.inv(gt_poses[0].to(dev).float())]
    for idx in range(1, n):
        if bad[idx]:
            continue
        rel = torch.eye(4, device=dev)
        rel[:3, :3] = slam.build_rotation(F.normalize(params['cam_unnorm_rots'][..., idx].detach()))[0]
        rel[:3, 3] = params['cam_trans'][0, :, idx].detach()
        est.append(rel)
        gt.append(torch.linalg.inv(gt_poses[idx].to(dev).float()))
    return slam.evaluate_ate(gt, est)


def _frame(dataset, t):
    color, depth, intrinsics, pose = dataset[t]
    return (color.permute(2, 0, 1) / 255).contiguous(), depth.permute(2, 0, 1).contiguous(), intrinsics[:3, :3], pose


def _read_table(table):
    """THE host read of an evaluation."""
    return table.cpu().numpy()


def _mirror_row(params, curr_data, t, sil_thres, sil_mask, ms_ssim, lpips_weights=None):
    """One frame by the torch mirror: the reference's two renders through ``slam.Renderer`` + ``slam.eval_frame_metrics``."""
    with torch.no_grad():
        p = {k: v.detach() for k, v in params.items()}
        tg = slam.transform_to_frame(p, t, gaussians_grad=False, camera_grad=False)
        depth_sil, _, _ = slam.Renderer(raster_settings=curr_data['cam'])(**slam.transformed_params2depthplussilhouette(p, curr_data['w2c'], tg))
        im, _, _ = slam.Renderer(raster_settings=curr_data['cam'])(**slam.transformed_params2rendervar(p, tg))
        m = slam.eval_frame_metrics(im, depth_sil, curr_data, sil_thres, sil_mask, with_ms_ssim=ms_ssim, lpips_weights=lpips_weights)
    nan = torch.full((), float("nan"))
    zero = torch.zeros((), dtype=torch.float64)
    vals = [m['psnr'], m['depth_rmse'], m['depth_l1'], m['ms_ssim'] if ms_ssim else nan, m['valid'], zero, zero, m.get('lpips', zero)]
    return torch.stack([v.detach().double().cpu() for v in vals])


class _FrameSaver:
    """``save_frames``: per evaluated frame four pictures [H, W, 3] uint8 -- rendered colour and depth from the planes the evaluation
    render left, the ground-truth frame's colour and depth (its image, its depth, a silhouette of ones) -- formed on the device by
    splat_view_finish, copied into one of ``SLOTS`` pinned slots on the current stream (an event after the copy) and encoded to PNG
    by a small thread pool, which waits for the slot's event, not the evaluation.  A slot is reused once its PNGs are written."""
    SLOTS, WORKERS = 4, 4
    NAMES = (("rendered_rgb", "gs"), ("rendered_depth", "gs"), ("rgb", "gt"), ("depth", "gt"))

    def __init__(self, eval_dir, dev, H, W, rendered_prefix="gs"):
        from concurrent.futures import ThreadPoolExecutor
        from .view import jet_lut
        if torch.device(dev).type != "cuda":
            raise ValueError(f"save_frames forms the pictures on a HIP device (the frames are on {dev})")
        self.names = tuple((d, rendered_prefix if d.startswith("rendered_") else p) for d, p in self.NAMES)    # (eval_nvs: splatam_%04d.png)
        self.dirs = [os.path.join(eval_dir, d) for d, _ in self.NAMES]
        for d in self.dirs:
            os.makedirs(d, exist_ok=True)
        self.dev = dev
        self.lut = torch.from_numpy(jet_lut()).to(dev)
        self.bytes = torch.zeros(4, H, W, 3, dtype=torch.uint8, device=dev)
        self.gt6 = torch.ones(5, H, W, dtype=torch.float32, device=dev)        # plane 4, the silhouette, stays 1
        self.slots = [dict(host=torch.empty(4, H, W, 3, dtype=torch.uint8, pin_memory=True), event=torch.cuda.Event(), jobs=[]) for _ in range(self.SLOTS)]
        self.turn = 0
        self.by_frame = {}              # frame -> its PNG jobs: a frame saved again (evaluated again on re-learnt lists) waits for them
        self.pool = ThreadPoolExecutor(max_workers=self.WORKERS)

    def save(self, t, out6, im, depth):
        """Enqueue frame ``t``: ``out6`` the render's planes, ``im`` [3, H, W] / ``depth`` [1, H, W] the ground truth."""
        from .fused import view_finish
        from PIL import Image
        view_finish(out6, "color", rgb8=self.bytes[0])
        view_finish(out6, "depth", lut=self.lut, rgb8=self.bytes[1])           # (vmin 0, vmax 6: eval_helpers.py:513-514)
        self.gt6[0:3], self.gt6[3] = im, depth[0]
        view_finish(self.gt6, "color", rgb8=self.bytes[2])
        view_finish(self.gt6, "depth", lut=self.lut, rgb8=self.bytes[3])
        slot = self.slots[self.turn]
        self.turn = (self.turn + 1) % self.SLOTS
        for job in slot['jobs'] + self.by_frame.pop(t, []):
            job.result()                                                       # (the PNGs of the slot's previous frame, and any earlier ones of THIS frame, are written)
        slot['host'].copy_(self.bytes, non_blocking=True)
        slot['event'].record(torch.cuda.current_stream(self.dev))
        host, event = slot['host'].numpy(), slot['event']

        def write(i):
            event.synchronize()
            Image.fromarray(host[i]).save(os.path.join(self.dirs[i], f"{self.names[i][1]}_{t:04d}.png"))
        slot['jobs'] = self.by_frame[t] = [self.pool.submit(write, i) for i in range(4)]

    def close(self):
        """Every PNG is on disk (a failed write raises here) and the pool is gone."""
        try:
            for slot in self.slots:
                for job in slot['jobs']:
                    job.result()
        finally:
            self.pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.pool.shutdown(wait=True)                                      # (the evaluation failed: its own error is the one to raise)


def _lpips_arguments(lpips_weights, dev, mirror):
    """(weights or None, keyword arguments for evaluate_frame / evaluate_view): without weights NOTHING is passed on, so the calls are
    the ones they were."""
    from . import lpips as lp
    if isinstance(lpips_weights, lp.Lpips):                 # (a caller that evaluates often keeps the packed network)
        if mirror:
            raise ValueError("the mirror engine takes the weights (a path or LpipsWeights), not a device network")
        return lpips_weights, {'lpips': lpips_weights}
    weights = lp.as_weights(lpips_weights)
    if weights is None or mirror:
        return weights, {}
    return weights, {'lpips': lp.Lpips(weights, dev)}


def _evaluate(dataset, params, num_frames, sil_thres, mapping_iters, add_new_gaussians, eval_every, engine, eval_dir, ms_ssim, save_frames,
              lpips_weights, *, indices, item_of, every_pose, steps, what, rendered_prefix="gs", validity=None):
    """The body of ``evaluate`` and ``evaluate_novel_views`` (their arguments, then what differs between them).  ``indices(num_frames,
    eval_every)``: the scored indices, ``item_of(index)`` the dataset item of one; ``every_pose``: every item of the dataset is visited
    (its pose kept in ``env.poses``), not the scored ones alone.  ``steps(env)`` returns ``(locate, learn, score)``: ``locate(pose)``
    forms, once per scored item, what the other two receive as ``at`` (None: the pose itself); ``learn(t, data, at, again)`` learns the
    lists on item ``t`` (``again``: for a flagged item, after a reset of the camera's status; None on the mirror); ``score(t, data, at,
    row)`` enqueues item ``t``'s metrics into ``row`` -- the mirror instead returns them as a host row -- and returns ``(host row or
    None, the rendered planes or None)``.  ``validity(out, host, env)`` may add entries to the result and returns
    the mask of the frames the averages run over (None: all).  ``what`` names a frame in the error of a row that stays flagged.
    Returns ``(result, env)``; ``env`` carries what the set-up made (engine, mirror, dev, H, W, intrinsics, first_frame_w2c, sil_mask,
    the LPIPS arguments) and ``poses``, the poses of the visited items."""
    from types import SimpleNamespace
    from .fused import FusedEngine
    from .map_pass import run_pass
    t_start = time.perf_counter()
    num_frames = min(int(num_frames), len(dataset))
    frames = indices(num_frames, eval_every)
    sil_mask = uses_silhouette_mask(mapping_iters, add_new_gaussians)
    color0, depth0, intrinsics, pose0 = _frame(dataset, 0)
    dev = depth0.device
    H, W = int(color0.shape[1]), int(color0.shape[2])
    first_frame_w2c = torch.linalg.inv(pose0).to(dev).float().contiguous()
    mirror = isinstance(engine, str)
    if mirror and engine != "mirror":
        raise ValueError(f"engine must be a FusedEngine, None or 'mirror' (got {engine!r})")
    if not mirror and engine is not None and not isinstance(engine, FusedEngine):
        raise ValueError(f"engine must be a FusedEngine, None or 'mirror' (got {type(engine).__name__})")
    if ms_ssim and min(H, W) <= 160:
        raise ValueError(f"MS-SSIM needs frames with min(H, W) > 160 (got {(H, W)}); pass ms_ssim=False")
    if save_frames and eval_dir is None:
        raise ValueError("save_frames needs eval_dir")
    if mirror or engine is None:
        cam = slam.setup_camera(W, H, intrinsics.cpu().numpy(), first_frame_w2c.detach().cpu().numpy(), device=dev)
        if engine is None:
            engine = FusedEngine({k: v.detach().float().contiguous() for k, v in params.items()}, cam)
    else:
        cam = engine.cam_settings
    lpips_w, lpips_kw = _lpips_arguments(lpips_weights, dev, mirror)
    env = SimpleNamespace(engine=engine, mirror=mirror, dev=dev, H=H, W=W, intrinsics=intrinsics, first_frame_w2c=first_frame_w2c,
                          sil_mask=sil_mask, lpips_w=lpips_w, lpips_kw=lpips_kw, poses=[], host=None)
    locate, learn, score = steps(env)
    row_of = {item_of(k): i for i, k in enumerate(frames)}
    items = list(range(num_frames)) if every_pose else list(row_of)
    table = torch.zeros(max(len(frames), 1), _capi.SPLAT_EVAL_ROW, dtype=torch.float64, device="cpu" if mirror else dev)[:len(frames)]

    def item(t):
        color, depth, _, pose = _frame(dataset, t)
        return {'cam': cam, 'im': color, 'depth': depth, 'id': t, 'intrinsics': intrinsics, 'w2c': first_frame_w2c}, pose

    def put(t, data, at, row):
        values, planes = score(t, data, at, row)
        if values is not None:
            row.copy_(values)
        return planes

    def save(t, data, planes):
        if saver is not None:
            saver.save(frames[row_of[t]], planes, data['im'], data['depth'])

    def enqueue(n, t):
        data, pose = item(t)
        env.poses.append(pose)
        if t not in row_of:
            return
        at = pose if locate is None else locate(pose)
        if learn is not None and n == first:              # (one read: sizes the list buckets for the map as it is)
            learn(t, data, at, False)
        save(t, data, put(t, data, at, table[row_of[t]]))

    def read():
        env.host = _read_table(table)
        return [n for n, t in enumerate(items) if t in row_of and env.host[row_of[t], _capi.SPLAT_EVAL_FLAGGED] != 0]

    def redo(n, t):
        # this view's lists outgrew the buckets learnt on the first scored one: its row was formed on truncated lists.  Re-learn on this
        # view (exact lists, capacity grown as needed) and evaluate it again
        data, pose = item(t)
        at = pose if locate is None else locate(pose)
        learn(t, data, at, True)
        again = torch.zeros(_capi.SPLAT_EVAL_ROW, dtype=torch.float64, device=dev)
        planes = put(t, data, at, again)
        env.host[row_of[t]] = _read_table(again)
        if env.host[row_of[t], _capi.SPLAT_EVAL_FLAGGED] != 0:
            raise RuntimeError(f"{what} {frames[row_of[t]]}: the per-tile lists could not be sized for its evaluation render")
        save(t, data, planes)                                  # (its pictures again, from the complete lists)

    first = min((n for n, t in enumerate(items) if t in row_of), default=None)
    saver = _FrameSaver(eval_dir, dev, H, W, rendered_prefix) if save_frames else None
    with saver if saver is not None else contextlib.nullcontext():       # (leaving it: every PNG is on disk, the pool shut down)
        repeated = [frames[row_of[t]] for t in run_pass(items, enqueue, read, redo)]
    t_metrics = time.perf_counter() - t_start          # (the table read above waited for the device)
    host = env.host
    out = {'frames': list(frames), 'eval_s': t_metrics, 'eval_ms_per_frame': 1e3 * t_metrics / max(len(frames), 1), 'psnr': host[:, _capi.SPLAT_EVAL_PSNR].copy(),
           'depth_rmse': host[:, _capi.SPLAT_EVAL_DEPTH_RMSE].copy(), 'depth_l1': host[:, _capi.SPLAT_EVAL_DEPTH_L1].copy(),
           'ms_ssim': host[:, _capi.SPLAT_EVAL_MS_SSIM].copy(), 'valid_pixels': host[:, _capi.SPLAT_EVAL_VALID].copy(), 'lpips': None,
           'repeated': repeated, 'sil_mask': bool(sil_mask)}
    valid = validity(out, host, env) if validity is not None else np.ones(len(frames), dtype=bool)
    if lpips_w is not None:
        out['lpips'] = host[:, _capi.SPLAT_EVAL_LPIPS].copy()
    for k in ('psnr', 'depth_rmse', 'depth_l1', 'ms_ssim') + (('lpips',) if lpips_w is not None else ()):
        out['avg_' + k] = float(out[k][valid].mean()) if valid.any() else float("nan")       # (numpy's mean of nothing, without its warning)
    if eval_dir is not None:
        os.makedirs(eval_dir, exist_ok=True)
        for name, k in (("psnr.txt", 'psnr'), ("rmse.txt", 'depth_rmse'), ("l1.txt", 'depth_l1'), ("ssim.txt", 'ms_ssim')) + ((("lpips.txt", 'lpips'),) if lpips_w is not None else ()):
            np.savetxt(os.path.join(eval_dir, name), out[k])
    return out, env


def evaluate(dataset, params, num_frames, sil_thres, mapping_iters, add_new_gaussians, eval_every=1, engine=None, eval_dir=None,
             ms_ssim=True, save_frames=False, lpips_weights=None):
    """Evaluates ``params`` (the final map and trajectory of a run over ``dataset``) on frames ``eval_frame_indices(num_frames,
    eval_every)``.  Returns a dict: per-frame float64 arrays ``psnr``, ``depth_rmse``, ``depth_l1``, ``ms_ssim`` (NaN when
    ``ms_ssim=False``), their means ``avg_psnr`` ..., ``ate_rmse``, ``frames`` (the evaluated indices), ``lpips`` / ``avg_lpips``
    (with ``lpips_weights`` -- a path ``lpips.load_weights`` reads, an ``lpips.LpipsWeights``, or an ``lpips.Lpips`` already on the device --: the per-frame array and its mean;
    without: ``lpips`` is None, there is no ``avg_lpips``, and nothing more is launched),
    ``repeated`` (frames evaluated twice because their render outgrew the learnt list buckets), ``eval_s`` / ``eval_ms_per_frame`` (wall
    time from the call to the table read, dataset access and list learning included).  With ``eval_dir`` the reference's text
    files psnr.txt, rmse.txt, l1.txt, ssim.txt (and lpips.txt with ``lpips_weights``) are written there; ``save_frames`` (needs ``eval_dir`` and an engine) also writes the
    evaluated frames as PNGs (``_FrameSaver``) -- the metrics and their single table read are the same with and without it.

    ``engine``: a ``FusedEngine`` that holds ``params`` (it evaluates on its own map), ``None`` (a throw-away engine is built
    around ``params``), or the string ``"mirror"``: the torch mirror (``slam.eval_frame_metrics`` on two ``slam.Renderer`` calls per
    frame, one host copy per frame) -- the parity target, and the only form that runs without a GPU.

    Host synchronisation on an engine: one read to learn the list statistics (``relearn_lists``) before the first frame; then every
    frame is enqueued; one read fetches the table; flagged rows (rare) are evaluated again on re-learnt lists."""
    if save_frames and (eval_dir is None or isinstance(engine, str)):
        raise ValueError("save_frames needs eval_dir and an engine (the pictures are formed on the device)")

    def steps(env):
        if env.mirror:
            return None, None, lambda t, data, at, row: (_mirror_row(params, data, t, sil_thres, env.sil_mask, ms_ssim, env.lpips_w), None)
        eng = env.engine

        def learn(t, data, at, again):
            if again:
                eng._camera.reset_status()
            eng.relearn_lists(data, t)

        def score(t, data, at, row):
            eng.evaluate_frame(data, t, row, sil_thres, sil_mask=env.sil_mask, ms_ssim=ms_ssim, **env.lpips_kw)
            return None, eng.buf['out6']
        return None, learn, score

    out, env = _evaluate(dataset, params, num_frames, sil_thres, mapping_iters, add_new_gaussians, eval_every, engine, eval_dir, ms_ssim,
                         save_frames, lpips_weights, indices=eval_frame_indices, item_of=lambda t: t, every_pose=True, steps=steps, what="frame")
    # (every frame's pose feeds the trajectory error)
    out['ate_rmse'] = trajectory_error(params, env.first_frame_w2c, torch.stack([p.detach().to(env.dev).float() for p in env.poses]), len(env.poses))
    return out


# ---------------------------------------------------------------------- novel views (the reference's eval_nvs)
def novel_view_indices(num_frames, eval_every=1):
    """Held-out indices k = t - 1 the reference scores among items 1 .. num_frames - 1 of a test split (item 0 is the first training
    frame): k = 0 and every k with (k + 1) % eval_every == 0."""
    return [k for k in range(max(int(num_frames) - 1, 0)) if k == 0 or (k + 1) % int(eval_every) == 0]


def percent_holes(holes, height, width):
    """``holes / (H W) * 100`` as torch evaluates the reference's expression: an integer count divided by a Python int is float32."""
    return np.asarray(holes).astype(np.float32) / np.float32(int(height) * int(width)) * np.float32(100)


def _rigid_inverse(m):
    """inv of a rigid [4, 4] as [R^T, -R^T t]: elementwise work that enqueues without a host read (``torch.linalg.inv`` reads its status)."""
    rt = m[:3, :3].t()
    return torch.cat([torch.cat([rt, -(rt @ m[:3, 3:4])], dim=1), m[3:4]], dim=0)        # (the last row of a rigid matrix is its own)


def _mirror_nvs_row(params, curr_data, gt_w2c, sil_thres, sil_mask, ms_ssim, lpips_weights=None):
    """One held-out frame by the torch mirror, rendered the way eval_nvs renders it: the centres are moved by ``gt_w2c`` (and for an
    anisotropic map the rotations composed with its quaternion), then seen through the first frame's camera and depth row.  Returns
    (row, planes [5, H, W]: r, g, b, depth, silhouette)."""
    with torch.no_grad():
        p = {k: v.detach() for k, v in params.items()}
        pts = p['means3D']
        pts4 = torch.cat((pts, torch.ones_like(pts[:, :1])), dim=1)
        tg = {'means3D': (gt_w2c @ pts4.T).T[:, :3]}
        if p['log_scales'].shape[1] == 1:
            tg['unnorm_rotations'] = p['unnorm_rotations']
        else:
            q = F.normalize(slam.matrix_to_quaternion(gt_w2c[:3, :3]).unsqueeze(0))
            tg['unnorm_rotations'] = slam.quat_mult(q, F.normalize(p['unnorm_rotations']))
        depth_sil, _, _ = slam.Renderer(raster_settings=curr_data['cam'])(**slam.transformed_params2depthplussilhouette(p, curr_data['w2c'], tg))
        im, _, _ = slam.Renderer(raster_settings=curr_data['cam'])(**slam.transformed_params2rendervar(p, tg))
        m = slam.eval_frame_metrics(im, depth_sil, curr_data, sil_thres, sil_mask, with_ms_ssim=ms_ssim, lpips_weights=lpips_weights)
        holes = (~((depth_sil[1] > sil_thres) | ~(curr_data['depth'][0] > 0))).sum()
    nan = torch.full((), float("nan"))
    zero = torch.zeros((), dtype=torch.float64)
    vals = [m['psnr'], m['depth_rmse'], m['depth_l1'], m['ms_ssim'] if ms_ssim else nan, m['valid'], zero, holes, m.get('lpips', zero)]
    return torch.stack([v.detach().double().cpu() for v in vals]), torch.cat([im, depth_sil[0:2]]).contiguous()


def evaluate_novel_views(dataset, params, num_frames, sil_thres, mapping_iters, add_new_gaussians, eval_every=1, engine=None, eval_dir=None,
                         ms_ssim=True, save_frames=False, lpips_weights=None):
    """Novel-view synthesis of a finished map, with the semantics of the reference's ``eval_nvs``.  ``dataset`` is a held-out split:
    item 0 is the first training frame -- it only supplies ``first_frame_w2c = inv(pose_0)`` and the camera, and is not scored --,
    items 1 .. num_frames - 1 are the held-out frames; index k = t - 1 is scored when ``k == 0 or (k + 1) % eval_every == 0``.  The
    effective world-to-camera of item t is ``first_frame_w2c @ inv(pose_t)`` (eval_nvs moves the Gaussians by ``inv(pose_t)`` and
    looks at them through the camera and the depth row of ``first_frame_w2c``).  Mask variant and metrics as in ``evaluate`` (the
    "RMSE" that equals L1 included); ``params`` needs no trajectory.

    A frame is VALID unless ``holes / (H W) * 100 > 0.1`` (in float32, as torch evaluates it), holes = pixels with depth > 0 whose
    silhouette is not above ``sil_thres``.  Returns the dict of ``evaluate`` without ``ate_rmse`` -- ``frames`` are the scored k,
    the per-frame arrays hold ALL scored frames, the four averages run over the VALID frames only (NaN when there is none) -- and
    ``holes`` (int64 per frame), ``percent_holes`` (float32), ``valid_nvs_frames`` (bool), ``lpips: None`` -- or, with
    ``lpips_weights`` (as in ``evaluate``), ``lpips`` per scored frame and ``avg_lpips`` over the VALID frames.  With ``eval_dir``:
    psnr.txt, rmse.txt, l1.txt, ssim.txt (lpips.txt with weights) and valid_nvs_frames.npy; with ``save_frames`` also the four picture directories with
    ``splatam_%04d.png`` (rendered) and ``gt_%04d.png``, numbered by k.

    ``engine``: a ``FusedEngine`` that holds the map, ``None`` (a throw-away one) or ``"mirror"`` (torch, runs without a GPU: the
    parity target).  On an engine a view camera of the frame's size is moved from pose to pose (``evaluate_view``: the engine's own
    camera, map and optimiser state stay untouched; the poses must be rigid); host synchronisation as in ``evaluate``: one read to
    learn the view's list statistics on the first held-out pose, every frame enqueued, one table read, flagged rows again."""
    from .fused import _intrinsics4
    if min(int(num_frames), len(dataset)) < 1:
        raise ValueError("a held-out split starts with the first training frame: the dataset is empty")

    def steps(env):
        if env.mirror:
            return torch.linalg.inv, None, lambda t, data, gt_w2c, row: _mirror_nvs_row(params, data, gt_w2c, sil_thres, env.sil_mask, ms_ssim, env.lpips_w)
        eng, view = env.engine, env.engine.view_camera(env.W, env.H)
        k_host = _intrinsics4(env.intrinsics)                             # (on the host once: a device matrix would be read per view)

        def locate(pose):                                                 # (the item's effective world-to-camera: its learn and its score step share it)
            return (env.first_frame_w2c @ _rigid_inverse(pose.to(env.dev).float())).contiguous()

        def learn(t, data, w2c, again):
            if again:
                view.camera.reset_status()
            eng.relearn_lists(data, 0, view=view, w2c=w2c, intrinsics=k_host)

        def score(t, data, w2c, row):
            eng.evaluate_view(view, w2c, data, row, sil_thres, sil_mask=env.sil_mask, ms_ssim=ms_ssim, holes=True, intrinsics=k_host, **env.lpips_kw)
            return None, view.camera.buf['out6']
        return locate, learn, score

    def validity(out, host, env):
        out['holes'] = np.rint(host[:, _capi.SPLAT_EVAL_HOLES]).astype(np.int64)
        out['percent_holes'] = percent_holes(out['holes'], env.H, env.W)
        out['valid_nvs_frames'] = ~(out['percent_holes'] > np.float32(0.1))
        return out['valid_nvs_frames']

    out, _ = _evaluate(dataset, params, num_frames, sil_thres, mapping_iters, add_new_gaussians, eval_every, engine, eval_dir, ms_ssim,
                       save_frames, lpips_weights, indices=novel_view_indices, item_of=lambda k: k + 1, every_pose=False, steps=steps,
                       what="held-out frame", rendered_prefix="splatam", validity=validity)
    if eval_dir is not None:
        np.save(os.path.join(eval_dir, "valid_nvs_frames.npy"), out['valid_nvs_frames'])
    return out
