"""``python -m splatam_amd.post_opt CONFIG.py``: refines the map of a finished run (the reference's ``scripts/post_splatam_opt.py``).

The file is one of the reference's own experiment files (configs/<dataset>/post_splatam_opt.py); this package ships none.  What the
script does, restated (line numbers: /root/reference/scripts/post_splatam_opt.py), quirks kept:

  * loading (:68-108): ``config['data']['param_ckpt_path']`` is a ``params.npz``; ``intrinsics, w2c, org_width, org_height,
    gt_w2c_all_frames, keyframe_time_indices`` are dropped, every other entry becomes a float32 tensor, ``timestep`` moves to
    ``variables``, ``max_2D_radius / means2D_gradient_accum / denom`` start at zero, ``scene_radius = max(depth of frame 0) / 2``
    (a 2 of its own, not ``scene_radius_depth_ratio``);
  * frames (:238-262): EVERY mapping frame (``stride``) is held on the device, colour ``/ 255``; the pose of frame ``t`` is the
    ESTIMATED one, ``build_rotation(normalize(cam_unnorm_rots[..., t])), cam_trans[..., t]`` of the loaded map -- no first-frame
    matrix -- and the evaluation runs on a dataset of its own (``eval_stride``);
  * the loop (:265-347): the outer loop over the frames does nothing until the last frame, where ``num_iters_mapping`` iterations
    run; each: the ``means3D`` rate for ``iter + 1`` (``get_expon_lr_func``; the script passes ``lr_delay_mult`` without
    ``lr_delay_steps``, so it has no effect), a frame from ``random.randint(0, time_idx)`` (Python's generator), ``get_loss_gs`` +
    backward, ``densify(iter, densify_dict)`` when ``use_gaussian_splatting_densification``, the Adam step.  ``densify`` re-creates
    the five Gaussian parameters on its schedule, so THAT iteration's ``optimizer.step()`` moves nothing (as the frame loop's
    pruning iterations, ``pipeline._map_frame``); an opacity reset re-creates ``logit_opacities`` alone, so on a reset iteration
    off the densification schedule that group alone takes no step (on the fused engine ``_reset_opacities`` zeroes the group's
    gradient and moments and the Adam kernel leaves such elements as they are; the group's bias corrections run on the engine's one
    step count, i.e. one step ahead of torch's per-parameter count after each reset, as in the frame loop);
  * evaluation (:333-345, :357-366): at ``iter + 1 == 7000`` into ``eval_7k/`` and at the end into ``eval/``, both as
    ``eval(..., mapping_iters=num_iters_mapping, add_new_gaussians=True)``;
  * output (:368-381): ``params.npz`` with the map, ``timestep``, ``intrinsics`` (the dataset item's matrix as it is), ``w2c`` (first
    frame), ``org_width / org_height`` and ``gt_w2c_all_frames`` -- which here holds the ESTIMATED poses the loop rendered from;
    ``keyframe_time_indices`` is not written back.

Engines: ``"fused"`` (one FusedEngine that owns the map; the loss is the ``gs`` mode of the fused mapping iteration, the camera the
engine's transform to frame ``t`` with ``curr_data['w2c']`` = identity: the same quantity as the reference's camera at pose ``t``),
``"dropin"`` (the torch statements on the HIP rasterizer's autograd surface) and ``"mirror"`` (the same statements on CPU tensors:
the parity target; needs a CPU ``slam.Renderer``).  On the fused engine nothing is read back per iteration: ``densify`` synchronises on
its counts on its own schedule, and the capacity flag is read there, before each evaluation and every ``check_every`` iterations --
iterations the device skipped because a view's lists outgrew their buckets are run again on re-learnt lists (plain iterations at
the rate of the check's iteration, on frames drawn anew), as the frame loop does.

``use_wandb`` and ``report_iter_progress`` are refused.  LPIPS is part of both evaluations with ``config['lpips_weights']`` (``--lpips-weights``).
Not covered: ``scripts/gaussian_splatting.py``, multi-rank runs.
"""
from __future__ import annotations

import argparse
import os
import random
import shutil
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import slam

DROPPED_KEYS = ('intrinsics', 'w2c', 'org_width', 'org_height', 'gt_w2c_all_frames', 'keyframe_time_indices')
EVAL_AT = 7000


def check_supported(config):
    """Stops with the name of a key this driver cannot honour."""
    if config.get('use_wandb'):
        raise SystemExit("config['use_wandb'] = True: wandb logging is not supported; set it to False")
    if config.get('report_iter_progress'):
        raise SystemExit("config['report_iter_progress'] = True: per-iteration progress reports are not supported; set it to False")


def load_finished_map(path, device):
    """``params.npz`` of a finished run as the script reads it: (params, variables without scene_radius)."""
    raw = dict(np.load(path, allow_pickle=True))
    for k in DROPPED_KEYS:
        raw.pop(k)
    params = {k: torch.tensor(v).to(device).float().contiguous() for k, v in raw.items()}
    n = params['means3D'].shape[0]
    variables = {k: torch.zeros(n, device=device) for k in ('max_2D_radius', 'means2D_gradient_accum', 'denom')}
    variables['timestep'] = params.pop('timestep')
    return params, variables


def estimated_w2c(params, t):
    """The world-to-camera matrix the script builds from the loaded pose of frame ``t``."""
    q = F.normalize(params['cam_unnorm_rots'][..., t].detach())
    w2c = torch.eye(4, device=q.device)
    w2c[:3, :3] = slam.build_rotation(q)[0]
    w2c[:3, 3] = params['cam_trans'][..., t].detach().reshape(3)
    return w2c


def _datasets(config, device):
    from . import datasets
    data = config['data']
    data.setdefault('ignore_bad', False)
    data.setdefault('use_train_split', True)
    if "gradslam_data_cfg" not in data:
        data_cfg = {"dataset_name": data["dataset_name"]}
    else:
        data_cfg = datasets.load_dataset_config(data["gradslam_data_cfg"])
    common = dict(config_dict=data_cfg, basedir=data["basedir"], sequence=os.path.basename(data["sequence"]), start=data["start"],
                  end=data["end"], desired_height=data["desired_image_height"], desired_width=data["desired_image_width"],
                  device=device, relative_pose=True, ignore_bad=data["ignore_bad"], use_train_split=data["use_train_split"])
    return datasets.get_dataset(stride=data["stride"], **common), datasets.get_dataset(stride=data["eval_stride"], **common)


def post_splatam_opt(config, engine="fused", dataset=None, eval_dataset=None, num_iters=None, evaluate=True, check_every=500,
                     timed=False, record_losses=False):
    """Runs the refinement ``config`` describes; returns ``(params, variables, stats, path of params.npz)``.

    ``dataset`` / ``eval_dataset``: the mapping and evaluation datasets when the caller has them already (default: built from
    ``config['data']`` with ``stride`` / ``eval_stride``); ``num_iters`` overrides ``config['train']['num_iters_mapping']``;
    ``evaluate=False`` skips both evaluations.  ``stats``: ``views`` (the frame of every iteration), ``rows`` ((iteration, rows
    before, rows after) of every scheduled densification), ``losses`` (mirror / dropin: per iteration; fused: with ``record_losses``,
    copied on the device per iteration and read once at the end, else None), ``redone_iterations`` / ``redone_views`` ((iteration of the check, frame) of every iteration run again: they
    draw from Python's generator too, so the frames after them are no longer the reference's sequence), ``eval_7k`` / ``eval``, ``loop_s``, and on the
    fused engine ``phase_s`` (``timed``) and ``engine`` (the FusedEngine that holds the refined map)."""
    if engine not in ("fused", "dropin", "mirror"):
        raise ValueError(f"engine must be 'fused', 'dropin' or 'mirror' (got {engine!r})")
    check_supported(config)
    train, data = config['train'], config['data']
    device = torch.device("cpu" if engine == "mirror" else config.get("primary_device", "cuda:0"))
    own = dataset is None
    if own:
        dataset, eval_dataset = _datasets(config, device)
    elif eval_dataset is None:
        eval_dataset = dataset
    try:
        num_frames = data["num_frames"]
        num_frames = len(dataset) if num_frames == -1 else num_frames
        eval_num_frames = data.get("eval_num_frames", -1)
        eval_num_frames = len(eval_dataset) if eval_num_frames == -1 else eval_num_frames
        n_iters = int(train['num_iters_mapping'] if num_iters is None else num_iters)
        out_dir = os.path.join(config["workdir"], config["run_name"])

        # ---- the finished map and the first frame (:68-108)
        color0, depth0, map_intrinsics, pose0 = dataset[0]
        depth0 = depth0.permute(2, 0, 1)
        H, W = int(depth0.shape[1]), int(depth0.shape[2])
        intrinsics = map_intrinsics[:3, :3]
        first_w2c = torch.linalg.inv(pose0)
        params, variables = load_finished_map(data['param_ckpt_path'], device)
        variables['scene_radius'] = torch.max(depth0) / 2.0
        scene_radius = float(variables['scene_radius'])

        # ---- every mapping frame and its camera at the estimated pose (:238-262)
        frames = []
        k_host = intrinsics.cpu().numpy()
        eye = torch.eye(4, device=device)
        for t in range(num_frames):
            color, depth, _, _ = dataset[t]
            w2c_t = estimated_w2c(params, t)
            fr = {'im': (color.permute(2, 0, 1) / 255).contiguous(), 'depth': depth.permute(2, 0, 1).contiguous(), 'id': t,
                  'intrinsics': map_intrinsics, 'gt_w2c': w2c_t}
            if engine == "fused":
                fr['w2c'] = eye                     # (the engine transforms to frame t itself: see the module docstring)
            else:
                fr['w2c'] = w2c_t
                fr['cam'] = slam.setup_camera(W, H, k_host, w2c_t.detach().cpu().numpy(), device=device)
            frames.append(fr)

        lrs = dict(train['lrs_mapping'])
        schedule = slam.get_expon_lr_func(lr_init=lrs['means3D'], lr_final=train['lrs_mapping_means3D_final'],
                                          lr_delay_mult=train['lr_delay_mult'], max_steps=train['num_iters_mapping'])
        densifying = bool(train['use_gaussian_splatting_densification'])
        dd = train['densify_dict'] if densifying else None
        weights = train['loss_weights']
        sil_thres = train['sil_thres']
        ms_ssim = min(H, W) > 160
        stats = {'views': [], 'rows': [], 'losses': [] if engine != "fused" else None, 'redone_iterations': 0, 'redone_views': [], 'eval_7k': None, 'eval': None}
        time_idx = num_frames - 1

        def run_eval(params_now, eng, name):
            from . import evaluation
            if not evaluate:
                return None
            if not ms_ssim:
                print("frames with min(H, W) <= 160: MS-SSIM is not computed")
            return evaluation.evaluate(eval_dataset, params_now, eval_num_frames, sil_thres, mapping_iters=train['num_iters_mapping'],
                                       add_new_gaussians=True, engine=eng, eval_dir=os.path.join(out_dir, name), ms_ssim=ms_ssim,
                                       **({'lpips_weights': config['lpips_weights']} if config.get('lpips_weights') is not None else {}))

        t_loop = time.perf_counter()
        if engine == "fused":
            params, variables, eng = _fused_loop(params, variables, frames, (W, H, k_host), device, n_iters, time_idx, schedule, lrs, weights,
                                                 dd, scene_radius, stats, run_eval, check_every, timed, record_losses)
        else:
            for k in params:
                params[k].requires_grad_(True)
            optimizer = slam.initialize_optimizer(params, lrs, tracking=False)
            for it in range(n_iters):
                slam.update_learning_rate(optimizer, schedule, it + 1)
                t = random.randint(0, time_idx)
                stats['views'].append(t)
                loss, variables, _ = slam.get_loss_gs(params, frames[t], variables, weights)
                loss.backward()
                stats['losses'].append(float(loss.detach()))
                with torch.no_grad():
                    if densifying:
                        rows = int(params['means3D'].shape[0])
                        params, variables = slam.densify(params, variables, optimizer, it, dd)
                        if slam.edit_schedule(it, dd, 'densify_every').edits:
                            stats['rows'].append((it, rows, int(params['means3D'].shape[0])))
                    optimizer.step()
                    optimizer.zero_grad(set_to_none=True)
                    if it + 1 == EVAL_AT:
                        stats['eval_7k'] = run_eval({k: v.detach().clone() for k, v in params.items()}, "mirror" if engine == "mirror" else None,
                                                    "eval_7k")
            eng = "mirror" if engine == "mirror" else None
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        stats['loop_s'] = time.perf_counter() - t_loop
        stats['iterations'] = n_iters
        final = {k: v.detach() for k, v in params.items()}
        with torch.no_grad():
            stats['eval'] = run_eval(final, eng, "eval")

        # ---- params.npz as the script writes it (:368-381)
        out = dict(final)
        out['timestep'] = variables['timestep']
        out['intrinsics'] = map_intrinsics.detach().cpu().numpy()
        out['w2c'] = first_w2c.detach().cpu().numpy()
        out['org_width'] = data["desired_image_width"]
        out['org_height'] = data["desired_image_height"]
        out['gt_w2c_all_frames'] = np.stack([fr['gt_w2c'].detach().cpu().numpy() for fr in frames], axis=0)
        from .pipeline import save_params
        path = save_params(out, out_dir)
    finally:
        if own:
            for ds in (dataset, eval_dataset):
                if ds is not None and hasattr(ds, "close"):
                    ds.close()
    return params, variables, stats, path


def _fused_loop(params, variables, frames, cam_args, device, n_iters, time_idx, schedule, lrs, weights, dd, scene_radius, stats, run_eval,
                check_every, timed, record_losses):
    """The iterations on one FusedEngine that owns the map.  Returns (params, variables, engine)."""
    from . import _capi
    from .fused import FusedEngine
    from .pipeline import _PhaseTimer
    W, H, k_host = cam_args
    cam = slam.setup_camera(W, H, k_host, np.eye(4, dtype=np.float32), device=device)
    for fr in frames:
        fr['cam'] = cam
    P = int(params['means3D'].shape[0])
    eng = FusedEngine(params, cam, gaussian_capacity=int(1.5 * P) + 65536, variables=variables)
    eng.keep_map_grads = False                     # (the loop discards its gradients after the step, :320)
    eng.reset_map_optimizer()
    cfg = {'loss': 'gs', 'loss_weights': weights, 'lrs': lrs}
    phase = _PhaseTimer(device, on=timed)
    pending = 0                                    # iterations since the capacity flag was last read
    losses = torch.zeros(n_iters, dtype=torch.float32, device=device) if record_losses else None

    def settle(it):
        """Reads the capacity flag; iterations the device skipped are run again (plain ones, at iteration ``it``'s rate)."""
        nonlocal pending
        pending = 0
        rounds = 0
        while lost := eng.settle("map"):
            stats['redone_iterations'] += lost
            rounds += 1
            if rounds > 3:
                raise RuntimeError(f"iteration {it}: the per-tile lists overflowed three times in a row")
            for _ in range(lost):
                t = random.randint(0, time_idx)
                stats['redone_views'].append((it, t))
                eng.mapping_iteration(frames[t], t, cfg)

    for it in range(n_iters):
        lrs['means3D'] = float(schedule(it + 1))
        t = random.randint(0, time_idx)
        stats['views'].append(t)
        fr = frames[t]
        sched = slam.edit_schedule(it, dd, 'densify_every') if dd is not None else None
        if sched is None or not sched.active:
            # nothing between backward() and step(): one call, the Adam step rides in the last kernel
            with phase("iteration"):
                eng.mapping_iteration(fr, t, cfg)
        else:
            with phase("loss_backward"):
                eng.loss_backward(fr, t, cfg, tracking=False)
            with phase("means2d_accumulate"):
                eng.accumulate_mean2d_gradient()
            if sched.edits:
                settle(it)                         # (densify reads its counts anyway; the selection must not see a flagged iteration's map)
                rows = eng.P
            with phase("densify"):
                edited = eng.densify(it, dd, scene_radius, accumulate=False)
            if sched.edits:
                stats['rows'].append((it, rows, eng.P))
            if edited and not eng.lists_known():
                with phase("relearn_lists"):
                    eng.relearn_lists(fr, t)
            if not sched.edits:                    # re-created parameters carry no gradient: no Adam step
                with phase("adam"):
                    eng.adam_map(lrs)
        if losses is not None:                     # (a device-side copy of the report's slot: nothing is read here)
            losses[it:it + 1].copy_(eng.buf['d_cam'][_capi.SPLAT_REPORT_LOSS:_capi.SPLAT_REPORT_LOSS + 1])
        pending += 1
        if pending >= check_every or it + 1 == EVAL_AT or it + 1 == n_iters:
            settle(it)
        if it + 1 == EVAL_AT:
            stats['eval_7k'] = run_eval({k: v.detach().clone() for k, v in eng.params.items()}, eng, "eval_7k")
    stats['phase_s'] = {k: 1e-3 * ms for k, ms in phase.frame.items()}
    stats['engine'] = eng
    if losses is not None:
        stats['losses'] = losses.cpu().tolist()
    return eng.params, eng.variables, eng


def main(argv=None):
    from .run import load_experiment, seed_everything
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.post_opt", description=__doc__.split("\n\n")[0])
    parser.add_argument("experiment", help="path to a post_splatam_opt experiment file (a Python file that defines `config`)")
    parser.add_argument("--engine", default="fused", choices=("fused", "dropin", "mirror"))
    parser.add_argument("--num-iters", type=int, default=None, help="overrides config['train']['num_iters_mapping']")
    parser.add_argument("--no-eval", action="store_true", help="skip the evaluations (at 7000 iterations and of the final map)")
    parser.add_argument("--lpips-weights", default=None, metavar="PATH",
                        help="AlexNet + LPIPS linear-layer weights (canonical .npz or a torch state dict): the evaluations also report LPIPS")
    args = parser.parse_args(argv)
    config = load_experiment(args.experiment)
    check_supported(config)
    if args.lpips_weights is not None:
        config = dict(config, lpips_weights=args.lpips_weights)        # (a copy: the experiment module's dict stays as written)
    seed_everything(config['seed'])
    print(f"Seed set to: {config['seed']}")
    results_dir = os.path.join(config["workdir"], config["run_name"])
    os.makedirs(results_dir, exist_ok=True)
    shutil.copy(args.experiment, os.path.join(results_dir, "config.py"))
    params, _, stats, path = post_splatam_opt(config, engine=args.engine, num_iters=args.num_iters, evaluate=not args.no_eval)
    for name in ('eval_7k', 'eval'):
        ev = stats[name]
        if ev is not None:
            print(f"[{name}] Average PSNR: {ev['avg_psnr']:.2f}  Depth RMSE: {100 * ev['avg_depth_rmse']:.2f} cm  "
                  f"Depth L1: {100 * ev['avg_depth_l1']:.2f} cm  MS-SSIM: {ev['avg_ms_ssim']:.3f}")
            if ev.get('lpips') is not None:
                print(f"[{name}] Average LPIPS: {ev['avg_lpips']:.3f}")
    print(f"{stats['iterations']} iterations, {params['means3D'].shape[0]} Gaussians: "
          f"{stats['iterations'] / max(stats['loop_s'], 1e-9):.1f} iterations/s in the loop")
    print(f"saved {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
