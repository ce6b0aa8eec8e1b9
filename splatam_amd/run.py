"""``python -m splatam_amd.run CONFIG.py``: runs a SplaTAM experiment file over a sequence on disk.

The file is one of the reference's own (configs/<dataset>/*.py: a Python module whose ``config`` dict the reference's
``scripts/splatam.py`` loads with ``SourceFileLoader``, :992-1001); this package ships none of them.  What happens here is what that
script does around its frame loop, restated: the defaults of :458-464 and :494-517, the seeding of utils/common_utils.py:8-22, the
datasets (``datasets.get_dataset`` at the full size, ``at_size`` siblings where tracking or densification have a size of their own),
``pipeline.rgbd_slam`` (with the reference's checkpoint keys: saving every ``checkpoint_interval`` frames, ``load_checkpoint``), the
evaluation as the run's last act, and ``params.npz`` under ``workdir/run_name`` with the reference's extra
entries (:973-986).  Keys the loop cannot honour stop the run with a message that names them.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time
from importlib.machinery import SourceFileLoader

import numpy as np
import torch

EXTRA_PARAMS = ("timestep", "intrinsics", "w2c", "org_width", "org_height", "gt_w2c_all_frames", "keyframe_time_indices")


def load_experiment(path):
    """The ``config`` dict of an experiment file."""
    import importlib.util
    loader = SourceFileLoader(os.path.basename(path), path)
    spec = importlib.util.spec_from_loader(loader.name, loader)
    module = importlib.util.module_from_spec(spec)
    loader.exec_module(module)
    if not isinstance(getattr(module, "config", None), dict):
        raise ValueError(f"{path} defines no `config` dict")
    return module.config


def seed_everything(seed=42):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False


def apply_defaults(config):
    """The entries the reference fills in before its loop; returns (separate densification size?, separate tracking size?)."""
    tracking = config['tracking']
    if "use_depth_loss_thres" not in tracking:
        tracking['use_depth_loss_thres'] = False
        tracking['depth_loss_thres'] = 100000
    tracking.setdefault('visualize_tracking_loss', False)
    config.setdefault('gaussian_distribution', "isotropic")
    data = config['data']
    data.setdefault('ignore_bad', False)
    data.setdefault('use_train_split', True)
    separate = {}
    for which in ("densification", "tracking"):
        if f"{which}_image_height" not in data:
            data[f"{which}_image_height"] = data["desired_image_height"]
            data[f"{which}_image_width"] = data["desired_image_width"]
        separate[which] = (data[f"{which}_image_height"], data[f"{which}_image_width"]) != \
            (data["desired_image_height"], data["desired_image_width"])
    return separate["densification"], separate["tracking"]


def check_supported(config):
    """Stops with the name of a key this loop cannot honour."""
    if config.get('use_wandb'):
        raise SystemExit("config['use_wandb'] = True: wandb logging is not supported; set it to False")
    if config.get('load_checkpoint') and 'checkpoint_time_idx' not in config:
        raise SystemExit("config['load_checkpoint'] = True needs config['checkpoint_time_idx']: the frame whose checkpoint is loaded")
    if config.get('save_checkpoints') and 'checkpoint_interval' not in config:
        raise SystemExit("config['save_checkpoints'] = True needs config['checkpoint_interval']")
    if config['tracking'].get('visualize_tracking_loss'):
        raise SystemExit("config['tracking']['visualize_tracking_loss']: the tracking-loss viewer is not supported; set it to False")
    if config.get('mean_sq_dist_method') != "projective":
        raise SystemExit(f"config['mean_sq_dist_method'] = {config.get('mean_sq_dist_method')!r}: only \"projective\" is supported")


def run(config, engine="fused", num_frames=None, evaluate=True, prefetch=4, resume_exact=None, exact_checkpoints=False, mesh=False, gt_mesh=None,
        gt_transform=None, cull=False, align=False):
    """Runs ``config`` (an experiment file's dict); returns ``(params, variables, stats, path of params.npz)``.  The reference's four
    checkpoint keys (``save_checkpoints``, ``checkpoint_interval``, ``load_checkpoint``, ``checkpoint_time_idx``) are honoured under
    ``workdir/run_name``; ``exact_checkpoints=True`` makes every checkpoint ``save_checkpoints`` writes an exact one (``session<t>.npz``
    beside the pair) and ``resume_exact=t`` continues from the exact checkpoint of frame ``t`` there (``pipeline.rgbd_slam``).
    ``mesh=True`` (or a dict of ``mesh.mesh_from_params`` keywords, ``dict(sparse=True)`` for a sparse volume): ``mesh.ply`` next to
    ``params.npz``, from the saved map.
    ``gt_mesh`` (with ``mesh``): the path of a ground-truth PLY; ``stats['mesh_score']`` is ``mesh_score.score_mesh`` of the written mesh
    against it, with ``gt_transform`` (a 4 x 4, or the path of a text file of one) applied to the reconstruction: the first frame's
    ABSOLUTE camera-to-world pose, which the loaders do not keep (Replica: the first line of ``traj.txt``).  ``cull`` (with ``gt_mesh``):
    both meshes are first culled to the frusta of the dataset's poses in the MAP's frame, where those poses live, the inverse of
    ``gt_transform`` bringing the ground truth there (``mesh_score.score_culled_in_map_frame``).  ``align`` (with ``gt_mesh``; True or a
    dict of ``mesh_score.align_icp`` keywords): the reconstruction is registered to the ground truth by ICP before it is measured, and
    ``stats['mesh_score']['alignment']`` records what was found.  ``mesh=dict(method="cubes")``: the mesh is extracted by marching
    cubes instead of marching tetrahedra (``mesh.extract_mesh``).  ``mesh=dict(clean=True)`` (or ``clean=`` a dict of
    ``mesh_clean.clean_mesh`` keywords): the mesh's small connected components are removed before it is written and scored;
    ``stats['mesh_cleaning']`` is the report, and with ``gt_mesh`` it is ``stats['mesh_score']['cleaning']`` too.
    ``mesh=dict(simplify=CELL)`` (or ``simplify=`` a dict of ``mesh_simplify.simplify_mesh`` keywords that names ``cell``): the mesh is
    simplified after the cleaning and before it is written, so with ``gt_mesh`` the simplified mesh is what is scored;
    ``stats['mesh_simplification']`` is the report."""
    from . import datasets, pipeline
    separate_densification, separate_tracking = apply_defaults(config)
    check_supported(config)
    data = config['data']
    device = torch.device(config.get("primary_device", "cuda:0"))
    if "gradslam_data_cfg" not in data:
        data_cfg = {"dataset_name": data["dataset_name"]}
    else:
        data_cfg = datasets.load_dataset_config(data["gradslam_data_cfg"])
    dataset = datasets.get_dataset(
        config_dict=data_cfg, basedir=data["basedir"], sequence=os.path.basename(data["sequence"]), start=data["start"], end=data["end"],
        stride=data["stride"], desired_height=data["desired_image_height"], desired_width=data["desired_image_width"], device=device,
        relative_pose=True, ignore_bad=data["ignore_bad"], use_train_split=data["use_train_split"], prefetch=prefetch)
    try:
        n = data["num_frames"] if num_frames is None else num_frames
        n = len(dataset) if n == -1 else min(int(n), len(dataset))
        densify = dataset.at_size(data["densification_image_height"], data["densification_image_width"]) if separate_densification else None
        tracking = dataset.at_size(data["tracking_image_height"], data["tracking_image_width"]) if separate_tracking else None
        opts = None
        if evaluate:
            ms_ssim = min(data["desired_image_height"], data["desired_image_width"]) > 160
            if not ms_ssim:
                print("frames with min(H, W) <= 160: MS-SSIM is not computed")
            opts = dict(eval_every=config['eval_every'], ms_ssim=ms_ssim)
            if config.get('save_frames'):       # the reference's eval(..., save_frames=True): pictures under <run>/eval
                opts.update(save_frames=True, eval_dir=os.path.join(config["workdir"], config["run_name"], "eval"))
        t0 = time.perf_counter()
        params, variables, stats = pipeline.rgbd_slam(dataset, config, engine=engine, num_frames=n, evaluate=opts,
                                                      tracking_dataset=tracking, densify_dataset=densify,
                                                      checkpoint_dir=os.path.join(config["workdir"], config["run_name"]),
                                                      resume_exact=resume_exact, exact_checkpoints=exact_checkpoints)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        stats['run_s'] = time.perf_counter() - t0
        stats['frames'] = n
        stats['dataset'] = dict(dataset.stats)
        intrinsics, pose0 = dataset.intrinsics, dataset.transformed_poses[0]
        out = {k: v for k, v in params.items()}
        out['timestep'] = variables['timestep']
        out['intrinsics'] = intrinsics[:3, :3].detach().cpu().numpy()
        out['w2c'] = torch.linalg.inv(pose0).detach().cpu().numpy()
        out['org_width'] = data["desired_image_width"]
        out['org_height'] = data["desired_image_height"]
        out['gt_w2c_all_frames'] = np.stack([torch.linalg.inv(dataset.transformed_poses[t]).cpu().numpy() for t in range(n)], axis=0)
        out['keyframe_time_indices'] = np.array(stats['keyframe_time_indices'])
        path = pipeline.save_params(out, os.path.join(config["workdir"], config["run_name"]))
        if mesh:
            from .mesh import mesh_from_params
            stats['mesh'] = os.path.join(os.path.dirname(path), "mesh.ply")
            mesh_options = dict(mesh) if isinstance(mesh, dict) else {}
            cleaning = {} if mesh_options.get("clean") else None
            simplification = {} if mesh_options.get("simplify") else None
            mesh_from_params(path, stats['mesh'], device=device, **mesh_options, **({"cleaning": cleaning} if cleaning is not None else {}),
                             **({"simplification": simplification} if simplification is not None else {}))
            if mesh_options.get("views"):
                stats['mesh_views'] = mesh_options["views"]
            if cleaning is not None:
                stats['mesh_cleaning'] = cleaning
            if simplification is not None:
                stats['mesh_simplification'] = simplification
            if gt_mesh is not None:
                from .mesh_score import load_transform, score_culled_in_map_frame, score_mesh
                transform = load_transform(gt_transform) if isinstance(gt_transform, (str, os.PathLike)) else gt_transform
                if cull:
                    try:
                        stats['mesh_score'] = score_culled_in_map_frame(
                            stats['mesh'], gt_mesh, out['gt_w2c_all_frames'], out['intrinsics'],
                            (data["desired_image_width"], data["desired_image_height"]), gt_transform=transform, device=device,
                            **({"align": align} if align else {}))
                    except ValueError as e:
                        raise SystemExit(f"--cull: {e}") from None
                else:
                    stats['mesh_score'] = score_mesh(stats['mesh'], gt_mesh, transform=transform, device=device, **({"align": align} if align else {}))
                if cleaning is not None:
                    stats['mesh_score']['cleaning'] = cleaning
    finally:
        dataset.close()
    return params, variables, stats, path


def _parser():
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.run", description=__doc__.split("\n\n")[0])
    parser.add_argument("experiment", help="path to a SplaTAM experiment file (a Python file that defines `config`)")
    parser.add_argument("--engine", default="fused", choices=("fused", "dropin", "plugin", "plugin_map_edits"))
    parser.add_argument("--num-frames", type=int, default=None, help="overrides config['data']['num_frames'] (-1 = all)")
    parser.add_argument("--no-eval", action="store_true", help="skip the evaluation of the final map")
    parser.add_argument("--lpips-weights", default=None, metavar="PATH",
                        help="AlexNet + LPIPS linear-layer weights (canonical .npz or a torch state dict: splatam_amd.lpips): the evaluation "
                             "then also reports LPIPS; sets config['lpips_weights']")
    parser.add_argument("--resume-exact", type=int, default=None, metavar="T",
                        help="continue at frame T + 1 from the exact checkpoint (session<T>.npz) under workdir/run_name")
    parser.add_argument("--exact-checkpoints", action="store_true",
                        help="with config['save_checkpoints']: also write session<t>.npz, the state --resume-exact continues from")
    parser.add_argument("--mesh", action="store_true", help="write mesh.ply next to params.npz (python -m splatam_amd.mesh on the saved map)")
    parser.add_argument("--mesh-sparse", action="store_true",
                        help="with --mesh: fuse into a sparse volume (python -m splatam_amd.mesh --sparse): the same mesh, memory only near surfaces")
    parser.add_argument("--mesh-method", choices=("tetrahedra", "cubes"), default=None,
                        help="with --mesh: the surface extractor (python -m splatam_amd.mesh --method); cubes: about a third of the triangles")
    parser.add_argument("--clean-mesh", action="store_true",
                        help="with --mesh: remove the mesh's small connected components before it is written and scored (splatam_amd.mesh_clean)")
    parser.add_argument("--simplify-mesh", type=float, default=None, metavar="CELL",
                        help="with --mesh: merge the vertices in each cell of a grid of this edge (metres) before the mesh is written and scored "
                             "(splatam_amd.mesh_simplify)")
    parser.add_argument("--mesh-views", default=None, metavar="DIR",
                        help="with --mesh: pictures of the mesh along the estimated trajectory into DIR (python -m splatam_amd.mesh --views)")
    parser.add_argument("--gt-mesh", default=None, metavar="GT.ply",
                        help="with --mesh: score mesh.ply against this ground-truth mesh (python -m splatam_amd.mesh_score)")
    parser.add_argument("--gt-transform", default=None, metavar="FILE",
                        help="text file of the 4 x 4 first-frame camera-to-world pose that takes the map into the ground truth's frame "
                             "(Replica: the first line of traj.txt)")
    parser.add_argument("--cull", action="store_true",
                        help="with --gt-mesh: cull both meshes to the frusta of the dataset's poses before scoring (splatam_amd.mesh_render)")
    parser.add_argument("--align", action="store_true",
                        help="with --gt-mesh: register the mesh to the ground truth by point-to-point ICP before scoring")
    return parser


def main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    if args.align and not args.gt_mesh:
        parser.error("--align needs --gt-mesh")
    if args.gt_mesh and not args.mesh:
        parser.error("--gt-mesh needs --mesh")
    if args.mesh_sparse and not args.mesh:
        parser.error("--mesh-sparse needs --mesh")
    if args.cull and not args.gt_mesh:
        parser.error("--cull needs --gt-mesh")
    if args.clean_mesh and not args.mesh:
        parser.error("--clean-mesh needs --mesh")
    if args.mesh_method and not args.mesh:
        parser.error("--mesh-method needs --mesh")
    if args.mesh_views and not args.mesh:
        parser.error("--mesh-views needs --mesh")
    if args.simplify_mesh is not None and not args.mesh:
        parser.error("--simplify-mesh needs --mesh")
    mesh = args.mesh
    if args.mesh_sparse or args.clean_mesh or args.mesh_method or args.mesh_views or args.simplify_mesh is not None:
        mesh = dict(**({"sparse": True} if args.mesh_sparse else {}), **({"clean": True} if args.clean_mesh else {}),
                    **({"simplify": args.simplify_mesh} if args.simplify_mesh is not None else {}),
                    **({"method": args.mesh_method} if args.mesh_method else {}), **({"views": args.mesh_views} if args.mesh_views else {}))
    config = load_experiment(args.experiment)
    seed_everything(config['seed'])
    print(f"Seed set to: {config['seed']}")
    if args.lpips_weights is not None:
        config = dict(config, lpips_weights=args.lpips_weights)        # (a copy: the experiment module's dict stays as written)
    _, _, stats, path = run(config, engine=args.engine, num_frames=args.num_frames, evaluate=not args.no_eval, resume_exact=args.resume_exact,
                            exact_checkpoints=args.exact_checkpoints, mesh=mesh, gt_mesh=args.gt_mesh, gt_transform=args.gt_transform,
                            cull=args.cull, **({"align": True} if args.align else {}))
    ev = stats.get('eval')
    if ev is not None:
        print(f"Average PSNR: {ev['avg_psnr']:.2f}\nAverage Depth RMSE: {100 * ev['avg_depth_rmse']:.2f} cm\n"
              f"Average Depth L1: {100 * ev['avg_depth_l1']:.2f} cm\nAverage MS-SSIM: {ev['avg_ms_ssim']:.3f}")
        if ev.get('lpips') is not None:          # (right after MS-SSIM, three decimals, as the reference prints it)
            print(f"Average LPIPS: {ev['avg_lpips']:.3f}")
        print(f"Final Average ATE RMSE: {100 * ev['ate_rmse']:.2f} cm")
    if stats.get('mesh_score') is not None:
        from .mesh_score import format_score
        print(format_score(stats['mesh_score']))
    loop_s = sum(stats['frame_s'])
    print(f"{stats['frames']} frames, {stats['num_gaussians'][-1]} Gaussians, keyframes {stats['keyframe_time_indices']}: "
          f"{stats['frames'] / loop_s:.2f} frames/s in the loop")
    print(f"saved {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
