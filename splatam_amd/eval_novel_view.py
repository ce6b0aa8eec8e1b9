"""``python -m splatam_amd.eval_novel_view CONFIG.py``: scores a finished map on a dataset split.

The file is one of the reference's ``eval_novel_view`` experiment files (configs/scannetpp/eval_novel_view.py,
configs/replica_v2/eval_novel_view.py); this package ships none of them.  What happens here is what the reference's
``scripts/eval_novel_view.py`` does, restated: the dataset of ``config['data']`` is opened with its ``use_train_split`` /
``ignore_bad`` (poses relative to the first training frame), the map is read from ``config['scene_path']`` (the ``params.npz`` a run
of ``python -m splatam_amd.run`` leaves), and
  * with ``use_train_split`` the training frames are scored by ``evaluation.evaluate`` into ``<workdir>/<run_name>/eval_train``,
  * otherwise the held-out frames by ``evaluation.evaluate_novel_views`` into ``<workdir>/<run_name>/eval_nvs``,
with the pictures saved (``save_frames=True``), and the reference's five lines printed; LPIPS is "not computed" unless
``--lpips-weights PATH`` (or ``config['lpips_weights']``) names the AlexNet weights (``splatam_amd.lpips``).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from .run import load_experiment, seed_everything

MAP_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "cam_unnorm_rots", "cam_trans")


def load_scene(path, device):
    """The map of a ``params.npz``: the five Gaussian arrays and the trajectory as float32 tensors on ``device`` (the file's other
    entries -- intrinsics, keyframes, ... -- are not the evaluation's)."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such file (config['scene_path'] names the params.npz of a finished run)")
    with np.load(path, allow_pickle=True) as z:
        missing = [k for k in MAP_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path} holds no {', '.join(missing)}")
        return {k: torch.tensor(z[k]).to(device=device, dtype=torch.float32).contiguous() for k in MAP_KEYS}


def run(config, engine="fused", prefetch=4):
    """Evaluates ``config`` (an eval_novel_view experiment file's dict); returns ``(result dict, eval_dir)``."""
    from . import datasets, evaluation
    if config.get('use_wandb'):
        raise SystemExit("config['use_wandb'] = True: wandb logging is not supported; set it to False")
    data = config['data']
    data.setdefault('ignore_bad', False)
    data.setdefault('use_train_split', True)
    device = torch.device(config.get("primary_device", "cuda:0"))
    if "gradslam_data_cfg" not in data:
        data_cfg = {"dataset_name": data["dataset_name"]}
    else:
        data_cfg = datasets.load_dataset_config(data["gradslam_data_cfg"])
    results_dir = os.path.join(config["workdir"], config["run_name"])
    dataset = datasets.get_dataset(
        config_dict=data_cfg, basedir=data["basedir"], sequence=os.path.basename(data["sequence"]), start=data["start"], end=data["end"],
        stride=data["stride"], desired_height=data["desired_image_height"], desired_width=data["desired_image_width"], device=device,
        relative_pose=True, ignore_bad=data["ignore_bad"], use_train_split=data["use_train_split"], prefetch=prefetch)
    try:
        n = len(dataset) if data["num_frames"] == -1 else int(data["num_frames"])
        params = load_scene(config['scene_path'], device)
        ms_ssim = min(data["desired_image_height"], data["desired_image_width"]) > 160
        if not ms_ssim:
            print("frames with min(H, W) <= 160: MS-SSIM is not computed")
        mapping = config['mapping']
        opts = dict(eval_every=config['eval_every'], engine="mirror" if engine == "mirror" else None, ms_ssim=ms_ssim,
                    save_frames=engine != "mirror")        # (the pictures are formed on the device: the mirror writes the numbers only)
        if config.get('lpips_weights') is not None:
            opts['lpips_weights'] = config['lpips_weights']
        if data['use_train_split']:
            eval_dir = os.path.join(results_dir, "eval_train")
            out = evaluation.evaluate(dataset, params, n, mapping['sil_thres'], mapping['num_iters'], mapping['add_new_gaussians'],
                                      eval_dir=eval_dir, **opts)
        else:
            eval_dir = os.path.join(results_dir, "eval_nvs")
            out = evaluation.evaluate_novel_views(dataset, params, n, mapping['sil_thres'], mapping['num_iters'], mapping['add_new_gaussians'],
                                                  eval_dir=eval_dir, **opts)
    finally:
        dataset.close()
    return out, eval_dir


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.eval_novel_view", description=__doc__.split("\n\n")[0])
    parser.add_argument("experiment", help="path to an eval_novel_view experiment file (a Python file that defines `config`)")
    parser.add_argument("--engine", default="fused", choices=("fused", "mirror"),
                        help="fused: the HIP path (default); mirror: the torch form (slow; saves no pictures)")
    parser.add_argument("--lpips-weights", default=None, metavar="PATH",
                        help="AlexNet + LPIPS linear-layer weights (canonical .npz or a torch state dict): LPIPS is then computed")
    args = parser.parse_args(argv)
    config = load_experiment(args.experiment)
    seed_everything(config['seed'])
    if args.lpips_weights is not None:
        config = dict(config, lpips_weights=args.lpips_weights)        # (a copy: the experiment module's dict stays as written)
    out, eval_dir = run(config, engine=args.engine)
    print(f"Average PSNR: {out['avg_psnr']:.2f}\nAverage Depth RMSE: {100 * out['avg_depth_rmse']:.2f} cm\n"
          f"Average Depth L1: {100 * out['avg_depth_l1']:.2f} cm\nAverage MS-SSIM: {out['avg_ms_ssim']:.3f}\n"
          + (f"Average LPIPS: {out['avg_lpips']:.3f}" if out.get('lpips') is not None else "Average LPIPS: not computed"))
    if 'valid_nvs_frames' in out:
        print(f"{int(out['valid_nvs_frames'].sum())} of {len(out['frames'])} held-out frames are valid novel views (at most 0.1 % holes)")
    print(f"wrote {eval_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
