"""Generates tests/golden/loop_resume_reference.npz by EXECUTING THE REFERENCE'S OWN ``rgbd_slam`` (/root/reference/scripts/splatam.py:455-990)
twice per case on the C oracle, with the machinery of tests/golden/make_golden_loop.py (imported, not edited):

  1. straight, with ``save_checkpoints=True, checkpoint_interval=2``: the reference writes ``params<t>.npz`` and
     ``keyframe_time_indices<t>.npy`` under ``workdir/run_name`` (:927-931) -- the arrays of the two files of ``t = 2`` are stored as
     ``<case>/ckpt/params/<key>`` and ``<case>/ckpt/keyframe_time_indices`` (data its program wrote; the tests resume from them);
  2. again, with ``load_checkpoint=True, checkpoint_time_idx=2`` (:604-640): recorded as make_golden_loop.py records a run --
     ``<case>/events``, ``values``, ``selected``, ``final/<key>`` (``keyframe_time_indices`` among them), ``config``.

The cases are ``base`` and ``variant`` of tests/golden/loop_reference.npz: their frames and their configuration (with the
``depth_loss_thres`` that file's generator worked out) are read from it, so the resumed recording belongs to the straight one the loop
tests already hold.  In ``base`` frame 2 is not a keyframe; in ``variant`` (``keyframe_every=3``) it is, so the reference's restart AT
frame 2 stores it a second time: ``keyframe_time_indices`` ends as [0, 2, 2, 4, 5].

Run:  python tests/golden/make_golden_resume.py [log file]      (needs /root/reference; not needed on the GPU box)
"""
import copy
import json
import os
import shutil
import sys
import tempfile
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_loop as M                                    # noqa: E402  (puts the repository and tests/ on sys.path)

CASES = ("base", "variant")
CHECKPOINT_TIME_IDX, CHECKPOINT_INTERVAL = 2, 2


def run(S, dataset, cfg):
    """One execution of the reference's ``rgbd_slam`` under the recorder, as ``make_golden_loop.run_case`` does it."""
    from loop_trace import LoopRecorder
    final = {}
    rec = LoopRecorder().wrap(S)
    saved = {k: getattr(S, k) for k in ("get_dataset", "report_progress", "eval", "save_params", "tqdm")}
    S.get_dataset = lambda **kw: dataset
    S.report_progress = lambda *a, **k: None
    S.eval = lambda *a, **k: None
    S.save_params = lambda params, output_dir: final.update(params)
    S.tqdm = lambda it=None, *a, **k: mock.MagicMock() if it is None else M._Quiet(it)
    try:
        with open(os.devnull, "w") as null:                     # (save_params_ckpt and the checkpoint loader print)
            out, sys.stdout = sys.stdout, null
            try:
                S.seed_everything(seed=cfg['seed'])             # scripts/splatam.py:1004
                S.rgbd_slam(copy.deepcopy(cfg))
            finally:
                sys.stdout = out
    finally:
        for k, v in saved.items():
            setattr(S, k, v)
        rec.restore()
    return rec, final


def main():
    from loop_trace import KIND_NAMES, RecordedRGBDSequence, load_config
    log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(M.REPO, "profiles", "reference_resume_loop.log")
    gold = np.load(os.path.join(HERE, "loop_reference.npz"))
    M.install_device_shim()
    S = M.load_reference_module(M.oracle_renderer_module())
    workdir = tempfile.mkdtemp(prefix="splatam_golden_resume")
    out, t = {}, CHECKPOINT_TIME_IDX
    try:
        with open(log_path, "w") as log:
            print(f"reference module: {S.__file__}; rgbd_slam at line {S.rgbd_slam.__code__.co_firstlineno}; Renderer = "
                  f"{S.Renderer.__module__}.{S.Renderer.__name__} (C oracle); torch {torch.__version__}", file=log)
            for name in CASES:
                dataset = RecordedRGBDSequence(gold, name)
                config = load_config(gold, name)
                config.update(workdir=workdir, save_checkpoints=True, checkpoint_interval=CHECKPOINT_INTERVAL, load_checkpoint=False)
                _, straight = run(S, dataset, config)
                run_dir = os.path.join(workdir, config['run_name'])
                print(f"[{name}] straight run wrote {sorted(os.listdir(run_dir))}; keyframes {np.asarray(straight['keyframe_time_indices']).tolist()}", file=log)
                with np.load(os.path.join(run_dir, f"params{t}.npz")) as z:
                    for k in z.files:
                        out[f"{name}/ckpt/params/{k}"] = z[k]
                        print(f"[{name}]   params{t}.npz: {k} {z[k].dtype} {z[k].shape}", file=log)
                kf = np.load(os.path.join(run_dir, f"keyframe_time_indices{t}.npy"))
                out[f"{name}/ckpt/keyframe_time_indices"] = kf
                print(f"[{name}]   keyframe_time_indices{t}.npy: {kf.dtype} {kf.tolist()}", file=log)
                config.update(save_checkpoints=False, load_checkpoint=True, checkpoint_time_idx=t)
                rec, final = run(S, dataset, config)
                events, values, selected = rec.arrays()
                stored = dict(config, workdir="unused")
                out[f"{name}/config"] = np.array(json.dumps(stored))
                out[f"{name}/events"], out[f"{name}/values"], out[f"{name}/selected"] = events, values, selected
                for k, v in final.items():
                    out[f"{name}/final/{k}"] = v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
                counts = {KIND_NAMES[k]: int((events[:, 0] == k).sum()) for k in range(len(KIND_NAMES))}
                print(f"[{name}] resumed at {t}: {len(events)} events {counts}; keyframes {np.asarray(final['keyframe_time_indices']).tolist()}; "
                      f"{final['means3D'].shape[0]} Gaussians at the end", file=log)
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    path = os.path.join(HERE, "loop_resume_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays; log", log_path)


if __name__ == "__main__":
    main()
