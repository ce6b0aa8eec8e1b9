"""Generates tests/golden/loop_multires_reference.npz by EXECUTING THE REFERENCE'S OWN FRAME LOOP (``rgbd_slam`` of
/root/reference/scripts/splatam.py:455-990) with tracking and densification at resolutions of their own -- the flow of its
configs/replica/splatam_s.py and configs/iphone/* -- on CPU, on the C oracle, with the machinery of make_golden_loop.py (imported:
the device shim, the stand-in modules, the oracle behind ``diff_gaussian_rasterization``, the configuration loader, the sequence).

What differs from make_golden_loop.py:
  * ``get_dataset`` returns the dataset that matches the ``desired_height`` / ``desired_width`` it is asked for (:519-582): the full
    frames, the tracking frames or the densification frames;
  * the reduced frames are made from the full frames by tests/frame_ref.py, the float64 numpy restatement of what the reference's
    datasets do with cv2.resize (basedataset.py:210-257: colour INTER_LINEAR on 0..255, depth INTER_NEAREST, intrinsics through
    scale_intrinsics) -- the stand-in for those calls; the stand-in ``cv2`` module itself is a mock and OpenCV is not installed, so
    the frames are NOT pinned against OpenCV;
  * the recorder also writes down the frame size of ``curr_data`` at every get_loss / add_new_gaussians call
    (tests/loop_trace_multires.py).

Run:  python tests/golden/make_golden_loop_multires.py [log file]      (needs /root/reference; not needed on the GPU box)
"""
import copy
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_loop as M                                     # noqa: E402  (puts the repository and tests/ on sys.path)

import frame_ref                                                 # noqa: E402
from loop_trace import KIND_NAMES, LOSS, RecordedRGBDSequence    # noqa: E402
from loop_trace_multires import SizeRecorder                     # noqa: E402

BASE = M.CASES['base']
# the base case prunes with a size bound that removes SOME rows (scene radius = max depth / 8.1).  Here the first frame's Gaussians come
# from the half-size densification frame, whose projective radius depth / focal length is twice as large: half the ratio keeps the bound
# where it was relative to them
RATIO = 4.05
CASES = {
    # SplaTAM-S in small (configs/replica/splatam_s.py): full-size tracking and mapping, densification at half size; isotropic, pruning on
    "splatam_s": dict(scene=BASE['scene'], sizes=dict(tracking=None, densification=(32, 48)),
                      config=dict(BASE['config'], run_name="splatam_s", scene_radius_depth_ratio=RATIO)),
    # a phone capture in small (configs/iphone/*): tracking at 3/4 (72 x 48: a partial tile column), densification at 1/2, a keyframe
    # on every 2nd frame
    "phone": dict(scene=BASE['scene'], sizes=dict(tracking=(48, 72), densification=(32, 48)),
                  config=dict(BASE['config'], run_name="phone", keyframe_every=2, scene_radius_depth_ratio=RATIO)),
}


def reduced(frames, size):
    """The frame set a dataset of ``size`` = (height, width) hands over: what tests/frame_ref.py makes of every full frame."""
    H, W = frames['color'].shape[1:3]
    h, w = size
    return dict(color=np.stack([frame_ref.resize_linear(c, h, w) for c in frames['color']]).astype(np.float32),
                depth=np.stack([frame_ref.resize_nearest(d, h, w) for d in frames['depth']]).astype(np.float32),
                intrinsics=frame_ref.scale_intrinsics(frames['intrinsics'], h / H, w / W),
                poses=frames['poses'])


def run_case(S, name, case, out, log):
    full = M.make_sequence(case['scene'])
    sets = {"frames": full}
    data_cfg = dict(case['config']['data'])
    for which, key in (("tracking", "tracking_frames"), ("densification", "densify_frames")):
        size = case['sizes'][which]
        if size is not None:
            sets[key] = reduced(full, size)
            data_cfg[f"{which}_image_height"], data_cfg[f"{which}_image_width"] = size
    by_size = {}
    for key, frames in sets.items():
        # (the cases share a scene: a frame set an earlier case has stored is stored once, by name)
        twin = next((c for c in CASES if f"{c}/{key}/color" in out and all(np.array_equal(out[f"{c}/{key}/{k}"], v) for k, v in frames.items())), None)
        if twin is not None:
            out[f"{name}/{key}/same_as"] = np.array(twin)
        else:
            for k, v in frames.items():
                out[f"{name}/{key}/{k}"] = v
        by_size[tuple(frames['color'].shape[1:3])] = RecordedRGBDSequence({f"{name}/frames/{k}": v for k, v in frames.items()}, name)
    overrides = copy.deepcopy(M.COMMON)
    for k, v in dict(case['config'], data=data_cfg).items():
        if isinstance(v, dict) and isinstance(overrides.get(k), dict):
            overrides[k].update(v)
        else:
            overrides[k] = v
    config = M.reference_config(overrides)
    config['data'].pop('gradslam_data_cfg')
    config['data']['dataset_name'] = "synthetic"

    final = {}
    rec = SizeRecorder().wrap(S)
    saved = {k: getattr(S, k) for k in ("get_dataset", "report_progress", "eval", "save_params", "tqdm")}
    S.get_dataset = lambda **kw: by_size[(kw['desired_height'], kw['desired_width'])]
    S.report_progress = lambda *a, **k: None
    S.eval = lambda *a, **k: None
    S.save_params = lambda params, output_dir: final.update(params)
    S.tqdm = lambda it=None, *a, **k: mock.MagicMock() if it is None else M._Quiet(it)
    try:
        S.seed_everything(seed=config['seed'])
        S.rgbd_slam(copy.deepcopy(config))
    finally:
        for k, v in saved.items():
            setattr(S, k, v)
        rec.restore()
    events, values, selected = rec.arrays()
    out[f"{name}/config"] = np.array(json.dumps(config))
    out[f"{name}/events"], out[f"{name}/values"], out[f"{name}/selected"] = events, values, selected
    out[f"{name}/sizes"] = rec.size_array()
    for k, v in final.items():
        out[f"{name}/final/{k}"] = v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    counts = {KIND_NAMES[k]: int((events[:, 0] == k).sum()) for k in range(len(KIND_NAMES))}
    sizes = sorted({(int(k), int(h), int(w)) for k, h, w in rec.size_array()})
    print(f"[{name}] {len(events)} events {counts}; keyframes {final['keyframe_time_indices'].tolist()}; "
          f"{final['means3D'].shape[0]} Gaussians at the end; (kind, height, width) of the calls: "
          f"{[(KIND_NAMES[k], h, w) for k, h, w in sizes]}", file=log)
    assert int((events[:, 0] == LOSS).sum()) + counts['ADD'] == len(rec.sizes)


def main():
    log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(M.REPO, "profiles", "multires_reference_loop.log")
    M.install_device_shim()
    S = M.load_reference_module(M.oracle_renderer_module())
    out = {}
    with open(log_path, "w") as log:
        print(f"reference module: {S.__file__}; rgbd_slam at line {S.rgbd_slam.__code__.co_firstlineno}; Renderer = "
              f"{S.Renderer.__module__}.{S.Renderer.__name__} (C oracle); torch {torch.__version__}", file=log)
        for name, case in CASES.items():
            run_case(S, name, case, out, log)
    path = os.path.join(HERE, "loop_multires_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays; log", log_path)


if __name__ == "__main__":
    main()
