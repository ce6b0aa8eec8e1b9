"""``datasets.NeRFCaptureDataset`` on a capture the test writes itself (tests/nerfcapture_files.py): twelve frames ``0.png ... 11.png``
(lexicographic order would be 0, 1, 10, 11, 2, ...), depth at a size of its own, listed in transforms.json in a shuffled order.  Checked:
the order, the poses (``P @ c2w @ P.T``, relative to the first frame), the intrinsics at a desired size, the item contract, ``at_size``,
the message for an image without an entry, and ``splatam_amd.run.run`` on an iPhone-shaped experiment dict for a few tiny frames on the
CPU.  The expected values are restated (datasets/gradslam_datasets/nerfcapture.py cannot be executed here: no natsort, no cv2)."""
import os

import numpy as np
import pytest
import torch

import dataset_files
import frame_ref
import nerfcapture_files

N, CW, CH, ZW, ZH = 12, 48, 36, 16, 12                 # (the phone: 1920 x 1440 colour over 256 x 192 depth, both 4:3)
FL, CX, CY = 40.0, 23.5, 17.5
SCALE = 6553.5
P = np.diag([1.0, -1.0, -1.0, 1.0])


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("captures"))
    frames = dataset_files.seeded_frames(N, CW, CH, ZW, ZH, seed=5)
    poses_gl = dataset_files.seeded_poses(N, seed=5)
    nerfcapture_files.write_nerfcapture(root, "scan", frames, poses_gl, FL, FL * 1.01, CX, CY)
    return root, frames, poses_gl


def open_capture(root, **kw):
    from splatam_amd import datasets
    return datasets.get_dataset({"dataset_name": "nerfcapture"}, root, "scan", device="cpu", **kw)


def test_supported_and_defaults(capture):
    from splatam_amd import datasets
    assert "nerfcapture" in datasets.SUPPORTED
    ds = datasets.NeRFCaptureDataset(basedir=capture[0], sequence="scan", device="cpu")
    assert (ds.desired_height, ds.desired_width) == (1440, 1920) and ds.png_depth_scale == SCALE and len(ds) == N
    ds.close()


def test_order_poses_intrinsics_and_items(capture):
    root, frames, poses_gl = capture
    ds = open_capture(root, desired_height=18, desired_width=24, prefetch=0)
    try:
        assert [os.path.basename(p) for p in ds.color_paths] == [f"{t}.png" for t in range(N)]          # natural, not lexicographic
        assert [os.path.relpath(p, os.path.join(root, "scan")) for p in ds.depth_paths] == [f"depth/{t}.png" for t in range(N)]
        want = np.stack([P @ poses_gl[t].astype(np.float32).astype(np.float64) @ P.T for t in range(N)]).astype(np.float32).astype(np.float64)
        rel = np.linalg.inv(want[0])[None] @ want
        assert np.abs(ds.poses.numpy() - rel).max() < 1e-6 and torch.equal(ds.poses[0], torch.eye(4))
        k = np.eye(4, dtype=np.float32)
        k[0, 0], k[1, 1], k[0, 2], k[1, 2] = FL, FL * 1.01, CX, CY
        assert np.array_equal(ds.intrinsics.numpy(), frame_ref.scale_intrinsics(k, 18 / CH, 24 / CW))
        for t in (0, 2, 10, 11):
            color, depth, intr, pose = ds[t]
            rgb, raw = frames[t]
            assert tuple(color.shape) == (18, 24, 3) and tuple(depth.shape) == (18, 24, 1) and color.dtype == depth.dtype == torch.float32
            assert np.abs(color.numpy() - frame_ref.resize_linear(rgb, 18, 24)).max() <= 255e-6
            assert np.array_equal(depth.numpy()[..., 0], (frame_ref.resize_nearest(raw, 18, 24).astype(np.float64) / SCALE).astype(np.float32))
            assert intr is ds.intrinsics and torch.equal(pose, ds.poses[t])
    finally:
        ds.close()


def test_at_size_resamples_the_original_frame(capture):
    root, frames, _ = capture
    ds = open_capture(root, desired_height=CH, desired_width=CW, prefetch=0)
    try:
        small = ds.at_size(9, 12)
        color, depth, _, _ = ds[3]
        assert np.array_equal(color.numpy(), frames[3][0].astype(np.float32))                          # identity: the bytes
        assert tuple(depth.shape) == (CH, CW, 1)                                                        # depth upsampled to the colour size
        scolor, sdepth, sk, _ = small[3]
        assert np.abs(scolor.numpy() - frame_ref.resize_linear(frames[3][0], 9, 12)).max() <= 255e-6
        assert np.array_equal(sdepth.numpy()[..., 0], (frame_ref.resize_nearest(frames[3][1], 9, 12).astype(np.float64) / SCALE).astype(np.float32))
        assert float(sk[0, 0]) == pytest.approx(FL * 12 / CW) and ds.stats['fetches'] == 1
    finally:
        ds.close()


def test_an_image_without_an_entry_is_named(tmp_path):
    frames = dataset_files.seeded_frames(3, 8, 6, 4, 3, seed=1)
    nerfcapture_files.write_nerfcapture(str(tmp_path), "scan", frames, dataset_files.seeded_poses(3), FL, FL, 3.5, 2.5, listed=(0, 2))
    with pytest.raises(ValueError, match=r"rgb/1\.png"):
        open_capture(str(tmp_path))


def test_run_accepts_an_iphone_experiment(capture, tmp_path):
    """``python -m splatam_amd.run configs/iphone/splatam.py`` in small: no ``gradslam_data_cfg``, ``dataset_name="nerfcapture"``, a
    densification size of its own; three frames on the CPU (the C oracle behind the drop-in loop's ``Renderer``)."""
    from oracle import c_ref
    from splatam_amd import pipeline, run, slam
    cfg = pipeline.replica_config(tracking_iters=2, mapping_iters=2, keyframe_every=2, mapping_window_size=4)
    cfg.update(workdir=str(tmp_path), run_name="SplaTAM_iPhone", use_wandb=False, load_checkpoint=False, eval_every=1, primary_device="cpu",
               num_frames=3, depth_scale=10.0,
               data=dict(dataset_name="nerfcapture", basedir=capture[0], sequence="scan", desired_image_height=CH // 2,
                         desired_image_width=CW // 2, densification_image_height=CH // 4, densification_image_width=CW // 4,
                         start=0, end=-1, stride=1, num_frames=3))
    saved, slam.Renderer = slam.Renderer, c_ref.CRasterizer
    try:
        run.seed_everything(cfg['seed'])
        params, variables, stats, path = run.run(cfg, engine="dropin", evaluate=False, prefetch=0)
    finally:
        slam.Renderer = saved
    assert stats['frames'] == 3 and stats['keyframe_time_indices'] == [0, 1] and len(stats['decisions']) == 3
    assert params['cam_trans'].shape == (1, 3, 3) and params['means3D'].shape[0] == stats['num_gaussians'][-1] > 0
    # the first frame's point cloud came from the densification frame: at most one Gaussian per pixel of 9 x 12
    assert stats['num_gaussians'][0] <= (CH // 4) * (CW // 4)
    saved_params = np.load(path)
    assert saved_params['org_height'] == CH // 2 and saved_params['gt_w2c_all_frames'].shape == (3, 4, 4)
