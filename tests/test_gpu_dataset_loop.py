"""A sequence on disk through the loaders, the ingest kernel, the fused frame loop and the command line (splatam_amd/datasets.py,
splatam_amd/run.py): six frames of the 160 x 112 synthetic sequence of tests/test_gpu_pipeline.py (same constructor arguments),
quantised as a dataset stores them (8-bit colour, depth round(z * 6553.5) as 16-bit PNG) and written in ReplicaV2 layout -- PNG is
lossless, so the items must EQUAL the in-memory quantised frames.

The reference's loaders cannot be executed here (cv2, imageio and natsort are absent): the expected items are restated (colour bytes as
float32, depth float32(float64(raw) / scale), poses inv(p0) @ p_i).  The loop from disk must reproduce the integer facts of
tests/test_gpu_pipeline.py's run -- keyframes [0, 1, 3], 4 x 12 tracking and 5 x 24 mapping iterations, which is that test's run over
FIVE frames (frame 0 is not tracked) -- and stay within that test's sanity bound of 0.02 m against the written trajectory."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_files as files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, F, SCALE = 160, 112, 140.0, 6553.5
FRAMES, LOOP_FRAMES = 6, 5


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    """(root, quantised frames [(rgb uint8, raw uint16)], poses [6, 4, 4] float32, path of the data YAML)."""
    from splatam_amd import pipeline
    root = str(tmp_path_factory.mktemp("sequence"))
    ds = pipeline.SyntheticRGBDSequence(6000, W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, num_frames=FRAMES, seed=2, step_m=0.012, step_deg=0.4)
    frames, poses = [], []
    for t in range(FRAMES):
        color, depth, _, pose = ds[t]
        rgb = np.rint(color.cpu().numpy()).clip(0, 255).astype(np.uint8)
        raw = np.rint(depth.cpu().numpy()[..., 0].astype(np.float64) * SCALE)
        assert raw.max() <= 65535
        frames.append((rgb, raw.astype(np.uint16)))
        poses.append(pose.cpu().numpy())
    poses = np.stack(poses)
    files.write_replica_v2(root, "room0", frames, poses)
    yaml_path = os.path.join(root, "synthetic.yaml")
    with open(yaml_path, "w") as f:
        f.write(f"dataset_name: 'replicav2'\ncamera_params:\n  image_height: {H}\n  image_width: {W}\n  fx: {F}\n  fy: {F}\n"
                f"  cx: {W / 2 - 0.5}\n  cy: {H / 2 - 0.5}\n  png_depth_scale: {SCALE}\n")
    return root, frames, poses, yaml_path


def open_dataset(on_disk, **kw):
    from splatam_amd import datasets
    root, _, _, yaml_path = on_disk
    kw = dict(dict(desired_height=H, desired_width=W, device="cuda", use_train_split=True, ignore_bad=False), **kw)
    return datasets.get_dataset(datasets.load_dataset_config(yaml_path), root, "room0", **kw)


def test_items_on_the_device_equal_the_quantised_frames(on_disk):
    from splatam_amd import fused
    _, frames, poses, _ = on_disk
    ds = open_dataset(on_disk)
    small = ds.at_size(56, 80)
    try:
        assert len(ds) == FRAMES
        k = torch.tensor([[F, 0, W / 2 - 0.5, 0], [0, F, H / 2 - 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        for t in (0, 1, 2, 5, 3):
            color, depth, intrinsics, pose = ds[t]
            rgb, raw = frames[t]
            assert color.device.type == depth.device.type == intrinsics.device.type == pose.device.type == "cuda"
            assert torch.equal(color.cpu(), torch.from_numpy(rgb.astype(np.float32)))
            assert torch.equal(depth.cpu()[..., 0], torch.from_numpy((raw.astype(np.float64) / SCALE).astype(np.float32)))
            assert torch.equal(intrinsics.cpu(), k)
            want = np.linalg.inv(poses[0].astype(np.float64)) @ poses[t].astype(np.float64)
            assert np.abs(pose.cpu().numpy() - want).max() <= 1e-6
            sc, sd, sk, _ = small[t]
            wc, wd = fused.ingest_frame(torch.from_numpy(rgb).cuda(), torch.from_numpy(raw).cuda(), SCALE, size=(56, 80))
            assert torch.equal(sc, wc) and torch.equal(sd, wd) and tuple(sc.shape) == (56, 80, 3)
            assert torch.equal(sk.cpu()[:2, :3], k[:2, :3] * 0.5)
        assert ds.stats['fetches'] == 5 and ds.stats['items'] == 10                     # two sizes of a frame: one decode, one upload
        assert torch.equal(ds[0][3].cpu(), torch.eye(4))
    finally:
        ds.close()


@pytest.fixture(scope="module")
def disk_run(on_disk):
    from splatam_amd import pipeline
    ds = open_dataset(on_disk)
    try:
        cfg = pipeline.replica_config(tracking_iters=12, mapping_iters=24, keyframe_every=2)
        torch.manual_seed(0)
        np.random.seed(0)
        params, _, stats = pipeline.rgbd_slam(ds, cfg, engine="fused", num_frames=LOOP_FRAMES)
        torch.cuda.synchronize()
    finally:
        ds.close()
    return params, stats


def test_fused_loop_from_disk(on_disk, disk_run):
    from splatam_amd import pipeline
    _, _, poses, _ = on_disk
    params, stats = disk_run
    assert stats['keyframe_time_indices'] == [0, 1, 3]
    assert stats['tracking_iters'] == 4 * 12 and stats['mapping_iters'] == 5 * 24
    p0 = np.linalg.inv(poses[0].astype(np.float64))
    for t in range(LOOP_FRAMES):
        gt = np.linalg.inv(p0 @ poses[t].astype(np.float64))                           # the written trajectory, world-to-camera
        est = pipeline._est_w2c(params, t).cpu().numpy().astype(np.float64)
        err = float(np.linalg.norm(est[:3, 3] - gt[:3, 3]))
        print(f"frame {t}: translation error {err:.5f} m")
        assert err < 0.02, (t, est[:3, 3], gt[:3, 3])


def test_command_line_runs_a_config_file(on_disk, disk_run, tmp_path):
    from splatam_amd import pipeline, run
    root, _, poses, yaml_path = on_disk
    cfg = pipeline.replica_config(tracking_iters=12, mapping_iters=24, keyframe_every=2)
    cfg.update(workdir=str(tmp_path / "experiments"), run_name="room0_0", seed=0, primary_device="cuda:0", eval_every=2,
               report_global_progress_every=500, report_iter_progress=False, load_checkpoint=False, save_checkpoints=False,
               use_wandb=False,
               data=dict(basedir=root, gradslam_data_cfg=yaml_path, sequence="room0", desired_image_height=H, desired_image_width=W,
                         start=0, end=-1, stride=1, num_frames=LOOP_FRAMES))
    path = str(tmp_path / "experiment.py")
    with open(path, "w") as f:
        f.write("# written by tests/test_gpu_dataset_loop.py\nconfig = " + repr(cfg) + "\n")
    done = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "-m", "splatam_amd.run", path], cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    print(done.stdout)
    assert done.returncode == 0
    assert "Average PSNR" in done.stdout and "frames/s" in done.stdout
    saved = np.load(os.path.join(cfg['workdir'], "room0_0", "params.npz"))
    map_keys = {'means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales', 'cam_unnorm_rots', 'cam_trans'}
    assert set(saved.files) == map_keys | set(run.EXTRA_PARAMS)
    assert set(run.EXTRA_PARAMS) == {'timestep', 'intrinsics', 'w2c', 'org_width', 'org_height', 'gt_w2c_all_frames', 'keyframe_time_indices'}
    assert saved['keyframe_time_indices'].tolist() == disk_run[1]['keyframe_time_indices'] == [0, 1, 3]
    assert saved['gt_w2c_all_frames'].shape == (LOOP_FRAMES, 4, 4) and saved['intrinsics'].shape == (3, 3) and saved['w2c'].shape == (4, 4)
    assert int(saved['org_width']) == W and int(saved['org_height']) == H
    assert saved['cam_trans'].shape == (1, 3, LOOP_FRAMES) and saved['timestep'].shape[0] == saved['means3D'].shape[0]
    p0 = np.linalg.inv(poses[0].astype(np.float64))
    assert np.abs(saved['gt_w2c_all_frames'][3] - np.linalg.inv(p0 @ poses[3].astype(np.float64))).max() <= 1e-5
    # a key the loop cannot honour stops the run with its name, before anything is loaded
    cfg['use_wandb'] = True
    with open(path, "w") as f:
        f.write("config = " + repr(cfg) + "\n")
    with pytest.raises(SystemExit, match="use_wandb"):
        run.main([path, "--no-eval"])
