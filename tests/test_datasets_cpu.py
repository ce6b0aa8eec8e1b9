"""The dataset loaders (splatam_amd/datasets.py) with ``device="cpu"`` over tiny sequences written into tmp_path with PIL.

The reference's loaders (datasets/gradslam_datasets/*.py) cannot be executed here -- cv2, imageio and natsort are absent -- so the
expected values are RESTATED in this file, as tests/frame_ref.py does for the resize rules: the file order (digit runs compare as
integers), the trajectory formats, TUM's nearest-stamp association (0.08 s, thinned to more than 1/32 s apart), ``start:end:stride``
slicing, poses ``inv(p0) @ p_i``, intrinsics scaled by the two size ratios, depth ``float32(float64(raw) / png_depth_scale)`` and
colour by tests/frame_ref.py's float64 bilinear form (within 255 * 1e-6, the project's COLOUR_ATOL on the 0..255 scale: at most 12
float32 roundings at magnitude <= 255; equal to the bytes at equal size)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import dataset_files as files
import frame_ref

from splatam_amd import datasets

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, "golden", "dataconfig")
COLOUR_ATOL = 255 * 1e-6
W, H = 16, 12


def config(name="replica", scale=6553.5, width=W, height=H, **camera):
    cam = dict(image_height=height, image_width=width, fx=14.0, fy=15.0, cx=7.5, cy=5.5, png_depth_scale=scale)
    cam.update(camera)
    return dict(dataset_name=name, camera_params=cam)


@pytest.fixture(scope="module")
def replica(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("replica"))
    frames, poses = files.seeded_frames(12, W, H, seed=1), files.seeded_poses(12, seed=1)
    files.write_replica(root, "room", frames, poses)
    return root, frames, poses


def open_replica(replica, **kw):
    kw = dict(dict(desired_height=H, desired_width=W, device="cpu"), **kw)
    return datasets.get_dataset(config(), replica[0], "room", **kw)


def expected_relative(poses32):
    p = np.asarray(poses32, dtype=np.float64)
    return np.linalg.inv(p[0])[None] @ p


def test_natural_order():
    names = ["frame10.jpg", "frame2.jpg", "frame1.jpg", "frame000003.jpg", "a/rgb_100.png", "a/rgb_99.png"]
    assert datasets.natural_sorted(names) == ["a/rgb_99.png", "a/rgb_100.png", "frame1.jpg", "frame2.jpg", "frame000003.jpg", "frame10.jpg"]


def test_replica_items_poses_and_intrinsics(replica):
    _, frames, poses = replica
    ds = open_replica(replica, prefetch=0)
    assert len(ds) == 12
    want_pose = expected_relative(poses.astype(np.float32))
    k = np.eye(4, dtype=np.float32)
    k[0, 0], k[1, 1], k[0, 2], k[1, 2] = 14.0, 15.0, 7.5, 5.5
    for t in (0, 5, 11):
        color, depth, intrinsics, pose = ds[t]
        rgb, raw = frames[t]
        assert color.dtype == depth.dtype == intrinsics.dtype == pose.dtype == torch.float32
        assert tuple(color.shape) == (H, W, 3) and tuple(depth.shape) == (H, W, 1) and tuple(intrinsics.shape) == (4, 4)
        assert np.array_equal(color.numpy(), rgb.astype(np.float32))
        assert np.array_equal(depth.numpy()[..., 0], (raw.astype(np.float64) / 6553.5).astype(np.float32))
        assert np.array_equal(intrinsics.numpy(), k)
        assert np.abs(pose.numpy() - want_pose[t]).max() <= 1e-6
    assert torch.equal(ds[0][3], torch.eye(4))                      # frame 0: exactly the identity


def test_replica_v2_orders_unpadded_names_and_resizes(tmp_path):
    frames, poses = files.seeded_frames(12, W, H, seed=2), files.seeded_poses(12, seed=2)
    files.write_replica_v2(str(tmp_path), "room", frames, poses)
    h, w = 7, 9
    ds = datasets.get_dataset(config("ReplicaV2"), str(tmp_path), "room", desired_height=h, desired_width=w, device="cpu",
                              use_train_split=True, ignore_bad=False)
    assert [os.path.basename(p) for p in ds.color_paths] == [f"rgb_{t}.png" for t in range(12)]
    assert [os.path.basename(p) for p in ds.depth_paths] == [f"depth_{t}.png" for t in range(12)]
    want_pose = expected_relative(poses.astype(np.float32))
    k = np.eye(4, dtype=np.float32)
    k[0, 0], k[1, 1], k[0, 2], k[1, 2] = 14.0, 15.0, 7.5, 5.5
    for t in (2, 10):
        color, depth, intrinsics, pose = ds[t]
        rgb, raw = frames[t]
        err = np.abs(color.numpy().astype(np.float64) - frame_ref.resize_linear(rgb, h, w)).max()
        print(f"frame {t}: max |colour - float64| {err:.2e}")
        assert err <= COLOUR_ATOL
        assert np.array_equal(depth.numpy()[..., 0], (frame_ref.resize_nearest(raw, h, w).astype(np.float64) / 6553.5).astype(np.float32))
        assert np.array_equal(intrinsics.numpy(), frame_ref.scale_intrinsics(k, h / H, w / W))
        assert np.abs(pose.numpy() - want_pose[t]).max() <= 1e-6
    with pytest.raises(NotImplementedError):
        datasets.get_dataset(config("replicav2"), str(tmp_path), "room", device="cpu", use_train_split=False)


def test_scannet_per_file_poses_and_two_source_sizes(tmp_path):
    cw, ch = 26, 20
    frames, poses = files.seeded_frames(11, cw, ch, W, H, seed=3), files.seeded_poses(11, seed=3)
    files.write_scannet(str(tmp_path), "scene0000_00", frames, poses)
    h, w = 9, 13
    ds = datasets.get_dataset(config("scannet", scale=1000.0, width=cw, height=ch), str(tmp_path), "scene0000_00", desired_height=h,
                              desired_width=w, device="cpu")
    assert [os.path.basename(p) for p in ds.color_paths] == [f"{t}.jpg" for t in range(11)]
    want_pose = expected_relative(poses)                                                # (read as float64, unlike the trajectories)
    for t in (0, 2, 10):
        color, depth, _, pose = ds[t]
        rgb, raw = frames[t]
        assert tuple(color.shape) == (h, w, 3) and tuple(depth.shape) == (h, w, 1)
        assert np.abs(color.numpy().astype(np.float64) - frame_ref.resize_linear(rgb, h, w)).max() <= COLOUR_ATOL
        assert np.array_equal(depth.numpy()[..., 0], (frame_ref.resize_nearest(raw, h, w).astype(np.float64) / 1000.0).astype(np.float32))
        assert np.abs(pose.numpy() - want_pose[t]).max() <= 1e-6
    assert torch.equal(ds[0][3], torch.eye(4))


def write_tum(root, pose_name="groundtruth.txt"):
    """Colour stamps 1.00 (kept), 1.02 (associated, but within 1/32 s of the last kept one), 1.12 (no depth within 0.08 s),
    1.20 (no pose within 0.08 s), 1.30 and 1.40 (kept)."""
    rgb_stamps = ("1.00", "1.02", "1.12", "1.20", "1.30", "1.40")
    depth_stamps = ("1.01", "1.03", "1.21", "1.30", "1.41")
    pose_stamps = (1.00, 1.02, 1.10, 1.31, 1.40)
    colours = files.seeded_frames(len(rgb_stamps), W, H, seed=4)
    depths = files.seeded_frames(len(depth_stamps), W, H, seed=5)
    os.makedirs(os.path.join(root, "rgb"))
    os.makedirs(os.path.join(root, "depth"))
    with open(os.path.join(root, "rgb.txt"), "w") as f:
        f.write("# color images\n# file: 'test.bag'\n# timestamp filename\n")
        for s, (rgb, _) in zip(rgb_stamps, colours):
            Image.fromarray(rgb).save(os.path.join(root, "rgb", s + ".png"))
            f.write(f"{s} rgb/{s}.png\n")
    with open(os.path.join(root, "depth.txt"), "w") as f:
        f.write("# depth maps\n# file: 'test.bag'\n# timestamp filename\n")
        for s, (_, raw) in zip(depth_stamps, depths):
            Image.fromarray(raw).save(os.path.join(root, "depth", s + ".png"))
            f.write(f"{s} depth/{s}.png\n")
    from scipy.spatial.transform import Rotation
    poses = files.seeded_poses(len(pose_stamps), seed=6)
    with open(os.path.join(root, pose_name), "w") as f:
        f.write("# ground truth trajectory\n# file: 'test.bag'\n# timestamp tx ty tz qx qy qz qw\n")
        for s, p in zip(pose_stamps, poses):
            q = Rotation.from_matrix(p[:3, :3]).as_quat()
            f.write(f"{s:.4f} " + " ".join(f"{x:.9f}" for x in list(p[:3, 3]) + list(q)) + "\n")
    return colours, depths, poses


@pytest.mark.parametrize("pose_name", ("groundtruth.txt", "pose.txt"))
def test_tum_association(tmp_path, pose_name):
    root = os.path.join(str(tmp_path), "rgbd_dataset_freiburg1_desk")
    os.makedirs(root)
    colours, depths, poses = write_tum(root, pose_name)
    ds = datasets.get_dataset(config("tum", scale=5000.0), str(tmp_path), "rgbd_dataset_freiburg1_desk", desired_height=H,
                              desired_width=W, device="cpu")
    assert [os.path.basename(p) for p in ds.color_paths] == ["1.00.png", "1.30.png", "1.40.png"]
    assert [os.path.basename(p) for p in ds.depth_paths] == ["1.01.png", "1.30.png", "1.41.png"]
    want_pose = expected_relative(poses[[0, 3, 4]].astype(np.float32))
    for i, (ci, di) in enumerate(((0, 0), (4, 3), (5, 4))):
        color, depth, _, pose = ds[i]
        assert np.array_equal(color.numpy(), colours[ci][0].astype(np.float32))
        assert np.array_equal(depth.numpy()[..., 0], (depths[di][1].astype(np.float64) / 5000.0).astype(np.float32))
        assert np.abs(pose.numpy() - want_pose[i]).max() <= 1e-6             # (the file holds 9 decimals)
    assert datasets.tum_associate([1.00, 1.02, 1.12, 1.20, 1.30, 1.40], [1.01, 1.03, 1.21, 1.30, 1.41], [1.00, 1.02, 1.10, 1.31, 1.40]) == \
        [(0, 0, 0), (4, 3, 3), (5, 4, 4)]


def test_start_end_stride_and_their_errors(replica):
    _, frames, poses = replica
    ds = open_replica(replica, start=2, end=11, stride=3, prefetch=0)
    assert len(ds) == 3 and ds.retained_inds.tolist() == [2, 5, 8]
    assert [os.path.basename(p) for p in ds.color_paths] == [f"frame{t:06d}.jpg" for t in (2, 5, 8)]
    p32 = poses.astype(np.float32).astype(np.float64)
    for i, t in enumerate((2, 5, 8)):
        color, _, _, pose = ds[i]
        assert np.array_equal(color.numpy(), frames[t][0].astype(np.float32))
        assert np.abs(pose.numpy() - np.linalg.inv(p32[2]) @ p32[t]).max() <= 1e-6
    assert torch.equal(ds[0][3], torch.eye(4))
    assert len(open_replica(replica, stride=None)) == 12 and len(open_replica(replica, start=4)) == 8
    absolute = open_replica(replica, relative_pose=False, prefetch=0)
    assert np.array_equal(absolute[3][3].numpy(), poses[3].astype(np.float32))
    with pytest.raises(ValueError):
        open_replica(replica, start=-1)
    with pytest.raises(ValueError):
        open_replica(replica, start=5, end=5)
    with pytest.raises(ValueError):
        open_replica(replica, start=5, end=3)
    with pytest.raises(IndexError):
        ds[3]


def test_yaml_inheritance_and_the_fixture_configs(tmp_path):
    base, mid, leaf = (os.path.join(str(tmp_path), n) for n in ("base.yaml", "mid.yaml", "leaf.yaml"))
    with open(base, "w") as f:
        f.write("dataset_name: 'tum'\ncamera_params:\n  image_height: 480\n  image_width: 640\n  fx: 500.0\n  png_depth_scale: 5000.0\n")
    with open(mid, "w") as f:
        f.write(f"inherit_from: {base}\ncamera_params:\n  fx: 517.3\n  crop_edge: 8\n")
    with open(leaf, "w") as f:
        f.write(f"inherit_from: {mid}\ndataset_name: 'TUM'\ncamera_params:\n  image_width: 320\n")
    cfg = datasets.load_dataset_config(leaf)
    assert cfg["dataset_name"] == "TUM"
    assert cfg["camera_params"] == dict(image_height=480, image_width=320, fx=517.3, png_depth_scale=5000.0, crop_edge=8)
    want = {
        "replica.yaml": ("replica", dict(image_height=680, image_width=1200, fx=600.0, fy=600.0, cx=599.5, cy=339.5, png_depth_scale=6553.5,
                                         crop_edge=0)),
        os.path.join("TUM", "freiburg1_desk.yaml"): ("tum", dict(image_height=480, image_width=640, fx=517.3, fy=516.5, cx=318.6, cy=255.3,
                                                                 crop_edge=8, png_depth_scale=5000.0)),
        "scannet.yaml": ("scannet", dict(image_height=968, image_width=1296, fx=1169.621094, fy=1167.105103, cx=646.295044, cy=489.927032,
                                         png_depth_scale=1000.0)),
    }
    for name, (dataset_name, camera) in want.items():
        cfg = datasets.load_dataset_config(os.path.join(CONFIGS, name))
        assert cfg["dataset_name"] == dataset_name and cfg["camera_params"] == camera        # (no `distortion`: it is commented out)


def test_rejected_inputs(replica, tmp_path):
    with pytest.raises(NotImplementedError, match="undistort"):
        datasets.get_dataset(config(distortion=[0.2624, -0.9531, -0.0054, 0.0026, 1.1633]), replica[0], "room", device="cpu")
    with pytest.raises(ValueError, match="replica, replicav2, tum, scannet"):
        datasets.get_dataset(config("kitti"), replica[0], "room", device="cpu")
    frames, poses = files.seeded_frames(5, W, H, seed=7), files.seeded_poses(5, seed=7)
    base = files.write_replica(str(tmp_path), "short", frames, poses)
    os.remove(os.path.join(base, "results", "depth000004.png"))
    with pytest.raises(ValueError, match="same"):
        datasets.get_dataset(config(), str(tmp_path), "short", device="cpu")
    root = os.path.join(str(tmp_path), "exr")                                          # a TUM list may name any depth file
    os.makedirs(root)
    write_tum(root)
    with open(os.path.join(root, "depth.txt")) as f:
        listing = f.read()
    with open(os.path.join(root, "depth.txt"), "w") as f:
        f.write(listing.replace(".png", ".exr"))
    with pytest.raises(NotImplementedError, match="EXR"):
        datasets.get_dataset(config("tum", scale=5000.0), str(tmp_path), "exr", device="cpu")
    with pytest.raises(NotImplementedError, match="EXR"):
        datasets._decode_depth(os.path.join(root, "depth", "1.01.exr"))


def test_real_jpeg_is_pils_decode(tmp_path):
    frames, poses = files.seeded_frames(5, W, H, seed=8), files.seeded_poses(5, seed=8)
    base = files.write_replica(str(tmp_path), "jpeg", frames, poses, color_ext="jpg")
    ds = datasets.get_dataset(config(), str(tmp_path), "jpeg", desired_height=H, desired_width=W, device="cpu")
    with Image.open(os.path.join(base, "results", "frame000003.jpg")) as im:
        assert im.format == "JPEG"
        want = np.asarray(im.convert("RGB")).astype(np.float32)
    assert np.array_equal(ds[3][0].numpy(), want)


def items_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_at_size_shares_the_decoded_frame(replica, monkeypatch):
    ds = open_replica(replica, prefetch=0)
    half, third = ds.at_size(6, 8), ds.at_size(5, 7)
    fresh = open_replica(replica, desired_height=6, desired_width=8, prefetch=0)
    decoded = []
    real = datasets._decode_color
    monkeypatch.setattr(datasets, "_decode_color", lambda path: (decoded.append(path), real(path))[1])
    for t in (0, 7, 3):
        full, a, b = ds[t], half[t], third[t]
        assert tuple(a[0].shape) == (6, 8, 3) and tuple(b[0].shape) == (5, 7, 3) and tuple(full[0].shape) == (H, W, 3)
    assert len(decoded) == 3 and ds.stats['fetches'] == 3 and ds.stats['items'] == 9     # three sizes of a frame: one decode
    for t in (0, 7, 3):
        assert items_equal(half[t], fresh[t])
        assert np.array_equal(half[t][2].numpy(), frame_ref.scale_intrinsics(ds[t][2].numpy(), 6 / H, 8 / W))
    assert torch.equal(ds[7][2], open_replica(replica)[7][2])                              # (the full-size dataset keeps its own)


def test_prefetch_gives_the_same_items_in_order_and_at_random(replica):
    plain, ahead = open_replica(replica, prefetch=0, desired_height=7, desired_width=9), open_replica(replica, prefetch=4, desired_height=7,
                                                                                                    desired_width=9)
    try:
        for t in range(12):
            assert items_equal(plain[t], ahead[t]), t
        assert ahead.stats['prefetch_hits'] == 11 and plain.stats['prefetch_hits'] == 0
        for t in (5, 0, 11, 3, 4, 5, 9, 2, 2, 10):
            assert items_equal(plain[t], ahead[t]), t
    finally:
        ahead.close()
    assert items_equal(plain[6], ahead[6])                                                 # closed: decodes on demand
