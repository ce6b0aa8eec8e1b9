"""The two loaders with a held-out split (splatam_amd/datasets.py: ScannetPPDataset, ReplicaV2Dataset with ``use_train_split=False``)
with ``device="cpu"`` over tiny sequences written into tmp_path (tests/novel_view_files.py).

As in tests/test_datasets_cpu.py the reference's loaders (datasets/gradslam_datasets/scannetpp.py, replica.py:69-144) cannot be
executed here -- no cv2, no natsort -- so the expected values are RESTATED: frames in the order of the split list (not sorted),
``ignore_bad``, the first training frame as item 0 of the held-out split, the ``.JPG`` -> ``.png`` depth name, poses
``P c2w P^T`` made relative to item 0, intrinsics from the JSON scaled by the two size ratios, depth
``float32(float64(raw) / 1000)``."""
import json
import os

import numpy as np
import pytest
import torch

import dataset_files as files
import frame_ref
import novel_view_files as nv

from splatam_amd import datasets

W, H = 16, 12
CAMERA = dict(w=W, h=H, fl_x=14.0, fl_y=15.0, cx=7.5, cy=5.5)
# the train list is deliberately NOT in alphabetical order, and neither is the test list
TRAIN_ORDER = ["DSC00007.JPG", "DSC00002.JPG", "DSC00011.JPG", "DSC00004.JPG", "DSC00009.JPG"]
TEST_ORDER = ["DSC00020.JPG", "DSC00013.JPG", "DSC00016.JPG"]
BAD = {"DSC00007.JPG", "DSC00004.JPG", "DSC00013.JPG"}       # the FIRST training frame is bad, one more, and one held-out frame


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scannetpp"))
    frames = files.seeded_frames(len(TRAIN_ORDER) + len(TEST_ORDER), W, H, seed=11)
    poses = files.seeded_poses(len(TRAIN_ORDER) + len(TEST_ORDER), seed=11)
    items = {name: (name, frames[i][0], frames[i][1], poses[i], name in BAD) for i, name in enumerate(TRAIN_ORDER + TEST_ORDER)}
    nv.write_scannetpp(root, "8b5caf3398", [items[n] for n in sorted(TRAIN_ORDER)], [items[n] for n in sorted(TEST_ORDER)], CAMERA,
                       train_order=TRAIN_ORDER, test_order=TEST_ORDER)
    return root, items


def open_scene(scene, **kw):
    kw = dict(dict(desired_height=H, desired_width=W, device="cpu", prefetch=0), **kw)
    return datasets.get_dataset({"dataset_name": "scannetpp"}, scene[0], "8b5caf3398", **kw)


def expected_relative(items, names):
    """inv(p0) @ p_i of the float32 loader poses: the JSON's c2w goes through float32 (the reference builds a float tensor), then
    P c2w P^T; P flips signs only, so the round trip through the writer's ``opengl_c2w`` is exact."""
    p = np.stack([(nv.FLIP @ nv.opengl_c2w(items[n][3]).astype(np.float32).astype(np.float64) @ nv.FLIP.T).astype(np.float32) for n in names]).astype(np.float64)
    return np.linalg.inv(p[0])[None] @ p


def check_items(ds, items, names, h=H, w=W):
    assert len(ds) == len(names)
    assert [os.path.basename(p) for p in ds.color_paths] == names
    assert [os.path.basename(p) for p in ds.depth_paths] == [n.replace(".JPG", ".png") for n in names]
    assert all(os.path.basename(os.path.dirname(p)) == "undistorted_images" for p in ds.color_paths)
    assert all(os.path.basename(os.path.dirname(p)) == "undistorted_depths" for p in ds.depth_paths)
    want_pose = expected_relative(items, names)
    k = np.eye(4, dtype=np.float32)
    k[0, 0], k[1, 1], k[0, 2], k[1, 2] = 14.0, 15.0, 7.5, 5.5
    for t, name in enumerate(names):
        color, depth, intrinsics, pose = ds[t]
        _, rgb, raw, _, _ = items[name]
        assert color.dtype == depth.dtype == intrinsics.dtype == pose.dtype == torch.float32
        assert tuple(color.shape) == (h, w, 3) and tuple(depth.shape) == (h, w, 1)
        if (h, w) == (H, W):
            assert np.array_equal(color.numpy(), rgb.astype(np.float32))
        else:
            assert np.abs(color.numpy().astype(np.float64) - frame_ref.resize_linear(rgb, h, w)).max() <= 255 * 1e-6
        assert np.array_equal(depth.numpy()[..., 0], (frame_ref.resize_nearest(raw, h, w).astype(np.float64) / 1000.0).astype(np.float32))
        assert np.array_equal(intrinsics.numpy(), frame_ref.scale_intrinsics(k, h / H, w / W))
        assert np.abs(pose.numpy() - want_pose[t]).max() <= 1e-6
    assert torch.equal(ds[0][3], torch.eye(4))


def test_train_split_follows_the_list_not_the_alphabet(scene):
    ds = open_scene(scene, use_train_split=True, ignore_bad=False)
    check_items(ds, scene[1], TRAIN_ORDER)
    assert ds.png_depth_scale == 1000.0 and (ds.orig_height, ds.orig_width) == (H, W)
    assert "scannetpp" in datasets.SUPPORTED and isinstance(ds, datasets.ScannetPPDataset)


def test_train_split_ignore_bad_drops_marked_frames(scene):
    ds = open_scene(scene, use_train_split=True, ignore_bad=True)
    check_items(ds, scene[1], [n for n in TRAIN_ORDER if n not in BAD])


def test_held_out_split_starts_with_the_first_training_frame(scene):
    """Item 0 is the first name of the TRAIN list, looked up in frames[]; the test names follow, looked up in test_frames[]: every
    held-out pose is relative to the first training frame."""
    ds = open_scene(scene, use_train_split=False, ignore_bad=False)
    check_items(ds, scene[1], [TRAIN_ORDER[0]] + TEST_ORDER)


def test_held_out_split_keeps_a_bad_first_training_frame(scene):
    ds = open_scene(scene, use_train_split=False, ignore_bad=True)
    assert TRAIN_ORDER[0] in BAD
    check_items(ds, scene[1], [TRAIN_ORDER[0]] + [n for n in TEST_ORDER if n not in BAD])


def test_resized_frames_scale_the_json_intrinsics(scene):
    ds = open_scene(scene, use_train_split=False, desired_height=7, desired_width=9)
    check_items(ds, scene[1], [TRAIN_ORDER[0]] + TEST_ORDER, h=7, w=9)


def test_slicing_and_the_class_defaults(scene):
    ds = datasets.ScannetPPDataset(basedir=scene[0], sequence="8b5caf3398", device="cpu", use_train_split=True, start=1, end=4)
    assert [os.path.basename(p) for p in ds.color_paths] == TRAIN_ORDER[1:4]
    assert (ds.desired_height, ds.desired_width) == (1168, 1752)        # the reference's defaults; nothing is decoded until an item is fetched


def test_missing_files_and_entries_name_the_path(scene, tmp_path):
    root, items = scene
    with pytest.raises(FileNotFoundError, match="train_test_lists.json"):
        datasets.get_dataset({"dataset_name": "scannetpp"}, str(tmp_path), "nothing", device="cpu")
    base = nv.write_scannetpp(str(tmp_path), "partial", [items[n] for n in TRAIN_ORDER], [items[n] for n in TEST_ORDER], CAMERA)
    os.remove(os.path.join(base, "nerfstudio", "transforms_undistorted.json"))
    with pytest.raises(FileNotFoundError, match="transforms_undistorted.json"):
        datasets.get_dataset({"dataset_name": "scannetpp"}, str(tmp_path), "partial", device="cpu")
    # a name in a list with no entry in the transforms file
    base = nv.write_scannetpp(str(tmp_path), "unlisted", [items[n] for n in TRAIN_ORDER], [items[n] for n in TEST_ORDER], CAMERA,
                              train_order=TRAIN_ORDER + ["DSC00099.JPG"], test_order=TEST_ORDER + ["DSC00007.JPG"])
    with pytest.raises(ValueError, match=r"transforms_undistorted\.json.*DSC00099\.JPG"):
        datasets.get_dataset({"dataset_name": "scannetpp"}, str(tmp_path), "unlisted", device="cpu", use_train_split=True)
    # a TRAIN name in the test list is not found: held-out names are looked up in test_frames[] only
    with pytest.raises(ValueError, match=r"DSC00007\.JPG.*test_frames"):
        datasets.get_dataset({"dataset_name": "scannetpp"}, str(tmp_path), "unlisted", device="cpu", use_train_split=False)
    with pytest.raises(ValueError, match="replica, replicav2, tum, scannet, scannetpp, nerfcapture"):
        datasets.get_dataset({"dataset_name": "kitti"}, str(tmp_path), "unlisted", device="cpu")


def test_run_builds_the_dataset_of_an_experiment_file_without_gradslam_data_cfg(scene):
    """What ``python -m splatam_amd.run`` passes for configs/scannetpp/splatam.py: ``{"dataset_name": ...}`` and both switches."""
    cfg = {"dataset_name": "ScanNetPP"}
    ds = datasets.get_dataset(config_dict=cfg, basedir=scene[0], sequence="8b5caf3398", start=0, end=-1, stride=1, desired_height=6, desired_width=8,
                              device=torch.device("cpu"), relative_pose=True, ignore_bad=False, use_train_split=False, prefetch=2)
    try:
        assert len(ds) == 1 + len(TEST_ORDER) and tuple(ds[1][0].shape) == (6, 8, 3)
        assert tuple(ds.at_size(3, 4)[2][1].shape) == (3, 4, 1)
    finally:
        ds.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# ReplicaV2
# ---------------------------------------------------------------------------------------------------------------------------------
def replica_config():
    return dict(dataset_name="replicav2", camera_params=dict(image_height=H, image_width=W, fx=14.0, fy=15.0, cx=7.5, cy=5.5, png_depth_scale=6553.5))


def test_replica_v2_held_out_split(tmp_path):
    """rgb_0 / depth_0 of imap/00 with line 0 of its trajectory, then imap/01 in natural order with the FIRST len - 1 lines of its
    trajectory (which holds more)."""
    train, test = files.seeded_frames(3, W, H, seed=21), files.seeded_frames(12, W, H, seed=22)
    train_poses, test_poses = files.seeded_poses(3, seed=21), files.seeded_poses(15, seed=22)
    nv.write_replica_v2_splits(str(tmp_path), "room", train, train_poses, test, test_poses)
    ds = datasets.get_dataset(replica_config(), str(tmp_path), "room", desired_height=H, desired_width=W, device="cpu", use_train_split=False, prefetch=0)
    assert len(ds) == 13
    sep = os.sep
    assert [p.split(sep)[-4:] for p in ds.color_paths] == [["imap", "00", "rgb", "rgb_0.png"]] + [["imap", "01", "rgb", f"rgb_{t}.png"] for t in range(12)]
    assert [p.split(sep)[-4:] for p in ds.depth_paths] == [["imap", "00", "depth", "depth_0.png"]] + [["imap", "01", "depth", f"depth_{t}.png"] for t in range(12)]
    all_poses = np.concatenate([train_poses[:1], test_poses[:12]]).astype(np.float32).astype(np.float64)
    want = np.linalg.inv(all_poses[0])[None] @ all_poses
    for t in (0, 1, 3, 11, 12):
        color, depth, _, pose = ds[t]
        rgb, raw = train[0] if t == 0 else test[t - 1]
        assert np.array_equal(color.numpy(), rgb.astype(np.float32))
        assert np.array_equal(depth.numpy()[..., 0], (raw.astype(np.float64) / 6553.5).astype(np.float32))
        assert np.abs(pose.numpy() - want[t]).max() <= 1e-6
    # the train split of the same tree is untouched by the held-out folder
    tr = datasets.get_dataset(replica_config(), str(tmp_path), "room", desired_height=H, desired_width=W, device="cpu", use_train_split=True, prefetch=0)
    assert [p.split(sep)[-4:] for p in tr.color_paths] == [["imap", "00", "rgb", f"rgb_{t}.png"] for t in range(3)]


def test_replica_v2_short_trajectories_are_errors(tmp_path):
    train, test = files.seeded_frames(4, W, H, seed=23), files.seeded_frames(5, W, H, seed=24)
    # a train trajectory shorter than the image count
    nv.write_replica_v2_splits(str(tmp_path), "short_train", train, files.seeded_poses(3, seed=23), test, files.seeded_poses(5, seed=24))
    with pytest.raises(ValueError, match=r"00.traj_w_c\.txt"):
        datasets.get_dataset(replica_config(), str(tmp_path), "short_train", device="cpu", use_train_split=True)
    # a held-out trajectory shorter than the held-out images
    nv.write_replica_v2_splits(str(tmp_path), "short_test", train, files.seeded_poses(4, seed=23), test, files.seeded_poses(4, seed=24))
    with pytest.raises(ValueError, match=r"01.traj_w_c\.txt"):
        datasets.get_dataset(replica_config(), str(tmp_path), "short_test", device="cpu", use_train_split=False)
    # an empty train trajectory cannot give the first training pose
    base = nv.write_replica_v2_splits(str(tmp_path), "no_first", train, [], test, files.seeded_poses(5, seed=24))
    assert os.path.getsize(os.path.join(base, "00", "traj_w_c.txt")) == 0
    with pytest.raises(ValueError, match=r"00.traj_w_c\.txt"):
        datasets.get_dataset(replica_config(), str(tmp_path), "no_first", device="cpu", use_train_split=False)


def test_transforms_json_round_trip_of_the_writer():
    """The writer's ``opengl_c2w`` is the inverse of the loader's P c2w P^T (P is its own inverse and flips signs only)."""
    pose = files.seeded_poses(1, seed=3)[0]
    assert np.array_equal(nv.FLIP @ nv.opengl_c2w(pose) @ nv.FLIP.T, pose)
    assert json.loads(json.dumps(nv.opengl_c2w(pose).tolist())) == nv.opengl_c2w(pose).tolist()
