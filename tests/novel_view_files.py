"""Writers of tiny sequences in the two layouts that have a held-out split (splatam_amd/datasets.py: ScannetPPDataset, ReplicaV2Dataset
with ``use_train_split=False``), for the loader tests and the run-from-disk test.  TEST INFRASTRUCTURE, in the style of
tests/dataset_files.py: the layouts are restated from the reference's loaders (datasets/gradslam_datasets/scannetpp.py and
replica.py:69-144), which cannot be executed here (cv2 and natsort are absent)."""
import json
import os

import numpy as np
from PIL import Image

FLIP = np.diag([1.0, -1.0, -1.0, 1.0])


def _save(path, array, fmt="PNG"):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(array).save(path, format=fmt)


def opengl_c2w(pose):
    """The ``transform_matrix`` (camera-to-world, OpenGL axes) whose loader pose ``P @ c2w @ P.T`` is ``pose``: P is its own inverse."""
    return FLIP @ np.asarray(pose, dtype=np.float64) @ FLIP.T


def write_scannetpp(root, sequence, train, test, camera, train_order=None, test_order=None, extra_entries=True):
    """``<root>/<sequence>/dslr/``: train_test_lists.json, nerfstudio/transforms_undistorted.json, undistorted_images/<name>,
    undistorted_depths/<name with .JPG replaced by .png>.

    ``train`` / ``test``: lists of ``(name, rgb uint8 [h, w, 3], depth uint16 [h, w], pose [4, 4] in the loader's axes, is_bad)``;
    ``camera``: dict with h, w, fl_x, fl_y, cx, cy.  ``train_order`` / ``test_order``: the names as the split lists give them (default:
    the order of ``train`` / ``test``); the transforms file lists its entries in ALPHABETICAL order, so a loader that follows the
    transforms file instead of the lists is caught.  The colour files carry PNG bytes under the .JPG name (PIL decides by content):
    the pixels survive exactly.  ``extra_entries``: the transforms file also lists a frame that is in neither list."""
    base = os.path.join(root, sequence, "dslr")

    def entries(items):
        out = []
        for name, rgb, raw, pose, is_bad in sorted(items, key=lambda item: item[0]):
            _save(os.path.join(base, "undistorted_images", name), rgb)
            _save(os.path.join(base, "undistorted_depths", name.replace(".JPG", ".png")), raw)
            out.append({"file_path": name, "transform_matrix": opengl_c2w(pose).tolist(), "is_bad": bool(is_bad)})
        return out

    meta = dict(camera)
    meta["frames"], meta["test_frames"] = entries(train), entries(test)
    if extra_entries:
        meta["frames"].append({"file_path": "DSC09999.JPG", "transform_matrix": np.eye(4).tolist(), "is_bad": False})
    lists = {"train": list(train_order) if train_order is not None else [item[0] for item in train],
             "test": list(test_order) if test_order is not None else [item[0] for item in test]}
    os.makedirs(os.path.join(base, "nerfstudio"), exist_ok=True)
    with open(os.path.join(base, "train_test_lists.json"), "w") as f:
        json.dump(lists, f)
    with open(os.path.join(base, "nerfstudio", "transforms_undistorted.json"), "w") as f:
        json.dump(meta, f)
    return base


def _trajectory(path, poses):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for p in poses:
            f.write(" ".join(repr(float(x)) for x in np.asarray(p).reshape(-1)) + "\n")


def write_replica_v2_splits(root, sequence, train_frames, train_poses, test_frames, test_poses):
    """imap/00 (the train split) and imap/01 (the held-out one): rgb/rgb_<t>.png (not zero padded), depth/depth_<t>.png, traj_w_c.txt.
    ``*_poses`` may hold more or fewer lines than there are frames."""
    base = os.path.join(root, sequence, "imap")
    for folder, frames, poses in (("00", train_frames, train_poses), ("01", test_frames, test_poses)):
        for t, (rgb, raw) in enumerate(frames):
            _save(os.path.join(base, folder, "rgb", f"rgb_{t}.png"), rgb)
            _save(os.path.join(base, folder, "depth", f"depth_{t}.png"), raw)
        _trajectory(os.path.join(base, folder, "traj_w_c.txt"), poses)
    return base
