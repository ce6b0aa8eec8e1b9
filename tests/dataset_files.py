"""Writers of tiny sequences in the dataset layouts splatam_amd/datasets.py reads, for the loader tests.  TEST INFRASTRUCTURE: the
layouts are restated from the reference's loaders (datasets/gradslam_datasets/{replica,tum,scannet}.py), which cannot be executed
here (cv2, imageio and natsort are absent)."""
import os

import numpy as np
from PIL import Image


def seeded_frames(n, cw, ch, zw=None, zh=None, seed=0):
    """n frames of (rgb uint8 [ch, cw, 3], depth uint16 [zh, zw]) with some zero depths, 0 and 65535 among the values."""
    rng = np.random.default_rng(seed)
    zw, zh = zw or cw, zh or ch
    out = []
    for _ in range(n):
        rgb = rng.integers(0, 256, size=(ch, cw, 3), dtype=np.uint8)
        raw = rng.integers(1, 65536, size=(zh, zw)).astype(np.uint16)
        raw[rng.random((zh, zw)) < 0.1] = 0
        raw[0, 0], raw[-1, -1] = 65535, 0
        out.append((rgb, raw))
    return out


def seeded_poses(n, seed=0):
    """n camera-to-world matrices [n, 4, 4] float64: proper rotations about a seeded axis, a drifting translation; the first is NOT
    the identity."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed + 1000)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    poses = np.tile(np.eye(4), (n, 1, 1))
    for t in range(n):
        poses[t, :3, :3] = Rotation.from_rotvec(axis * (0.3 + 0.05 * t)).as_matrix()
        poses[t, :3, 3] = np.array([0.4, -0.2, 1.0]) + 0.03 * t * np.array([1.0, 0.5, -0.25])
    return poses


def _save(path, array):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(array).save(path)


def _trajectory(path, poses):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for p in poses:
            f.write(" ".join(repr(float(x)) for x in np.asarray(p).reshape(-1)) + "\n")


def write_replica(root, sequence, frames, poses, color_ext="png"):
    """results/frame<000000>.<ext>, results/depth<000000>.png, traj.txt.  The real dataset's colour is JPEG; PNG under the .jpg name
    keeps the bytes (PIL decides by content), ``color_ext="jpg"`` writes real JPEG."""
    base = os.path.join(root, sequence)
    for t, (rgb, raw) in enumerate(frames):
        path = os.path.join(base, "results", f"frame{t:06d}.jpg")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(rgb).save(path, format="PNG" if color_ext == "png" else "JPEG")
        _save(os.path.join(base, "results", f"depth{t:06d}.png"), raw)
    _trajectory(os.path.join(base, "traj.txt"), poses)
    return base


def write_replica_v2(root, sequence, frames, poses):
    """imap/00/rgb/rgb_<t>.png (NOT zero padded: rgb_10 must sort after rgb_2), imap/00/depth/depth_<t>.png, imap/00/traj_w_c.txt."""
    base = os.path.join(root, sequence, "imap", "00")
    for t, (rgb, raw) in enumerate(frames):
        _save(os.path.join(base, "rgb", f"rgb_{t}.png"), rgb)
        _save(os.path.join(base, "depth", f"depth_{t}.png"), raw)
    _trajectory(os.path.join(base, "traj_w_c.txt"), poses)
    return base


def write_scannet(root, sequence, frames, poses):
    """color/<t>.jpg, depth/<t>.png, pose/<t>.txt with a 4 x 4 matrix each (names not zero padded)."""
    base = os.path.join(root, sequence)
    for t, (rgb, raw) in enumerate(frames):
        path = os.path.join(base, "color", f"{t}.jpg")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(rgb).save(path, format="PNG")
        _save(os.path.join(base, "depth", f"{t}.png"), raw)
        os.makedirs(os.path.join(base, "pose"), exist_ok=True)
        np.savetxt(os.path.join(base, "pose", f"{t}.txt"), poses[t], fmt="%.17g")
    return base
