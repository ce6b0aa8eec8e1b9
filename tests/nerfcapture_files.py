"""Writer of a tiny NeRFCapture capture in the layout splatam_amd/datasets.py reads (beside tests/dataset_files.py; PIL only).  TEST
INFRASTRUCTURE: the layout is restated from the reference's loader and from the demo that writes such captures
(datasets/gradslam_datasets/nerfcapture.py, scripts/iphone_demo.py:60-150), neither of which can be executed here (cv2, natsort and
cyclonedds are absent): ``transforms.json`` with ``w, h, fl_x, fl_y, cx, cy`` and ``frames[]`` of ``file_path`` = ``rgb/<t>.png`` and a
camera-to-world ``transform_matrix`` in OpenGL axes, the images ``rgb/<t>.png`` and 16-bit ``depth/<t>.png`` at a size of their own.
The names are NOT zero padded, so 10.png sorts before 2.png lexicographically."""
import json
import os

import numpy as np
from PIL import Image


def write_nerfcapture(root, sequence, frames, poses_gl, fl_x, fl_y, cx, cy, listed=None, shuffle_seed=0):
    """``frames``: (rgb uint8 [H, W, 3], depth uint16 [H', W']) per frame; ``poses_gl``: their camera-to-world matrices as the app
    sends them.  ``listed``: the frame indices that get an entry in transforms.json (default all), written in a shuffled order -- the
    loader must go by ``file_path``, not by position."""
    base = os.path.join(root, sequence)
    os.makedirs(os.path.join(base, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(base, "depth"), exist_ok=True)
    for t, (rgb, raw) in enumerate(frames):
        Image.fromarray(rgb).save(os.path.join(base, "rgb", f"{t}.png"))
        Image.fromarray(raw).save(os.path.join(base, "depth", f"{t}.png"))
    listed = list(range(len(frames))) if listed is None else list(listed)
    order = np.random.default_rng(shuffle_seed).permutation(len(listed))
    h, w = frames[0][0].shape[:2]
    meta = dict(fl_x=fl_x, fl_y=fl_y, cx=cx, cy=cy, w=w, h=h, integer_depth_scale=1.0 / 6553.5,
                frames=[dict(file_path=f"rgb/{listed[i]}.png", depth_path=f"depth/{listed[i]}.png",
                             transform_matrix=np.asarray(poses_gl[listed[i]], dtype=np.float64).tolist()) for i in order])
    with open(os.path.join(base, "transforms.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return base
