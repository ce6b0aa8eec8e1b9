"""RGB-D sequences from disk with the item contract of the reference's gradslam datasets, and the device frame ingest behind them.

=============================================  =============================================
here                                           reference (restated; nothing is copied)
=============================================  =============================================
``load_dataset_config``                        datasets/gradslam_datasets/dataconfig.py:5-54 (YAML with recursive ``inherit_from``)
``get_dataset``                                scripts/splatam.py:40-64 (replica, replicav2, tum, scannet, scannetpp, nerfcapture)
``RGBDDataset``                                datasets/gradslam_datasets/basedataset.py:105-341
``ReplicaDataset`` / ``ReplicaV2Dataset``      datasets/gradslam_datasets/replica.py (ReplicaV2: the train split and the held-out one)
``TUMDataset``                                 datasets/gradslam_datasets/tum.py (nearest-timestamp association, 1/32 s thinning)
``ScannetDataset``                             datasets/gradslam_datasets/scannet.py
``ScannetPPDataset``                           datasets/gradslam_datasets/scannetpp.py (``dslr/``: split lists, nerfstudio transforms,
                                               undistorted images and depths; the train split and the held-out one)
``NeRFCaptureDataset``                         datasets/gradslam_datasets/nerfcapture.py (``transforms.json``, ``rgb/*``, ``depth/*``)
``ingest_planes_cpu`` (from ``frames``)        scripts/iphone_demo.py:218-243 (a live frame's bytes and depth at the loop's sizes; the
                                               host form of ``fused.ingest_planes``, which ``session.SlamSession.add_raw_frame`` runs)
=============================================  =============================================

``dataset[i]`` is ``(color [H, W, 3] float32 in 0..255, depth [H, W, 1] float32 in metres, intrinsics [4, 4], pose [4, 4])`` on
``device``, poses camera-to-world relative to the first retained frame: what ``pipeline.rgbd_slam`` and ``evaluation.evaluate`` take.
A held-out split (``use_train_split=False`` of ScanNet++ and ReplicaV2) starts with the FIRST TRAINING FRAME, the map's origin, so that
every held-out pose is relative to it: what ``evaluation.evaluate_novel_views`` takes.

Where the reference decodes to float64, resizes twice with OpenCV on one core and uploads floats, once per resolution, this decodes
ONCE with PIL (ahead of the loop, on a few threads, into reused pinned buffers), uploads the raw bytes (4 MB at 1200 x 680 instead of
13 MB) and lets one kernel, ``fused.ingest_frame`` (frames.py; csrc/frameprep.hip, splat_frame_ingest), write the frame at every size wanted:
``dataset.at_size(h, w)`` is a second dataset over the same files that shares the decoded and uploaded frame of the last index
fetched.  With ``device="cpu"`` the same arithmetic runs in torch on the host (``ingest_frame_cpu``).  The resize rules are OpenCV's documented
ones as csrc/frame_math.h restates them; they are not pinned against OpenCV, which is not available here.

Not supported (NotImplementedError): lens undistortion (``camera_params.distortion``; every data config the reference ships has it
commented out, and cv2.undistort cannot be pinned here), ``.exr`` depth, embeddings.
"""
from __future__ import annotations

import glob
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import slam
from .frames import ingest_frame_cpu, ingest_planes_cpu  # noqa: F401  (the host forms of fused.ingest_frame / ingest_planes)

SUPPORTED = ("replica", "replicav2", "tum", "scannet", "scannetpp", "nerfcapture")
MAX_WORKERS = 4             # decode threads (PIL releases the GIL while it inflates); never sized by the host's core count
MAX_DEPTH = 4               # frames decoded ahead


# --------------------------------------------------------------------------
# configuration
# --------------------------------------------------------------------------

def _update_recursive(into, other):
    for key, value in other.items():
        if isinstance(value, dict):
            if not isinstance(into.get(key), dict):
                into[key] = {}
            _update_recursive(into[key], value)
        else:
            into[key] = value


def load_dataset_config(path):
    """The dict of a dataset YAML; a file with ``inherit_from: other.yaml`` starts from that file's dict (recursively) and lays its
    own entries over it, nested dicts merged key by key."""
    import yaml
    with open(path, "r") as f:
        own = yaml.full_load(f) or {}
    parent = own.get("inherit_from")
    cfg = load_dataset_config(parent) if parent is not None else {}
    _update_recursive(cfg, own)
    return cfg


def natural_sorted(names):
    """Names ordered with every run of digits compared as an integer: frame2 before frame10."""
    def key(name):
        return [(0, int(part), "") if part.isdigit() else (1, 0, part.lower()) for part in re.split(r"(\d+)", name) if part != ""]
    return sorted(names, key=key)


# --------------------------------------------------------------------------
# decoding and read-ahead
# --------------------------------------------------------------------------

def _decode_color(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "RGB":
            im = im.convert("RGB")
        return np.asarray(im)


def _decode_depth(path):
    if path.lower().endswith(".exr"):
        raise NotImplementedError(f"{path}: EXR depth is not supported (no OpenEXR reader here); convert the depth to 16-bit PNG")
    from PIL import Image
    with Image.open(path) as im:
        raw = np.asarray(im)
    if raw.ndim != 2:
        raise ValueError(f"{path}: a depth image must have one channel (got shape {raw.shape})")
    if raw.dtype != np.uint16:                              # (8-bit PNGs, and 16-bit ones that older PIL versions open as int32)
        if raw.size and (raw.min() < 0 or raw.max() > 65535):
            raise ValueError(f"{path}: depth values outside 0..65535")
        raw = raw.astype(np.uint16)
    return raw


class _Slot:
    """One decoded frame on the host.  For a HIP device the two arrays live in pinned buffers that are kept and written again
    (``busy``: the event after the last upload from them); for the CPU they are the decoder's own arrays."""

    def __init__(self, pinned):
        self.pinned, self.rgb, self.depth, self.busy = pinned, None, None, None

    def fill(self, rgb, depth):
        if not self.pinned:
            self.rgb, self.depth = torch.from_numpy(np.array(rgb)), torch.from_numpy(np.array(depth))       # (PIL's arrays are read-only)
            return
        if self.busy is not None:
            self.busy.synchronize()                          # (the upload of the frame these buffers held has finished)
            self.busy = None
        if self.rgb is None or tuple(self.rgb.shape) != rgb.shape:
            self.rgb = torch.empty(rgb.shape, dtype=torch.uint8, pin_memory=True)
        if self.depth is None or tuple(self.depth.shape) != depth.shape:
            self.depth = torch.empty(depth.shape, dtype=torch.uint16, pin_memory=True)
        np.copyto(self.rgb.numpy(), rgb)
        np.copyto(self.depth.numpy(), depth)


class _FrameSource:
    """The files of one sequence and the raw frame of the last index fetched, shared by a dataset and its ``at_size`` siblings:
    three sizes of one frame decode and upload once.  ``prefetch`` > 0: after index i is fetched, the next ``prefetch`` (at most 4)
    frames are decoded on at most 4 threads; an index outside that window is decoded on the spot, so access stays random."""

    def __init__(self, color_paths, depth_paths, device, prefetch):
        self.color_paths, self.depth_paths = list(color_paths), list(depth_paths)
        self.device = torch.device(device)
        self.on_device = self.device.type == "cuda"
        self.depth_ahead = max(0, min(int(prefetch), MAX_DEPTH))
        self._pool = ThreadPoolExecutor(max_workers=min(MAX_WORKERS, self.depth_ahead)) if self.depth_ahead else None
        self._free = [_Slot(self.on_device) for _ in range(self.depth_ahead + 1)]
        self._pending = {}                                   # index -> (future, slot)
        self._last = None                                    # (index, rgb, depth) on the device
        self.stats = dict(fetches=0, prefetch_hits=0, fetch_s=0.0, wait_s=0.0, upload_s=0.0, item_s=0.0, items=0)

    def _decode(self, index, slot):
        slot.fill(_decode_color(self.color_paths[index]), _decode_depth(self.depth_paths[index]))
        return slot

    def _release(self, slot):
        self._free.append(slot)

    def _drop(self, index):
        future, slot = self._pending.pop(index)
        if future.cancel():
            self._release(slot)
        else:
            future.add_done_callback(lambda _f, s=slot: self._release(s))

    def raw(self, index):
        """(rgb uint8 [H, W, 3], depth uint16 [H', W']) of frame ``index`` on the device."""
        if self._last is not None and self._last[0] == index:
            return self._last[1], self._last[2]
        t0 = time.perf_counter()
        self.stats['fetches'] += 1
        pooled = True
        if index in self._pending:
            future, slot = self._pending.pop(index)
            self.stats['prefetch_hits'] += 1
            future.result()
        else:
            pooled = bool(self._free)                        # (every buffer is out with a decode thread: a throw-away one)
            slot = self._free.pop() if pooled else _Slot(self.on_device)
            self._decode(index, slot)
        t1 = time.perf_counter()
        self.stats['wait_s'] += t1 - t0
        if self.on_device:
            rgb, depth = slot.rgb.to(self.device, non_blocking=True), slot.depth.to(self.device, non_blocking=True)
            slot.busy = torch.cuda.Event()
            slot.busy.record(torch.cuda.current_stream(self.device))
        else:
            rgb, depth = slot.rgb, slot.depth
            slot.rgb = slot.depth = None
        if pooled:
            self._release(slot)
        self._last = (index, rgb, depth)
        self.stats['upload_s'] += time.perf_counter() - t1
        if self._pool is not None:
            window = range(index + 1, min(index + 1 + self.depth_ahead, len(self.color_paths)))
            for stale in [i for i in self._pending if i not in window]:
                self._drop(stale)
            for i in window:
                if i not in self._pending and self._free:
                    slot = self._free.pop()
                    self._pending[i] = (self._pool.submit(self._decode, i, slot), slot)
        self.stats['fetch_s'] += time.perf_counter() - t0
        return rgb, depth

    def close(self):
        if self._pool is not None:
            for index in list(self._pending):
                self._drop(index)
            self._pool.shutdown(wait=True)
            self._pool = None
            self.depth_ahead = 0


# --------------------------------------------------------------------------
# datasets
# --------------------------------------------------------------------------

class RGBDDataset:
    """Base of the loaders: a subclass names the files (``_filepaths``) and reads the camera-to-world poses (``_load_poses``).

    ``stride`` / ``start`` / ``end`` slice the frame list (``end=-1``: all), ``desired_height`` / ``desired_width`` are the size
    of the frames handed over, ``relative_pose`` makes poses relative to the first retained frame (which is then exactly the
    identity).  ``prefetch``: frames decoded ahead (0: none; at most 4).  Other keyword arguments (``ignore_bad``,
    ``use_train_split=True``, ...) are accepted and ignored, as the reference's classes do."""

    def __init__(self, config_dict, stride=1, start=0, end=-1, desired_height=480, desired_width=640, device="cuda:0",
                 relative_pose=True, prefetch=MAX_DEPTH, **kwargs):
        cam = config_dict["camera_params"]
        self.name = config_dict["dataset_name"]
        self.device = torch.device(device)
        self.png_depth_scale = float(cam["png_depth_scale"])
        self.orig_height, self.orig_width = cam["image_height"], cam["image_width"]
        self.fx, self.fy, self.cx, self.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        self.relative_pose = relative_pose
        if kwargs.get("load_embeddings"):
            raise NotImplementedError("embeddings are not supported")
        if start < 0:
            raise ValueError(f"start must not be negative (got {start})")
        if not (end == -1 or end > start):
            raise ValueError(f"end ({end}) must be -1 (use all images) or greater than start ({start})")
        if cam.get("distortion") is not None:
            raise NotImplementedError(
                "camera_params.distortion: lens undistortion is not implemented -- the reference applies cv2.undistort to the colour "
                "image, which is not available here and whose resampling could not be checked; remove the entry (every data config "
                "the reference ships has it commented out) or undistort the images beforehand")
        color_paths, depth_paths = self._filepaths()
        if len(color_paths) != len(depth_paths):
            raise ValueError(f"number of colour ({len(color_paths)}) and depth ({len(depth_paths)}) images must be the same")
        for path in depth_paths:
            if path.lower().endswith(".exr"):
                raise NotImplementedError(f"{path}: EXR depth is not supported (no OpenEXR reader here); convert the depth to 16-bit PNG")
        poses = self._load_poses(len(color_paths))
        pick = slice(start, len(color_paths) if end == -1 else end, stride)
        self.retained_inds = torch.arange(len(color_paths))[pick]
        self.color_paths, self.depth_paths = color_paths[pick], depth_paths[pick]
        poses = np.stack([np.asarray(p, dtype=np.float64).reshape(4, 4) for p in poses[pick]])
        if relative_pose:
            poses = np.linalg.inv(poses[0])[None] @ poses
            poses[0] = np.eye(4)
        self.poses = torch.from_numpy(poses).to(torch.float32)
        self.transformed_poses = self.poses.to(self.device)
        self._source = _FrameSource(self.color_paths, self.depth_paths, self.device, prefetch)
        self._set_size(desired_height, desired_width)

    def _set_size(self, height, width):
        self.desired_height, self.desired_width = int(height), int(width)
        self.height_downsample_ratio = float(self.desired_height) / self.orig_height
        self.width_downsample_ratio = float(self.desired_width) / self.orig_width
        k = torch.eye(4, dtype=torch.float32)
        k[0, 0], k[1, 1], k[0, 2], k[1, 2] = self.fx, self.fy, self.cx, self.cy
        self.intrinsics = slam.scale_intrinsics(k, self.height_downsample_ratio, self.width_downsample_ratio).to(self.device)

    def _filepaths(self):
        raise NotImplementedError

    def _load_poses(self, num_imgs):
        raise NotImplementedError

    def __len__(self):
        return len(self.color_paths)

    @property
    def stats(self):
        """Counters shared with the ``at_size`` siblings: raw frames fetched, how many of them the read-ahead had decoded or begun,
        seconds in the fetches (``fetch_s`` = ``wait_s`` for the decoded frame + ``upload_s`` for the copy calls + handing out the next
        decodes) and in ``dataset[i]`` altogether (``item_s``, host time: the kernel is only enqueued)."""
        return self._source.stats

    def at_size(self, height, width):
        """A dataset over the same files at another size (its own scaled intrinsics), resampled from the original image as a
        second dataset would; it shares this one's decoded and uploaded frame of the last index fetched."""
        import copy
        other = copy.copy(self)
        other._set_size(height, width)
        return other

    def close(self):
        """Stops the read-ahead threads (the dataset stays usable: frames are then decoded on demand)."""
        self._source.close()

    def __getitem__(self, index):
        index = int(index)
        if index < 0:
            index += len(self)
        if not 0 <= index < len(self):
            raise IndexError(index)
        t0 = time.perf_counter()
        rgb, raw = self._source.raw(index)
        size = (self.desired_height, self.desired_width)
        if self.device.type == "cuda":
            from . import fused
            color, depth = fused.ingest_frame(rgb, raw, self.png_depth_scale, size)
        else:
            color, depth = ingest_frame_cpu(rgb, raw, self.png_depth_scale, size)
        stats = self._source.stats
        stats['items'] += 1
        stats['item_s'] += time.perf_counter() - t0
        return color, depth, self.intrinsics, self.transformed_poses[index]


def _read_trajectory(path, count):
    """One camera-to-world matrix per line, 16 numbers, the first ``count`` lines."""
    with open(path, "r") as f:
        lines = f.readlines()
    if len(lines) < count:
        raise ValueError(f"{path}: {len(lines)} poses for {count} images")
    return [np.array([float(x) for x in lines[i].split()], dtype=np.float64).reshape(4, 4).astype(np.float32) for i in range(count)]


class ReplicaDataset(RGBDDataset):
    """``<basedir>/<sequence>/results/frame*.jpg``, ``results/depth*.png``, ``traj.txt``."""

    def __init__(self, config_dict, basedir, sequence, stride=None, start=0, end=-1, desired_height=480, desired_width=640, **kwargs):
        self.input_folder = os.path.join(basedir, sequence)
        self.pose_path = os.path.join(self.input_folder, "traj.txt")
        super().__init__(config_dict, stride=stride, start=start, end=end, desired_height=desired_height, desired_width=desired_width,
                         **kwargs)

    def _filepaths(self):
        return (natural_sorted(glob.glob(os.path.join(self.input_folder, "results", "frame*.jpg"))),
                natural_sorted(glob.glob(os.path.join(self.input_folder, "results", "depth*.png"))))

    def _load_poses(self, num_imgs):
        return _read_trajectory(self.pose_path, num_imgs)


class ReplicaV2Dataset(RGBDDataset):
    """The train split: ``<basedir>/<sequence>/imap/00/rgb/rgb_*.png``, ``depth/depth_*.png``, ``traj_w_c.txt``.  The held-out split
    (``use_train_split=False``): the first training frame (``imap/00/rgb/rgb_0.png``, ``depth/depth_0.png``, line 0 of its trajectory)
    followed by the frames of ``imap/01`` with the first lines of ``imap/01/traj_w_c.txt``."""

    def __init__(self, config_dict, basedir, sequence, use_train_split=True, stride=None, start=0, end=-1, desired_height=480,
                 desired_width=640, **kwargs):
        self.use_train_split = bool(use_train_split)
        self.train_input_folder = os.path.join(basedir, sequence, "imap", "00")
        self.train_pose_path = os.path.join(self.train_input_folder, "traj_w_c.txt")
        self.input_folder = self.train_input_folder if self.use_train_split else os.path.join(basedir, sequence, "imap", "01")
        self.pose_path = os.path.join(self.input_folder, "traj_w_c.txt")
        if not os.path.isdir(self.input_folder) and not self.use_train_split:
            # (the exception callers of the earlier releases caught for use_train_split=False, kept for a sequence that has no such split)
            raise NotImplementedError(f"{self.input_folder}: this sequence has no held-out split (use_train_split=False reads imap/01)")
        super().__init__(config_dict, stride=stride, start=start, end=end, desired_height=desired_height, desired_width=desired_width,
                         **kwargs)

    def _filepaths(self):
        color = natural_sorted(glob.glob(os.path.join(self.input_folder, "rgb", "rgb_*.png")))
        depth = natural_sorted(glob.glob(os.path.join(self.input_folder, "depth", "depth_*.png")))
        if not self.use_train_split:
            color.insert(0, os.path.join(self.train_input_folder, "rgb", "rgb_0.png"))
            depth.insert(0, os.path.join(self.train_input_folder, "depth", "depth_0.png"))
        return color, depth

    def _load_poses(self, num_imgs):
        if self.use_train_split:
            return _read_trajectory(self.pose_path, num_imgs)
        return _read_trajectory(self.train_pose_path, 1) + _read_trajectory(self.pose_path, num_imgs - 1)


class ScannetDataset(RGBDDataset):
    """``<basedir>/<sequence>/color/*.jpg``, ``depth/*.png`` (a size of its own), ``pose/*.txt`` with a 4 x 4 matrix each."""

    def __init__(self, config_dict, basedir, sequence, stride=None, start=0, end=-1, desired_height=968, desired_width=1296, **kwargs):
        self.input_folder = os.path.join(basedir, sequence)
        super().__init__(config_dict, stride=stride, start=start, end=end, desired_height=desired_height, desired_width=desired_width,
                         **kwargs)

    def _filepaths(self):
        return (natural_sorted(glob.glob(os.path.join(self.input_folder, "color", "*.jpg"))),
                natural_sorted(glob.glob(os.path.join(self.input_folder, "depth", "*.png"))))

    def _load_poses(self, num_imgs):
        return [np.loadtxt(path, dtype=np.float64).reshape(4, 4)
                for path in natural_sorted(glob.glob(os.path.join(self.input_folder, "pose", "*.txt")))]


def _read_list(path, skip_first=False):
    """Rows of a TUM list file split at blanks; '#' starts a comment.  ``skip_first``: the first line is dropped unread (the
    reference reads the pose list that way)."""
    with open(path, "r") as f:
        lines = f.readlines()
    rows = [line.split("#", 1)[0].split() for line in lines[1 if skip_first else 0:]]
    return [row for row in rows if row]


def tum_associate(stamps_image, stamps_depth, stamps_pose, max_dt=0.08, frame_rate=32):
    """(image, depth, pose) index triples: for every colour stamp the nearest depth and pose stamps, kept when both lie closer than
    ``max_dt``; then thinned so that consecutive kept colour stamps are more than 1 / frame_rate apart (the first is always kept)."""
    stamps_depth, stamps_pose = np.asarray(stamps_depth, dtype=np.float64), np.asarray(stamps_pose, dtype=np.float64)
    matched = []
    for i, t in enumerate(np.asarray(stamps_image, dtype=np.float64)):
        j, k = int(np.argmin(np.abs(stamps_depth - t))), int(np.argmin(np.abs(stamps_pose - t)))
        if abs(stamps_depth[j] - t) < max_dt and abs(stamps_pose[k] - t) < max_dt:
            matched.append((i, j, k))
    kept = matched[:1]
    for triple in matched[1:]:
        if stamps_image[triple[0]] - stamps_image[kept[-1][0]] > 1.0 / frame_rate:
            kept.append(triple)
    return kept


class TUMDataset(RGBDDataset):
    """``rgb.txt`` / ``depth.txt`` (stamp, file) and ``groundtruth.txt`` -- ``pose.txt`` when that is absent -- with rows
    ``stamp tx ty tz qx qy qz qw``, associated by nearest stamp."""

    def __init__(self, config_dict, basedir, sequence, stride=None, start=0, end=-1, desired_height=480, desired_width=640, **kwargs):
        self.input_folder = os.path.join(basedir, sequence)
        self._associated = None
        super().__init__(config_dict, stride=stride, start=start, end=end, desired_height=desired_height, desired_width=desired_width,
                         **kwargs)

    def _associate(self):
        if self._associated is None:
            pose_list = os.path.join(self.input_folder, "groundtruth.txt")
            if not os.path.isfile(pose_list):
                pose_list = os.path.join(self.input_folder, "pose.txt")
            if not os.path.isfile(pose_list):
                raise FileNotFoundError(f"{self.input_folder}: neither groundtruth.txt nor pose.txt")
            images = _read_list(os.path.join(self.input_folder, "rgb.txt"))
            depths = _read_list(os.path.join(self.input_folder, "depth.txt"))
            poses = _read_list(pose_list, skip_first=True)
            stamps = [np.array([float(row[0]) for row in rows], dtype=np.float64) for rows in (images, depths, poses)]
            triples = tum_associate(*stamps)
            self._associated = ([os.path.join(self.input_folder, images[i][1]) for i, _, _ in triples],
                                [os.path.join(self.input_folder, depths[j][1]) for _, j, _ in triples],
                                [np.array([float(x) for x in poses[k][1:8]], dtype=np.float64) for _, _, k in triples])
        return self._associated

    def _filepaths(self):
        return self._associate()[0], self._associate()[1]

    def _load_poses(self, num_imgs):
        from scipy.spatial.transform import Rotation
        out = []
        for vec in self._associate()[2]:
            pose = np.eye(4)
            pose[:3, :3] = Rotation.from_quat(vec[3:]).as_matrix()          # (qx, qy, qz, qw)
            pose[:3, 3] = vec[:3]
            out.append(pose.astype(np.float32))
        return out


def _read_json(path):
    import json
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such file")
    with open(path, "r") as f:
        return json.load(f)


class ScannetPPDataset(RGBDDataset):
    """A ScanNet++ scene's DSLR capture, ``<basedir>/<sequence>/dslr/``: ``train_test_lists.json`` (``{"train": [...], "test": [...]}``),
    ``nerfstudio/transforms_undistorted.json`` (``h``, ``w``, ``fl_x``, ``fl_y``, ``cx``, ``cy``; ``frames[]`` for the train names and
    ``test_frames[]`` for the held-out ones, each with ``file_path``, a camera-to-world ``transform_matrix`` in OpenGL axes and
    ``is_bad``), colour in ``undistorted_images/<name>``, depth in ``undistorted_depths/<name with .JPG replaced by .png>`` with 1000
    units per metre.  Frames come in the ORDER OF THE LIST (not sorted); ``ignore_bad`` drops the entries marked ``is_bad``.  Poses are
    ``P @ c2w @ P.T`` with P = diag(1, -1, -1, 1).

    ``use_train_split=False``: item 0 is the first name of the TRAIN list (looked up in ``frames[]``, kept whatever its ``is_bad``
    says), then the test names (looked up in ``test_frames[]``): with ``relative_pose`` every held-out pose is relative to the first
    training frame, the origin of a map built on the train split.  The camera comes from the capture: ``config_dict`` is accepted
    for ``get_dataset`` and not read."""

    def __init__(self, config_dict=None, basedir=None, sequence=None, ignore_bad=False, use_train_split=True, stride=None, start=0,
                 end=-1, desired_height=1168, desired_width=1752, **kwargs):
        self.input_folder = os.path.join(basedir, sequence)
        self.ignore_bad, self.use_train_split = bool(ignore_bad), bool(use_train_split)
        self.lists_path = os.path.join(self.input_folder, "dslr", "train_test_lists.json")
        self.cams_path = os.path.join(self.input_folder, "dslr", "nerfstudio", "transforms_undistorted.json")
        self.train_test_split = _read_json(self.lists_path)
        self.cams_metadata = meta = _read_json(self.cams_path)
        own = {"dataset_name": "scannetpp",
               "camera_params": {"png_depth_scale": 1000.0, "image_height": meta["h"], "image_width": meta["w"],
                                 "fx": meta["fl_x"], "fy": meta["fl_y"], "cx": meta["cx"], "cy": meta["cy"]}}
        super().__init__(own, stride=1 if stride is None else stride, start=start, end=end, desired_height=desired_height,
                         desired_width=desired_width, **kwargs)

    def _entries(self, key):
        return {frame["file_path"]: frame for frame in self.cams_metadata.get(key, [])}

    def _filepaths(self):
        base = os.path.join(self.input_folder, "dslr")
        flip = np.diag([1.0, -1.0, -1.0, 1.0])
        color_paths, depth_paths, self._poses = [], [], []

        def take(name, entries, key, droppable):
            if name not in entries:
                raise ValueError(f"{self.cams_path}: no entry with file_path {name!r} in {key}[] ({len(entries)} listed), "
                                 f"named by {self.lists_path}")
            if droppable and self.ignore_bad and entries[name]["is_bad"]:
                return
            color_paths.append(os.path.join(base, "undistorted_images", name))
            depth_paths.append(os.path.join(base, "undistorted_depths", name.replace(".JPG", ".png")))
            c2w = np.asarray(entries[name]["transform_matrix"], dtype=np.float64).astype(np.float32).astype(np.float64).reshape(4, 4)
            self._poses.append((flip @ c2w @ flip.T).astype(np.float32))

        for split in ("train",) if self.use_train_split else ("train", "test"):
            if split not in self.train_test_split:
                raise ValueError(f"{self.lists_path}: no {split!r} list")
        if self.use_train_split:
            names, entries, key = self.train_test_split["train"], self._entries("frames"), "frames"
        else:
            train = self.train_test_split["train"]
            if not train:
                raise ValueError(f"{self.lists_path}: the train list is empty (its first frame is the origin of the held-out poses)")
            take(train[0], self._entries("frames"), "frames", droppable=False)
            names, entries, key = self.train_test_split["test"], self._entries("test_frames"), "test_frames"
        for name in names:
            take(name, entries, key, droppable=True)
        return color_paths, depth_paths

    def _load_poses(self, num_imgs):
        return self._poses


class NeRFCaptureDataset(RGBDDataset):
    """A capture of the NeRFCapture app as the reference's demo writes it: ``<basedir>/<sequence>/transforms.json`` (``w``, ``h``,
    ``fl_x``, ``fl_y``, ``cx``, ``cy`` and ``frames[]`` with ``file_path`` = ``rgb/<name>`` and a camera-to-world ``transform_matrix``
    in OpenGL axes), the images ``rgb/*`` in natural order, depth as 16-bit PNGs at a size of their own with 6553.5 units per metre.
    The depth path is the colour path below the capture with EVERY occurrence of ``rgb`` replaced by ``depth`` (the reference's
    ``str.replace``: ``rgb/rgb_3.png`` would read ``depth/depth_3.png``).  Poses are ``P @ c2w @ P.T`` with P = diag(1, -1, -1, 1).
    The camera comes from the capture itself: ``config_dict`` is accepted for ``get_dataset`` and not read."""

    def __init__(self, config_dict=None, basedir=None, sequence=None, stride=None, start=0, end=-1, desired_height=1440,
                 desired_width=1920, **kwargs):
        import json
        self.input_folder = os.path.join(basedir, sequence)
        with open(os.path.join(self.input_folder, "transforms.json"), "r") as f:
            self.cams_metadata = json.load(f)
        meta = self.cams_metadata
        own = {"dataset_name": "nerfcapture",
               "camera_params": {"png_depth_scale": 6553.5, "image_height": meta["h"], "image_width": meta["w"],
                                 "fx": meta["fl_x"], "fy": meta["fl_y"], "cx": meta["cx"], "cy": meta["cy"]}}
        super().__init__(own, stride=1 if stride is None else stride, start=start, end=end, desired_height=desired_height,
                         desired_width=desired_width, **kwargs)

    def _filepaths(self):
        by_path = {frame["file_path"]: frame for frame in self.cams_metadata["frames"]}
        flip = np.diag([1.0, -1.0, -1.0, 1.0])
        color_paths, depth_paths, self._poses = [], [], []
        for name in natural_sorted(os.listdir(os.path.join(self.input_folder, "rgb"))):
            name = f"rgb/{name}"
            if name not in by_path:
                raise ValueError(f"{os.path.join(self.input_folder, name)}: no entry with file_path {name!r} in transforms.json "
                                 f"({len(by_path)} frames listed)")
            color_paths.append(os.path.join(self.input_folder, name))
            depth_paths.append(os.path.join(self.input_folder, name.replace("rgb", "depth")))
            c2w = np.asarray(by_path[name]["transform_matrix"], dtype=np.float32).astype(np.float64).reshape(4, 4)
            self._poses.append((flip @ c2w @ flip.T).astype(np.float32))
        return color_paths, depth_paths

    def _load_poses(self, num_imgs):
        return self._poses


_DATASETS = {"replica": ReplicaDataset, "replicav2": ReplicaV2Dataset, "tum": TUMDataset, "scannet": ScannetDataset,
             "scannetpp": ScannetPPDataset, "nerfcapture": NeRFCaptureDataset}


def get_dataset(config_dict, basedir, sequence, **kwargs):
    """The loader for ``config_dict['dataset_name']`` (case-insensitive) over ``<basedir>/<sequence>``."""
    name = str(config_dict["dataset_name"]).lower()
    if name not in _DATASETS:
        raise ValueError(f"Unknown dataset name {config_dict['dataset_name']!r}: supported are {', '.join(SUPPORTED)}")
    return _DATASETS[name](config_dict, basedir, sequence, **kwargs)
