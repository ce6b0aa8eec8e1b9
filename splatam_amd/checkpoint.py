"""The files of a checkpoint, the random streams of the frame loop, and the thread that writes.

Two kinds of checkpoint (INTEGRATION.md "Checkpoints"):

=============================================  =============================================
here                                           reference
=============================================  =============================================
``reference_paths`` / ``write_reference``      scripts/splatam.py:927-931 + utils/common_utils.py:45-52 (``params<t>.npz``: every
                                               entry of ``params``; ``keyframe_time_indices<t>.npy``)
``load_reference``                             scripts/splatam.py:608-617 (the two files read back)
``session<t>.npz`` / ``keyframes<t>.npz``      -- (the exact checkpoint of ``SlamSession.save_checkpoint``; no counterpart)
=============================================  =============================================

Nothing here is pickled: every entry of the two files of this package's own is a numeric array or a JSON string, and they are read
with ``allow_pickle=False``.
"""
from __future__ import annotations

import json
import os
import random
import threading

import numpy as np
import torch

FORMAT = 1
MAP_KEYS = ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales', 'cam_unnorm_rots', 'cam_trans')


def reference_paths(directory, time_idx):
    """(``params<t>.npz``, ``keyframe_time_indices<t>.npy``) under ``directory``: the reference's names."""
    return os.path.join(directory, f"params{time_idx}.npz"), os.path.join(directory, f"keyframe_time_indices{time_idx}.npy")


def session_path(directory, time_idx):
    return os.path.join(directory, f"session{time_idx}.npz")


def keyframes_path(directory, time_idx):
    return os.path.join(directory, f"keyframes{time_idx}.npz")


def default_directory(config):
    """``workdir/run_name`` where the config has both (scripts/splatam.py:929), else None."""
    if config.get('workdir') is not None and config.get('run_name') is not None:
        return os.path.join(config['workdir'], config['run_name'])
    return None


def _write_npz(path, arrays):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".part"
    with open(tmp, "wb") as f:                  # (a file object: savez keeps the name as it is)
        np.savez(f, **arrays)
    os.replace(tmp, path)                       # a reader never sees half a file
    return os.path.getsize(path)


def _write_npy(path, array):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".part"
    with open(tmp, "wb") as f:
        np.save(f, array)
    os.replace(tmp, path)
    return os.path.getsize(path)


def write_reference(directory, time_idx, params, keyframe_time_indices):
    """The pair of files the reference writes; ``params``: host arrays by name.  Returns the bytes written."""
    p_path, k_path = reference_paths(directory, time_idx)
    return _write_npz(p_path, {k: params[k] for k in params}) + _write_npy(k_path, np.array(keyframe_time_indices))


def _need(path):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"checkpoint file {path} does not exist")
    return path


def load_reference(directory, time_idx, device):
    """``(params, keyframe_time_indices)`` of the reference's pair of files, the parameters as its loader makes them
    (scripts/splatam.py:609-610: float32 on the device, ``requires_grad``), the list as ``tolist()`` gives it."""
    p_path, k_path = reference_paths(directory, time_idx)
    with np.load(_need(p_path), allow_pickle=False) as z:
        params = {k: torch.tensor(z[k]).to(device).float().requires_grad_(True) for k in z.files}
    return params, np.load(_need(k_path), allow_pickle=False).tolist()


def load_session(directory, time_idx):
    """``(arrays, meta)`` of ``session<t>.npz``."""
    with np.load(_need(session_path(directory, time_idx)), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    meta = json.loads(str(arrays.pop('meta')))
    if meta.get('format') != FORMAT:
        raise ValueError(f"{session_path(directory, time_idx)}: format {meta.get('format')!r}, this package reads format {FORMAT}")
    return arrays, meta


def load_keyframes(directory, time_idx):
    """The planes of ``keyframes<t>.npz`` as ``[(colour [3, H, W], depth [1, H, W])]`` in keyframe-list order, or None without the file."""
    path = keyframes_path(directory, time_idx)
    if not os.path.isfile(path):
        return None
    with np.load(path, allow_pickle=False) as z:
        n = int(z['count'])
        return [(z[f"color{i}"], z[f"depth{i}"]) for i in range(n)]


# ----------------------------------------------------------------------------------------------------------------------------------
# the random streams the loop draws from
# ----------------------------------------------------------------------------------------------------------------------------------

def capture_random(dev):
    """``(arrays, meta)``: Python's ``random`` (nothing in the loop draws from it today; the reference seeds it, so it is kept), numpy's
    global generator (``np.random.randint`` in the mapping iterations, ``permutation`` in keyframe selection), torch's CPU generator
    (``randint`` in keyframe selection) and the generator of the device.  Host state only: nothing is launched or synchronised."""
    version, words, gauss = random.getstate()
    name, keys, pos, has_gauss, cached = np.random.get_state()
    arrays = {'rng/python': np.array(words, dtype=np.uint64), 'rng/numpy': np.array(keys, dtype=np.uint32),
              'rng/torch_cpu': torch.get_rng_state().numpy().copy()}
    if dev.type == "cuda":
        arrays['rng/torch_device'] = torch.cuda.get_rng_state(dev).numpy().copy()
    return arrays, dict(python=[version, gauss], numpy=[name, int(pos), int(has_gauss), float(cached)])


def restore_random(arrays, meta, dev):
    version, gauss = meta['python']
    random.setstate((int(version), tuple(int(x) for x in arrays['rng/python']), gauss))
    name, pos, has_gauss, cached = meta['numpy']
    np.random.set_state((name, arrays['rng/numpy'].astype(np.uint32), int(pos), int(has_gauss), float(cached)))
    torch.set_rng_state(torch.from_numpy(arrays['rng/torch_cpu'].copy()))
    if dev.type == "cuda" and 'rng/torch_device' in arrays:
        torch.cuda.set_rng_state(torch.from_numpy(arrays['rng/torch_device'].copy()), dev)


# ----------------------------------------------------------------------------------------------------------------------------------
# device -> host, and the writer
# ----------------------------------------------------------------------------------------------------------------------------------

class HostCopies:
    """Host copies of device tensors for a checkpoint: pinned buffers kept by name and reused while they fit (a map grows: 25 %
    headroom), filled with non-blocking copies; ``wait()`` is the checkpoint's ONE synchronisation.  On the CPU the copies are clones
    (the loop edits its tensors in place while the writer thread still reads)."""

    def __init__(self, dev):
        self.dev, self._pinned = dev, {}

    def copy(self, name, t, keep=False):
        """numpy view of a host copy of ``t``; valid after ``wait()`` and until the next ``copy`` under the same name (``keep``: for good,
        in a buffer of its own)."""
        t = t.detach()
        if t.device.type != "cuda":
            return t.clone().contiguous().numpy()
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        flat = None if keep else self._pinned.get(name)
        if flat is None or flat.numel() < nbytes:
            flat = torch.empty(max(nbytes if keep else nbytes + nbytes // 4, 16), dtype=torch.uint8, pin_memory=True)
            if not keep:
                self._pinned[name] = flat
        host = flat[:nbytes].view(t.dtype).view(t.shape)
        host.copy_(t, non_blocking=True)
        return host.numpy()

    def wait(self):
        if self.dev.type == "cuda":
            torch.cuda.current_stream(self.dev).synchronize()


class Writer:
    """One background thread at a time writes a checkpoint's files; ``join()`` waits for it and raises what it raised."""

    def __init__(self):
        self._thread, self._error, self.bytes_written = None, None, {}

    def submit(self, jobs):
        """``jobs``: [(label, callable returning the bytes written)], run in order on a fresh thread (``join()`` first)."""
        self.join()

        def work():
            try:
                for label, job in jobs:
                    self.bytes_written[label] = job()
            except BaseException as e:             # noqa: B902  (handed to the thread that joins)
                self._error = e
        self.bytes_written = {}
        self._thread = threading.Thread(target=work, name="splatam-checkpoint-writer", daemon=False)
        self._thread.start()

    def join(self):
        thread, self._thread = self._thread, None
        if thread is not None:
            thread.join()
        error, self._error = self._error, None
        if error is not None:
            raise RuntimeError(f"writing a checkpoint failed: {error}") from error
