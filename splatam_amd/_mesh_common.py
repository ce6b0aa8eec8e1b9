"""What the wrappers of the mesh layers (``mesh_render``, ``mesh_view``, ``mesh_score``, ``mesh_clean``) share, one definition each: the
stream and device of a call, the check of a tensor argument, and how a mesh, a transform and a pose are read."""
from __future__ import annotations

import os

import numpy as np
import torch


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _on_device(dev, what):
    """Refuses a ``dev`` that is no CUDA/HIP device in the name of ``what``."""
    if dev.type != "cuda":
        raise RuntimeError(f"{what} needs a CUDA/HIP device; the HIP library has no CPU path")


def _device(device, what):
    dev = torch.device(device)
    _on_device(dev, what)
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _ptr(t, n=True):
    """The address of ``t``, or None for the array of a count ``n`` of zero (the library wants NULL there)."""
    return t.data_ptr() if n else None


_DTYPES = {torch.float32: "float32", torch.float64: "float64", torch.int32: "int32", torch.int64: "int64"}


def _tensor(t, name, dtype, shape, dev, contiguous=False):
    """``t``, which must be a ``dtype`` tensor of ``shape`` on ``dev`` -- a letter in ``shape`` stands for any size; an int instead of a
    tuple asks for that many elements in any shape, which are then contiguous."""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and (not contiguous or t.is_contiguous())
    if isinstance(shape, int):
        ok = ok and t.numel() == shape and t.is_contiguous()
        form = f"{shape} contiguous {_DTYPES[dtype]}"
    else:
        ok = ok and t.dim() == len(shape) and all(isinstance(s, str) or t.shape[k] == s for k, s in enumerate(shape))
        words = ("contiguous " if contiguous else "") + _DTYPES[dtype]
        form = f"{'an' if words[0] in 'aeiou' else 'a'} {words} tensor [{', '.join(str(s) for s in shape)}]"
    if not ok:
        raise RuntimeError(f"{name} must be {form} on {dev}")
    return t


def _mesh_arrays(vertices, faces, dev):
    return _tensor(vertices, "vertices", torch.float32, ("V", 3), dev).contiguous(), _tensor(faces, "faces", torch.int32, ("F", 3), dev).contiguous()


def _loaded(mesh):
    """``mesh``, read from disk where it is the path of a PLY."""
    if isinstance(mesh, (str, os.PathLike)):
        from .export import load_mesh_ply
        mesh = load_mesh_ply(mesh)
    return mesh


def _transform(transform):
    """``transform`` as a finite 4 x 4 float64 array, or None."""
    if transform is None:
        return None
    m = np.asarray(transform.detach().cpu() if isinstance(transform, torch.Tensor) else transform, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError("transform must be a finite 4 x 4 matrix")
    return m


def _pose_tensor(w2c):
    """One or many poses as a tensor: a tensor stays what and where it is; host values become float32 on the host, rounded ONCE, from
    float64."""
    if isinstance(w2c, torch.Tensor):
        return w2c.detach()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(w2c, dtype=np.float64).astype(np.float32)))
