"""The frame path: what a dataset, a decoder or a sensor delivers -> what the loop works on, at the same or at another size.

Three contracts over ONE resampling pass (csrc/frameprep.hip; the arithmetic is csrc/frame_math.h's: colour bilinear on the 0..255
values with pixel centres at half-integers, depth the nearest source pixel -- the rules of the two cv2.resize calls of the reference's
datasets as OpenCV documents them, datasets/gradslam_datasets/basedataset.py:210-257; not checked against OpenCV, which is not
available here):

=================  ==========================================================  ==========================================
on a HIP device    from -> to                                                  the same operations in torch
=================  ==========================================================  ==========================================
``prepare_frame``  dataset frame (float32 colour 0..255 [H, W, 3], depth)      ``prepare_frame_torch`` (``slam.prepare_frame``)
                   -> planes (im [3, h, w] in 0..1, depth [1, h, w])
``ingest_frame``   bytes [H, W, 3] + a depth PNG's uint16 [H', W']             ``ingest_frame_cpu``
                   -> dataset frame (colour [h, w, 3] 0..255, depth [h, w, 1])
``ingest_planes``  bytes + uint16 or float32 depth -> planes, in one launch    ``ingest_planes_cpu``
=================  ==========================================================  ==========================================

``fused``, ``slam`` and ``datasets`` carry these functions under the names their callers use.
"""
import torch

from . import _capi


# ---------------------------------------------------------------------- what both forms check
def _describe(t):
    return f"{t.dtype}, {tuple(t.shape)}, {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__


def _check_sources(color, depth, color_dtype, depth_dtypes, own_depth_size):
    """``color`` [H, W, 3] of ``color_dtype``; ``depth`` of one of ``depth_dtypes`` on the same device, [H', W'] or [H', W', 1] at a
    size of its own, or else any shape of H * W elements.  Returns ((H, W), (H', W'))."""
    if color.dtype != color_dtype or color.dim() != 3 or color.shape[2] != 3 or color.numel() == 0:
        raise RuntimeError(f"color must be a {color_dtype} tensor [H, W, 3] (got {_describe(color)})")
    H, W = int(color.shape[0]), int(color.shape[1])
    ok = isinstance(depth, torch.Tensor) and depth.dtype in depth_dtypes and depth.device == color.device
    if own_depth_size:
        if not (ok and depth.numel() > 0 and (depth.dim() == 2 or (depth.dim() == 3 and depth.shape[2] == 1))):
            raise RuntimeError(f"depth must be a {' or '.join(map(str, depth_dtypes))} tensor [H, W] or [H, W, 1] on {color.device} (got {_describe(depth)})")
        return (H, W), (int(depth.shape[0]), int(depth.shape[1]))
    if not (ok and depth.numel() == H * W):
        raise RuntimeError(f"depth must be a {depth_dtypes[0]} tensor of {H * W} elements on {color.device} (got {_describe(depth)})")
    return (H, W), (H, W)


def _out_size(size, default):
    h, w = default if size is None else (int(size[0]), int(size[1]))
    if h <= 0 or w <= 0:
        raise RuntimeError(f"size must be positive (got {(h, w)})")
    return h, w


def _positive_scale(png_depth_scale):
    if not float(png_depth_scale) > 0.0:
        raise RuntimeError(f"png_depth_scale must be positive (got {png_depth_scale})")
    return float(png_depth_scale)


def _depth_kind(dtype, depth_scale):
    """(SPLAT_DEPTH_*, divisor) of a raw depth image: float32 is metres already, uint16 needs its divisor."""
    if dtype == torch.float32:
        if depth_scale is not None and float(depth_scale) != 1.0:
            raise RuntimeError(f"float32 depth is in metres already: depth_scale must be None or 1 (got {depth_scale})")
        return _capi.SPLAT_DEPTH_F32, 1.0
    if depth_scale is None or not float(depth_scale) > 0.0:
        raise RuntimeError(f"uint16 depth needs a positive depth_scale (got {depth_scale})")
    return _capi.SPLAT_DEPTH_U16, float(depth_scale)


# ---------------------------------------------------------------------- the HIP entries (csrc/frameprep.hip)
def _launch(symbol, torch_form, color, depth, color_dtype, depth_dtypes, own_depth_size, scalars, size, out, planes):
    """Checks the sources, ``size`` and ``out`` and launches ``symbol`` on the current stream of the sources' device:
    ``symbol(W, H, color, [W', H',] depth, *scalars(depth.dtype), w, h, out[0], out[1], stream)``; the outputs are the loop's ``planes``
    or a dataset's interleaved frame.  Nothing is read back."""
    if not isinstance(color, torch.Tensor) or color.device.type != "cuda":
        raise RuntimeError(f"{symbol} needs CUDA/HIP tensors; the HIP library has no CPU path ({torch_form} is the torch form)")
    dev = color.device
    (H, W), (zH, zW) = _check_sources(color, depth, color_dtype, depth_dtypes, own_depth_size)
    middle = scalars(depth.dtype)
    h, w = _out_size(size, (H, W))
    color, depth = color.contiguous(), depth.contiguous()
    shapes = ((3, h, w), (1, h, w)) if planes else ((h, w, 3), (h, w, 1))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in shapes)
    for name, t, shape in zip(("out[0]", "out[1]"), out, shapes):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == shape and t.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous float32 tensor of shape {shape} on {dev}")
    with torch.cuda.device(dev):
        _capi.check(getattr(_capi.lib(), symbol)(W, H, color.data_ptr(), *((zW, zH) if own_depth_size else ()), depth.data_ptr(), *middle, w, h,
                                                 out[0].data_ptr(), out[1].data_ptr(), torch.cuda.current_stream(dev).cuda_stream), symbol)
    return out[0], out[1]


def prepare_frame(color, depth, size=None, out=None):
    """A frame as the datasets hand it over -- ``color`` [H, W, 3] in 0..255, ``depth`` [H, W, 1] (or [H, W]), float32 on one
    CUDA/HIP device -- as every entry of ``fused`` takes it: ``(im [3, h, w] in 0..1, depth [1, h, w])`` at ``size = (h, w)``
    (default: the frame's own size, i.e. the loop's ``permute(2, 0, 1) / 255``).  At another size colour is resampled bilinearly
    and depth by nearest source pixel (include/splat_hip.h splat_frame_prepare).  One launch on the current stream, nothing read
    back.  ``out = (im, depth)``: contiguous float32 tensors of those shapes to write into (views into larger buffers are fine);
    otherwise two new tensors."""
    return _launch("splat_frame_prepare", "slam.prepare_frame", color, depth, torch.float32, (torch.float32,), False, lambda dtype: (),
                   size, out, planes=True)


def ingest_frame(rgb_u8, depth_u16, png_depth_scale, size=None, out=None):
    """What an image decoder leaves -- ``rgb_u8`` [H, W, 3] uint8 and ``depth_u16`` [H', W'] (or [H', W', 1]) uint16, the integers
    of a depth PNG, on one CUDA/HIP device; the two sizes may differ -- as the frame a dataset hands over: ``(color [h, w, 3] float32
    in 0..255, depth [h, w, 1] float32 in metres)`` at ``size = (h, w)`` (default: the colour image's size).  Colour is resampled
    bilinearly on the byte values (exactly the bytes at equal size), depth is the nearest source pixel as
    ``float32(float64(raw) / png_depth_scale)`` (include/splat_hip.h splat_frame_ingest).  ``out = (color, depth)`` as for
    ``prepare_frame``."""
    return _launch("splat_frame_ingest", "datasets.ingest_frame_cpu", rgb_u8, depth_u16, torch.uint8, (torch.uint16,), True,
                   lambda dtype: (_positive_scale(png_depth_scale),), size, out, planes=False)


def ingest_planes(rgb_u8, depth_raw, depth_scale=None, size=None, out=None):
    """What a sensor or a decoder delivers -- ``rgb_u8`` [H, W, 3] uint8 and ``depth_raw`` [H', W'] (or [H', W', 1]), float32 metres
    (``depth_scale`` None or 1) or uint16 integers with their divisor ``depth_scale``, on one CUDA/HIP device; the depth image has a
    size of its own and may be smaller than the output -- as the planes the loop works on: ``(im [3, h, w] in 0..1, depth [1, h, w] in
    metres)`` at ``size = (h, w)`` (default: the colour image's size).  One launch (include/splat_hip.h splat_frame_ingest_planes),
    bit-equal to ``prepare_frame(*ingest_frame(...))`` without the frame in between; a float32 depth is copied bit for bit.
    ``out = (im, depth)`` as for ``prepare_frame``."""
    return _launch("splat_frame_ingest_planes", "datasets.ingest_planes_cpu", rgb_u8, depth_raw, torch.uint8, (torch.uint16, torch.float32), True,
                   lambda dtype: _depth_kind(dtype, depth_scale), size, out, planes=True)


# ---------------------------------------------------------------------- the torch forms: the kernel's operations in the kernel's order
def _linear_taps(dst, src, device):
    """Per destination index along one axis: the two source indices and the weight of the second (csrc/frame_math.h
    frame_linear_tap: f = (d + 0.5) * (src / dst) - 0.5 in double, clamped to the row with weight 0)."""
    f = (torch.arange(dst, dtype=torch.float64) + 0.5) * (float(src) / float(dst)) - 0.5
    fl = torch.floor(f)
    s, w = fl.to(torch.int64), (f - fl).to(torch.float32)
    out = (s < 0) | (s >= src - 1)
    s = s.clamp(0, src - 1)
    w = torch.where(out, torch.zeros_like(w), w)
    return s.to(device), (s + 1).clamp(max=src - 1).to(device), w.to(device)


def _nearest_index(dst, src, device):
    """csrc/frame_math.h frame_nearest_index: min(floor(d * (1 / (dst / src))), src - 1), in double."""
    inv = 1.0 / (float(dst) / float(src))
    return torch.floor(torch.arange(dst, dtype=torch.float64) * inv).to(torch.int64).clamp(max=src - 1).to(device)


def _blend(color, size):
    """csrc/frame_math.h frame_blend: [H, W, 3] in 0..255 -> float32 [h, w, 3] in 0..255, along x on both rows, then along y."""
    H, W = int(color.shape[0]), int(color.shape[1])
    h, w = size
    c = color.to(torch.float32)
    y0, y1, wy = _linear_taps(h, H, c.device)
    x0, x1, wx = _linear_taps(w, W, c.device)
    wx, wy = wx.view(1, w, 1), wy.view(h, 1, 1)
    r0, r1 = c[y0], c[y1]
    top = r0[:, x0] + wx * (r0[:, x1] - r0[:, x0])
    bottom = r1[:, x0] + wx * (r1[:, x1] - r1[:, x0])
    return top + wy * (bottom - top)


def _nearest(depth, size):
    """[H', W'] -> [h, w]: the nearest source pixel, a plain gather."""
    zH, zW = int(depth.shape[0]), int(depth.shape[1])
    return depth.reshape(zH, zW)[_nearest_index(size[0], zH, depth.device)][:, _nearest_index(size[1], zW, depth.device)]


def prepare_frame_torch(color, depth, size=None):
    """``prepare_frame`` in torch on any device, float32: the CPU / drop-in path of the frame loop.  ``color`` [H, W, 3] in 0..255,
    ``depth`` [H, W, 1] -> ``(im [3, h, w] in 0..1, depth [1, h, w])``: the blend, then ONE division by 255."""
    H, W = int(color.shape[0]), int(color.shape[1])
    h, w = (H, W) if size is None else (int(size[0]), int(size[1]))
    im = (_blend(color, (h, w)) / 255.0).permute(2, 0, 1).contiguous()
    return im, _nearest(depth.to(torch.float32).reshape(H, W), (h, w)).reshape(1, h, w).contiguous()


def ingest_frame_cpu(rgb_u8, depth_u16, png_depth_scale, size=None):
    """``ingest_frame`` in torch on the host: colour blended in float32, depth the nearest source pixel as
    ``float32(float64(raw) / png_depth_scale)``.  Arrays or CPU tensors in (uint8 [H, W, 3], uint16 [H', W']), tensors out:
    ``(color [h, w, 3] float32 in 0..255, depth [h, w, 1] float32)``."""
    rgb, raw = torch.as_tensor(rgb_u8), torch.as_tensor(depth_u16)
    h, w = (int(rgb.shape[0]), int(rgb.shape[1])) if size is None else (int(size[0]), int(size[1]))
    depth = (_nearest(raw.to(torch.int32), (h, w)).to(torch.float64) / float(png_depth_scale)).to(torch.float32)
    return _blend(rgb, (h, w)), depth.reshape(h, w, 1)


def ingest_planes_cpu(rgb_u8, depth_raw, depth_scale=None, size=None):
    """``ingest_planes`` in torch on the host: the blend on the bytes, one float32 division by 255, planar; depth the nearest source
    pixel -- a uint16 as ``float32(float64(raw) / depth_scale)``, a float32 copied bit for bit (it is gathered as int32, so NaN
    payloads survive; ``depth_scale`` must then be None or 1).  Arrays or CPU tensors in (uint8 [H, W, 3]; uint16 or float32 [H', W']
    or [H', W', 1]), tensors out: ``(im [3, h, w] float32 in 0..1, depth [1, h, w] float32)``."""
    rgb, raw = torch.as_tensor(rgb_u8), torch.as_tensor(depth_raw)
    (H, W), _ = _check_sources(rgb, raw, torch.uint8, (torch.uint16, torch.float32), True)
    kind, scale = _depth_kind(raw.dtype, depth_scale)
    h, w = _out_size(size, (H, W))
    if kind == _capi.SPLAT_DEPTH_F32:
        color, depth = _blend(rgb, (h, w)), _nearest(raw.contiguous().view(torch.int32), (h, w)).contiguous().view(torch.float32)
    else:
        color, depth = ingest_frame_cpu(rgb, raw, scale, size=(h, w))
    return (color / 255.0).permute(2, 0, 1).contiguous(), depth.reshape(1, h, w)
