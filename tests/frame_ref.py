"""Float64 numpy restatement of frame preparation (splatam_amd/csrc/frame_math.h), shared by the frame-preparation tests and by
tests/golden/make_golden_loop_multires.py, where it stands in for the two cv2.resize calls of the reference's datasets
(/root/reference/datasets/gradslam_datasets/basedataset.py:210-257).

TEST INFRASTRUCTURE.  It states OpenCV's DOCUMENTED rules and is not pinned against OpenCV (not installed here):
  colour  INTER_LINEAR on the 0..255 values: per axis f = (d + 0.5) * (src / dst) - 0.5, s = floor(f), weight f - s;
          s < 0 -> s = 0, weight 0; s >= src - 1 -> s = src - 1, weight 0;
  depth   INTER_NEAREST: s = min(floor(d * (1.0 / (double(dst) / src))), src - 1), a plain copy.
Everything in float64; nothing is divided by 255 here (``prepare`` does, in float64, for the tolerance tests; the bit-exact tests
divide ``float32(resize_linear)`` by ``float32(255)`` themselves)."""
import numpy as np

# (source width, height) -> (destination width, height): 2:1; a non-integer ratio with odd tails; identity; 3:1 (the double-rounded
# nearest index); an upscale (both clamp branches of the linear taps)
# ... and a non-integer ratio at a destination width that is a multiple of 4 (the kernel's 16-byte stores away from the exact 2:1 case)
SIZES = (((40, 24), (20, 12)), ((37, 23), (18, 11)), ((37, 23), (37, 23)), ((39, 24), (13, 8)), ((8, 6), (13, 7)), ((37, 23), (20, 11)))
EXACT = (((40, 24), (20, 12)), ((37, 23), (37, 23)))        # integer inputs: every blend is exact in float32


def linear_taps(dst, src):
    f = (np.arange(dst, dtype=np.float64) + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5
    s = np.floor(f)
    w = f - s
    s = s.astype(np.int64)
    w[s < 0] = 0.0
    s[s < 0] = 0
    w[s >= src - 1] = 0.0
    s[s >= src - 1] = src - 1
    return s, np.minimum(s + 1, src - 1), w


def nearest_index(dst, src):
    inv = 1.0 / (np.float64(dst) / np.float64(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * inv).astype(np.int64), src - 1)


def resize_linear(color, h, w):
    """color [H, W, C] (any range) -> [h, w, C], float64."""
    c = np.asarray(color, dtype=np.float64)
    y0, y1, wy = linear_taps(h, c.shape[0])
    x0, x1, wx = linear_taps(w, c.shape[1])
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = c[y0][:, x0] * (1.0 - wx) + c[y0][:, x1] * wx
    bottom = c[y1][:, x0] * (1.0 - wx) + c[y1][:, x1] * wx
    return top * (1.0 - wy) + bottom * wy


def resize_nearest(depth, h, w):
    """depth [H, W] or [H, W, 1] -> the same rank at [h, w]; values copied."""
    d = np.asarray(depth)
    return d[nearest_index(h, d.shape[0])][:, nearest_index(w, d.shape[1])]


def prepare(color, depth, h, w):
    """(im [3, h, w] in 0..1 as float64, depth [1, h, w] in depth's dtype)."""
    im = resize_linear(color, h, w).transpose(2, 0, 1) / 255.0
    return im, resize_nearest(np.asarray(depth).reshape(depth.shape[0], depth.shape[1]), h, w)[None]


def scale_intrinsics(k, h_ratio, w_ratio):
    out = np.array(k, dtype=np.float32, copy=True)
    out[..., 0, 0] *= w_ratio
    out[..., 1, 1] *= h_ratio
    out[..., 0, 2] *= w_ratio
    out[..., 1, 2] *= h_ratio
    return out


def seeded_frame(sw, sh, seed, integer):
    """(color [sh, sw, 3] float32 in 0..255, depth [sh, sw, 1] float32 with some zeros): integer-valued colours or not."""
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=(sh, sw, 3)).astype(np.float32) if integer else (rng.random((sh, sw, 3)) * 255.0).astype(np.float32)
    depth = (0.5 + 4.0 * rng.random((sh, sw, 1))).astype(np.float32)
    depth[rng.random((sh, sw, 1)) < 0.1] = 0.0
    return color, depth
