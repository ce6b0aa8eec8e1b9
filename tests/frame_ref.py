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


GUARD = 12345.0


def run_guarded(entry, inputs, shapes, lead):
    """``entry(*device inputs, out=(a, b))`` with both outputs as views inside ONE flat float32 buffer
    [lead guards | a | 8 guards | b | 64 guards], on a side stream: lead 64 puts the views on a 16-byte boundary, lead 61 off it, so a
    width divisible by 4 meets the 16-byte and the scalar stores.  The guards must stay as they were.  Returns the two outputs on the
    host in ``shapes``."""
    import torch
    dev = torch.device("cuda")
    n, m = int(np.prod(shapes[0])), int(np.prod(shapes[1]))
    flat = torch.full((lead + n + 8 + m + 64,), GUARD, dtype=torch.float32, device=dev)
    a, b = flat[lead:lead + n].view(shapes[0]), flat[lead + n + 8:lead + n + 8 + m].view(shapes[1])
    src = [torch.from_numpy(x).to(dev) for x in inputs]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = entry(*src, out=(a, b))
    stream.synchronize()
    assert got[0].data_ptr() == a.data_ptr() and got[1].data_ptr() == b.data_ptr()
    host = flat.cpu().numpy()
    guards = np.concatenate([host[:lead], host[lead + n:lead + n + 8], host[lead + n + 8 + m:]])
    assert np.all(guards == np.float32(GUARD)), "a store left the output views"
    return host[lead:lead + n].reshape(shapes[0]), host[lead + n + 8:lead + n + 8 + m].reshape(shapes[1])


def seeded_raw(cw, ch, zw, zh, seed):
    """(rgb [ch, cw, 3] uint8, raw [zh, zw] uint16 with some zeros): what a decoder leaves."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, size=(ch, cw, 3), dtype=np.uint8)
    raw = rng.integers(0, 65536, size=(zh, zw)).astype(np.uint16)
    raw[rng.random((zh, zw)) < 0.1] = 0
    return rgb, raw


def special_floats(zw, zh, seed):
    """float32 depth with 0, -0, -1, +inf, -inf, a NaN whose payload is not the default one, the smallest and the largest denormal."""
    rng = np.random.default_rng(seed)
    bits = (0.5 + 4.0 * rng.random((zh, zw))).astype(np.float32).view(np.uint32).reshape(-1).copy()
    special = np.array([0x00000000, 0x80000000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FA12345, 0xFFC00001, 0x00000001, 0x007FFFFF, 0x80000123],
                       dtype=np.uint32)
    where = rng.permutation(bits.size)[:special.size]
    bits[where] = special[:where.size]
    return bits.reshape(zh, zw).view(np.float32)


# ((colour w, h), (depth w, h), (destination w, h)): every SIZES pair with the depth at the colour's size and at a size of its own ...
OTHER_DEPTH = (11, 7)
RAW_CASES = (tuple((s, s, d) for s, d in SIZES) + tuple((s, OTHER_DEPTH, d) for s, d in SIZES)
             + (((26, 20), (16, 12), (13, 9)),          # a depth image of a size of its own, both reduced
                ((24, 16), (5, 3), (24, 16)),           # depth upsampled under an identity colour
                ((1, 1), (1, 1), (4, 3)), ((1, 1), (3, 2), (4, 3))))
GOLDEN_SCALE = 6553.5


def golden_frame_kernel_runs(fused, lead):
    """Every (key, im or colour, depth) that tests/golden/frame_kernels_reference.npz records, run now at ``lead``: the three entry
    points over SIZES / RAW_CASES with the seeds of their own tests, uint16 depth at 6553.5 and the special-float depth."""
    for i, ((sw, sh), (dw, dh)) in enumerate(SIZES):
        color, depth = seeded_frame(sw, sh, seed=sw * 100 + dw, integer=False)
        planes = ((3, dh, dw), (1, dh, dw))
        yield (f"prepare/{i}",) + run_guarded(lambda c, z, out: fused.prepare_frame(c, z, size=(dh, dw), out=out), (color, depth), planes, lead)
        yield (f"prepare_special/{i}",) + run_guarded(lambda c, z, out: fused.prepare_frame(c, z, size=(dh, dw), out=out),
                                                      (color, special_floats(sw, sh, seed=sw * 10 + dw)), planes, lead)
    for i, ((cw, ch), (zw, zh), (dw, dh)) in enumerate(RAW_CASES):
        rgb, raw = seeded_raw(cw, ch, zw, zh, seed=cw * 100 + dw)
        planes = ((3, dh, dw), (1, dh, dw))
        yield (f"ingest/{i}",) + run_guarded(lambda c, z, out: fused.ingest_frame(c, z, GOLDEN_SCALE, size=(dh, dw), out=out), (rgb, raw),
                                             ((dh, dw, 3), (dh, dw, 1)), lead)
        yield (f"planes_u16/{i}",) + run_guarded(lambda c, z, out: fused.ingest_planes(c, z, GOLDEN_SCALE, size=(dh, dw), out=out), (rgb, raw),
                                                 planes, lead)
        yield (f"planes_f32/{i}",) + run_guarded(lambda c, z, out: fused.ingest_planes(c, z, None, size=(dh, dw), out=out),
                                                 (rgb, special_floats(zw, zh, seed=zw * 10 + dw)), planes, lead)
