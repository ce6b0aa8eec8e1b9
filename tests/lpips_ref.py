"""LPIPS (AlexNet taps) restated in float64 numpy for the tests: explicit patch gather + ``einsum`` (no ``conv2d``: it shares no code
with ``splatam_amd.slam.lpips``), the max-pool, the channel norms and the distance exactly as splatam_amd/lpips.py states them.

Besides every tap it returns, per output element, S = sum_k |a_k b_k| + |bias|: the scale float32 summation error is measured in."""
import numpy as np

SHIFT = np.array([-0.030, -0.088, -0.188])
SCALE = np.array([0.458, 0.448, 0.450])
# stride, padding, pool in front
GEOMETRY = ((4, 2, False), (1, 2, True), (1, 1, True), (1, 1, False), (1, 1, False))


def weights64(weights):
    """(conv weights, biases, lins) of an ``LpipsWeights`` as float64 arrays."""
    return ([w.numpy().astype(np.float64) for w in weights.conv_weight], [b.numpy().astype(np.float64) for b in weights.conv_bias],
            [v.numpy().astype(np.float64) for v in weights.lin])


def patches(x, k, stride, pad):
    """x [B, C, H, W] -> [B, C, k, k, Ho, Wo], zero padding."""
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.zeros((B, C, H + 2 * pad, W + 2 * pad), dtype=np.float64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    out = np.empty((B, C, k, k, Ho, Wo), dtype=np.float64)
    for dy in range(k):
        for dx in range(k):
            out[:, :, dy, dx] = xp[:, :, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride]
    return out


def conv_relu(x, w, b, stride, pad):
    """(relu(conv(x) + b), S) for x [B, Cin, H, W] float64, w [Cout, Cin, k, k], b [Cout]."""
    p = patches(np.asarray(x, dtype=np.float64), w.shape[2], stride, pad)
    y = np.einsum('bcyxhw,ocyx->bohw', p, w, optimize=True) + b[None, :, None, None]
    S = np.einsum('bcyxhw,ocyx->bohw', np.abs(p), np.abs(w), optimize=True) + np.abs(b)[None, :, None, None]
    return np.maximum(y, 0.0), S


def max_pool(x):
    """3 x 3, stride 2, no padding, floor."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = np.full((B, C, Ho, Wo), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, x[:, :, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2])
    return out


def transform(x):
    """[..., 3, H, W] in any range -> the network's input."""
    x = np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0)
    return ((2.0 * x - 1.0) - SHIFT[:, None, None]) / SCALE[:, None, None]


def taps(x, weights):
    """x [B, 3, H, W] (images in 0..1) -> (five taps [B, C_l, H_l, W_l], five S of the same shapes, the five layer INPUTS)."""
    cw, cb, _ = weights64(weights)
    x = transform(x)
    out, scales, inputs = [], [], []
    for l, (stride, pad, pool) in enumerate(GEOMETRY):
        if pool:
            x = max_pool(x)
        inputs.append(x)
        x, S = conv_relu(x, cw[l], cb[l], stride, pad)
        out.append(x)
        scales.append(S)
    return out, scales, inputs


def distance(feats, weights):
    """feats: five [2, C_l, H_l, W_l]; sum over the taps of mean over pixels of sum_c w_c (u0_c - u1_c)^2."""
    _, _, lins = weights64(weights)
    total = 0.0
    for f, w in zip(feats, lins):
        u = f / (np.sqrt((f * f).sum(axis=1, keepdims=True)) + 1e-10)
        total += float((w[None, :, None, None] * (u[0:1] - u[1:2]) ** 2).sum(axis=1).mean())
    return total


def lpips(im0, im1, weights):
    """(value, taps, S, layer inputs) of two images [3, H, W]."""
    f, S, inputs = taps(np.stack([np.asarray(im0, dtype=np.float64), np.asarray(im1, dtype=np.float64)]), weights)
    return distance(f, weights), f, S, inputs


def image_pair(W, H, seed):
    """Two float32 images [3, H, W] in 0..1 that differ by smooth structure plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (a * xx + b * yy) + c) for a, b, c in rng.uniform(0.5, 4.0, size=(3, 3))])
    a = np.clip(base + 0.08 * rng.standard_normal(base.shape), 0, 1)
    b = np.clip(base + 0.1 * np.cos(2 * np.pi * (3 * xx - 2 * yy))[None] + 0.05 * rng.standard_normal(base.shape), 0, 1)
    return a.astype(np.float32), b.astype(np.float32)
