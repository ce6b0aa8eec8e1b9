"""Edge cases for the map-edit kernels (splatam_amd/csrc/mapedit.hip) and plain float64 statements of their results.

No GPU, no fixtures: tests/test_mapedit_cases_cpu.py checks the generators and pins splatam_amd.slam's torch formulations to the
float64 statements below on the CPU; tests/test_gpu_mapedit_edges.py runs the device against both.  Every generator is
deterministic (a seed of its own per case) and returns CPU tensors plus a short dict of the properties it was built to have.

The boundaries the cases are built around (mapedit.hip): 64-lane ballots, 256-thread rounds, 4 rounds = 1024 rows per workgroup,
and single-workgroup scans that walk the per-workgroup counts 256 at a time with a carry, i.e. 262144 rows per chunk.

Every value that a kernel compares with a threshold is placed at least a relative MARGIN away from it, so no discrete decision
rests on the last bit of expf / a division; depths and rendered depths lie on a grid of multiples of 2^-10, so |gt - rd| is exact
in float32.  Nothing here calls the code under test.
"""
import zlib

import numpy as np
import torch

WAVE, ROUND, GROUP = 64, 256, 1024
CHUNK = 256 * GROUP                     # rows whose workgroup counts one chunk of the scan covers
MARGIN = 1e-3
GRID = 1024.0                           # depths are multiples of 1 / GRID

GAUSSIAN_KEYS = ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales')
VAR_KEYS = ('max_2D_radius', 'means2D_gradient_accum', 'denom', 'timestep')

# ---------------------------------------------------------------------------------------------------------------------
# keep / select masks
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 262143, 262144, 262145, 263169)
CARRY_PATTERNS = ("first_256_groups", "after_256_groups")       # the whole selection on one side of the scan's first chunk
PATTERNS = ("none", "all", "first", "last", "last_of_64", "last_of_256", "last_of_1024", "first_of_1024", "all_but_one_per_group",
            "random50", "random1", "one_full_group") + CARRY_PATTERNS
EVERYWHERE = ("none", "all", "last", "random50")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def select_mask(n, pattern, seed=0):
    """bool[n]: the selected rows / pixels of ``pattern``."""
    m = np.zeros(n, dtype=bool)
    i = np.arange(n)
    rng = _rng("mask", n, pattern, seed)
    if pattern == "none":
        pass
    elif pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[n - 1] = True
    elif pattern == "last_of_64":
        m[i % WAVE == WAVE - 1] = True
    elif pattern == "last_of_256":
        m[i % ROUND == ROUND - 1] = True
    elif pattern == "last_of_1024":
        m[i % GROUP == GROUP - 1] = True
    elif pattern == "first_of_1024":
        m[i % GROUP == 0] = True
    elif pattern == "all_but_one_per_group":
        m[:] = True
        for start in range(0, n, GROUP):
            m[start + int(rng.integers(min(GROUP, n - start)))] = False
    elif pattern == "random50":
        m = rng.random(n) < 0.5
    elif pattern == "random1":
        m = rng.random(n) < 0.01
    elif pattern == "one_full_group":
        m[:GROUP] = True
    elif pattern == "first_256_groups":
        m[:CHUNK] = True
    elif pattern == "after_256_groups":
        m[CHUNK:] = True
    else:
        raise ValueError(pattern)
    return m


def _kept_compaction_cases():
    cases = [(n, p) for n in SIZES for p in EVERYWHERE]
    for n in (1025, 262145):
        cases += [(n, p) for p in PATTERNS if p not in EVERYWHERE and p not in CARRY_PATTERNS]
    cases += [(n, p) for n in (262145, 263169) for p in CARRY_PATTERNS]
    # a pattern once more where its period meets the size
    cases += [(64, "last_of_64"), (65, "last_of_64"), (256, "last_of_256"), (257, "last_of_256"), (1024, "last_of_1024"),
              (2049, "last_of_1024"), (2049, "first_of_1024"), (2049, "one_full_group"), (2049, "all_but_one_per_group")]
    return cases


# the kept cross product of sizes and patterns: every pattern at 1025 and at 262145 rows (the two carry patterns need more than 256
# workgroups: 262145 and 263169), "none" / "all" / "last" / "random50" at every size, and the periodic patterns at their own period
COMPACTION_CASES = _kept_compaction_cases()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def map_state(n, cols=1, seed=0):
    """A map of ``n`` rows with every copied field distinct and non-zero: parameters, both Adam moments, the four variables."""
    rng = _rng("map", n, cols, seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)        # noqa: E731
    widths = dict(zip(GAUSSIAN_KEYS, (3, 3, 4, 1, cols)))
    params = {'means3D': f(n, 3) * 2.0, 'rgb_colors': rng.random((n, 3)).astype(np.float32), 'unnorm_rotations': f(n, 4) + 0.1,
              'logit_opacities': f(n, 1), 'log_scales': (f(n, cols) * 0.3 - 4.0)}
    state = {'params': {k: _t(v) for k, v in params.items()},
             'exp_avg': {k: _t(f(n, w)) for k, w in widths.items()},
             'exp_avg_sq': {k: _t(rng.random((n, w)).astype(np.float32) + 0.01) for k, w in widths.items()},
             'variables': {'max_2D_radius': _t(rng.random(n).astype(np.float32) * 9 + 1), 'means2D_gradient_accum': _t(rng.random(n).astype(np.float32) + 0.5),
                           'denom': _t(rng.integers(1, 5, n).astype(np.float32)), 'timestep': _t(rng.integers(0, 3, n).astype(np.float32))}}
    return state


def compacted(state, keep):
    """``state`` with only the rows of bool ``keep``, by numpy boolean indexing: what remove_points(~keep) must leave, bit for bit."""
    keep = np.asarray(keep, dtype=bool)
    out = {}
    for group in ('params', 'exp_avg', 'exp_avg_sq', 'variables'):
        out[group] = {k: v.numpy()[keep] for k, v in state[group].items() if group != 'params' or k in GAUSSIAN_KEYS}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# depth-error planes for the median
# ---------------------------------------------------------------------------------------------------------------------
PLANE_SIZES = ((1, 1), (2, 1), (17, 15), (16, 16), (257, 1), (32, 32), (41, 25), (513, 512))
DISTRIBUTIONS = ("equal", "mostly_zero", "half_zero", "half_zero_less_one", "two_lower", "two_upper", "bits_low", "bits_mid", "bits_high",
                 "inf_minority", "inf_half", "inf_majority", "nan_one", "zero_times_inf")


def _applies(dist, hw):
    if dist in ("half_zero", "half_zero_less_one", "inf_half"):
        return hw % 2 == 0
    if dist == "two_upper":
        return hw >= 3
    if dist == "two_lower":
        return hw >= 2
    return True


MEDIAN_CASES = [(w, h, d) for (w, h) in PLANE_SIZES for d in DISTRIBUTIONS if _applies(d, w * h)]


def _grid(rng, lo, hi, n):
    return (rng.integers(int(lo * GRID), int(hi * GRID) + 1, n) / GRID).astype(np.float32)


def depth_error(gt, rd):
    """|gt - rd| * (gt > 0) in float32, as the reference forms it (inf * 0 = NaN included)."""
    gt, rd = np.asarray(gt, dtype=np.float32), np.asarray(rd, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (np.abs(gt - rd) * (gt > 0).astype(np.float32)).astype(np.float32).reshape(-1)


def lower_median(err):
    """torch.median of a float32 vector: the element of rank (n - 1) // 2, NaN if any element is NaN."""
    err = np.asarray(err, dtype=np.float32).reshape(-1)
    if np.isnan(err).any():
        return np.float32(np.nan)
    return np.sort(err)[(err.size - 1) // 2]


def median_plane(W, H, dist):
    """(gt, rd, props): float32 [H W] depth and rendered depth whose depth errors have distribution ``dist``."""
    hw = W * H
    rank = (hw - 1) // 2
    rng = _rng("plane", W, H, dist)
    gt = _grid(rng, 0.5, 5.0, hw)
    sign = np.where(rng.random(hw) < 0.5, -1.0, 1.0).astype(np.float32)
    some = _grid(rng, 1 / GRID, 0.4, hw)                # a spread of non-zero errors, all below 0.5 <= gt
    perm = rng.permutation(hw)
    props = {'rank': rank}
    e = some
    if dist == "equal":
        e = np.full(hw, 0.25, dtype=np.float32)
    elif dist in ("mostly_zero", "half_zero", "half_zero_less_one"):
        zeros = {"mostly_zero": hw // 2 + 1, "half_zero": hw // 2, "half_zero_less_one": hw // 2 - 1}[dist]
        props['zeros'] = zeros
    elif dist in ("two_lower", "two_upper"):
        lower = rank + 1 if dist == "two_lower" else rank
        e = np.full(hw, 0.375, dtype=np.float32)
        e[perm[:lower]] = 0.125
        props['lower'] = lower
    rd = gt + sign * e
    if 'zeros' in props:
        gt[perm[:props['zeros']]] = 0.0                 # invalid depth: error exactly 0 whatever was rendered
    if dist.startswith("bits_"):
        if dist == "bits_low":
            bits = 0x3f800000 | rng.integers(0, 1 << 10, hw)
        elif dist == "bits_mid":
            bits = 0x3f800000 | (rng.integers(0, 1 << 11, hw) << 10)
        else:
            bits = rng.integers(256, 1020, hw) << 21    # normal, finite, positive: only bits 21 and up differ
        gt = bits.astype(np.uint32).view(np.float32)
        rd = np.zeros(hw, dtype=np.float32)             # |gt - 0| = gt: the error IS the bit pattern
    elif dist in ("inf_minority", "inf_half", "inf_majority"):
        # the most that is still fewer than half; exactly half (even HW: the lower median is the last finite error); one more than the
        # median can bear
        k = {"inf_minority": (hw - 1) // 2, "inf_half": hw // 2, "inf_majority": hw - rank}[dist]
        rd[perm[:k]] = np.inf
        props['infs'] = k
    elif dist == "nan_one":
        rd[perm[0]] = np.nan
    elif dist == "zero_times_inf":
        gt[perm[0]], rd[perm[0]] = 0.0, np.inf
    props['expected'] = lower_median(depth_error(gt, rd))
    return _t(gt), _t(rd), props


# ---------------------------------------------------------------------------------------------------------------------
# frames for add_new_gaussians / add_valid_depth_points
# ---------------------------------------------------------------------------------------------------------------------
SPECIAL_FRAMES = ("invalid_selected", "depth_rule", "sil_rule", "nan_median", "median_zero")
TIME_IDX, SIL_THRES, N0, NUM_FRAMES = 2, 0.5, 37, 4


def _kept_add_cases():
    cases = []
    for j, (w, h) in enumerate(PLANE_SIZES):
        cases += [(w, h, p, 1 + 2 * ((j + i) % 2)) for i, p in enumerate(EVERYWHERE)]
    cases += [(41, 25, p, 1 + 2 * (i % 2)) for i, p in enumerate(PATTERNS) if p not in EVERYWHERE and p not in CARRY_PATTERNS]
    cases += [(513, 512, p, 3 - 2 * (i % 2)) for i, p in enumerate(PATTERNS) if p not in EVERYWHERE]
    for j, (w, h) in enumerate(((17, 15), (41, 25), (513, 512))):
        cases += [(w, h, k, 1 + 2 * ((i + j) % 2)) for i, k in enumerate(SPECIAL_FRAMES)]
    return cases


# (W, H, kind, log_scales columns): "none" / "all" / "last" / "random50" at every frame size, every pattern at 41x25 (1025 pixels)
# and 513x512 (257 workgroups: the carry patterns apply), the five rule frames at 255, 1025 and 262656 pixels; both layouts throughout
ADD_CASES = _kept_add_cases()


def intrinsics_for(W, H):
    """fx != fy, all four exact in float32, back-projected x / y within a few units at depth 5."""
    fx, fy = round(0.9 * max(W, 4) * 8) / 8, round(1.1 * max(H, 4) * 8) / 8
    return np.array([[fx, 0, W / 2 - 0.25], [0, fy, H / 2 - 0.75], [0, 0, 1]], dtype=np.float32)


def add_frame(W, H, kind, cols):
    """One add_new_gaussians case: a map of N0 rows (all four variables non-zero), poses of NUM_FRAMES frames with a non-identity
    one at TIME_IDX, an image, a depth plane, the [depth, silhouette] stand-in for the render, intrinsics with fx != fy."""
    hw = W * H
    rng = _rng("add", W, H, kind, cols)
    st = map_state(N0, cols, seed=("add", W, H, kind))
    rots = np.zeros((1, 4, NUM_FRAMES), dtype=np.float32)
    rots[0, 0, :] = 1.0
    rots[0, :, TIME_IDX] = np.array([0.9, 0.1, -0.2, 0.15], dtype=np.float32) * 1.3         # not normalised either
    trans = np.zeros((1, 3, NUM_FRAMES), dtype=np.float32)
    trans[0, :, TIME_IDX] = (0.3, -0.2, 0.4)
    gt = _grid(rng, 0.5, 5.0, hw)
    rd = gt - (rng.integers(1, 9, hw) / GRID).astype(np.float32)       # rendered in front of the measurement: the depth rule is silent
    sil = np.full(hw, 0.75, dtype=np.float32)
    u = rng.random(hw)
    props = {}
    if kind in PATTERNS:
        sil[select_mask(hw, kind, seed="add")] = 0.25
    elif kind == "invalid_selected":
        m = select_mask(hw, "random50", seed="add")
        sil[m], gt[m] = 0.25, 0.0
    elif kind == "depth_rule":
        # errors of 1..4 / GRID with the median on 2 / GRID, so the threshold is 100 / GRID; rendered BEHIND the measurement
        sil[:] = 1.0
        k = np.where(u < 0.05, 1, np.where(u < 0.70, 2, np.where(u < 0.75, 3, 4)))
        k = np.where(u >= 0.80, np.where(u < 0.85, 90, np.where(u < 0.90, 110, 256)), k)     # below / above / far above the threshold
        rd = gt + (k / GRID).astype(np.float32)
        far_front = rng.random(hw) < 0.1
        rd[far_front] = gt[far_front] - np.float32(0.25)                # a large error in FRONT never selects
        props['median'] = np.float32(2 / GRID)
    elif kind == "sil_rule":
        sil[u < 0.3] = 0.25
        rd = gt + (rng.integers(1, 4, hw) / GRID).astype(np.float32)    # behind, but all within 3 / GRID <= 50 x median
    elif kind == "nan_median":
        sil[u < 0.3] = 0.25
        behind = rng.random(hw) < 0.1
        rd[behind] = gt[behind] + np.float32(0.25)                      # would select under any finite median
        j = int(np.flatnonzero(u >= 0.3)[0])
        rd[j] = np.nan
    elif kind == "median_zero":
        sil[:] = 1.0
        gt[u < 0.6] = 0.0
        k = rng.integers(-8, 9, hw)                                     # behind (selects), in front, and exactly on it (k == 0)
        rd = np.where(gt > 0, gt + (k / GRID).astype(np.float32), np.float32(1.5)).astype(np.float32)
        props['median'] = np.float32(0.0)
    else:
        raise ValueError(kind)
    frame = {'params': dict(st['params'], cam_unnorm_rots=_t(rots), cam_trans=_t(trans)), 'variables': st['variables'],
             'exp_avg': st['exp_avg'], 'exp_avg_sq': st['exp_avg_sq'],
             'im': _t(rng.random((3, H, W)).astype(np.float32)), 'depth': _t(gt.reshape(1, H, W)),
             'depth_sil': _t(np.stack([rd.reshape(H, W), sil.reshape(H, W)])), 'intrinsics': _t(intrinsics_for(W, H)),
             'time_idx': TIME_IDX, 'sil_thres': SIL_THRES, 'W': W, 'H': H, 'cols': cols}
    return frame, props


def quat_rotation64(q):
    """Rotation(s) of the quaternion(s) (w, x, y, z) [..., 4], normalised here, in float64: [..., 3, 3]."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    r, x, y, z = np.moveaxis(q, -1, 0)
    rows = (1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y))
    return np.stack(rows, axis=-1).reshape(q.shape[:-1] + (3, 3))


def backproject64(depth, intrinsics, w2c, pick, W, H):
    """World-frame points and log scales of the picked pixels, float64: x = (u - cx) / fx z, y = (v - cy) / fy z, through the inverse
    of the world-to-camera transform; scale = z / ((fx + fy) / 2)."""
    k = np.asarray(intrinsics, dtype=np.float64)
    fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    i = np.flatnonzero(pick)
    v, u = i // W, i % W
    z = np.asarray(depth, dtype=np.float64).reshape(-1)[i]
    cam = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    c2w = np.linalg.inv(np.asarray(w2c, dtype=np.float64))
    return cam @ c2w[:3, :3].T + c2w[:3, 3], np.log(z / ((fx + fy) / 2))


def appended(frame, pick, w2c, reset, time_idx):
    """The map after appending one Gaussian per pixel of ``pick`` (pixel order): copied fields exact, means3D / log_scales float64."""
    W, H, cols = frame['W'], frame['H'], frame['cols']
    pts, ls = backproject64(frame['depth'].numpy(), frame['intrinsics'].numpy(), w2c, pick, W, H)
    n = pts.shape[0]
    i = np.flatnonzero(pick)
    p = {k: v.numpy() for k, v in frame['params'].items()}
    rot = np.zeros((n, 4), dtype=np.float32)
    rot[:, 0] = 1.0
    new = {'means3D': pts, 'rgb_colors': frame['im'].numpy().reshape(3, -1).T[i], 'unnorm_rotations': rot,
           'logit_opacities': np.zeros((n, 1), dtype=np.float32), 'log_scales': np.repeat(ls[:, None], cols, axis=1)}
    out = {'params': {k: np.concatenate([p[k].astype(new[k].dtype), new[k]]) for k in GAUSSIAN_KEYS}, 'added': n,
           'copied': np.arange(p['means3D'].shape[0] + n) < p['means3D'].shape[0]}
    for m in ('exp_avg', 'exp_avg_sq'):
        out[m] = {k: np.concatenate([frame[m][k].numpy(), np.zeros((n,) + new[k].shape[1:], dtype=np.float32)]) for k in GAUSSIAN_KEYS}
    var = {k: v.numpy() for k, v in frame['variables'].items()}
    if reset:
        out['variables'] = {k: np.zeros(p['means3D'].shape[0] + n, dtype=np.float32) for k in VAR_KEYS[:3]}
        out['variables']['timestep'] = np.concatenate([var['timestep'], np.full(n, float(time_idx), dtype=np.float32)])
    else:
        out['variables'] = var
    return out


def expected_add(frame):
    """add_new_gaussians on ``frame``: non_presence = sil < thres | (rd > gt & err > 50 median); rows for non_presence & gt > 0; the
    three per-Gaussian variables re-created for ALL rows whenever non_presence has a set pixel, even if no row is added."""
    gt = frame['depth'].numpy().reshape(-1)
    rd, sil = frame['depth_sil'][0].numpy().reshape(-1), frame['depth_sil'][1].numpy().reshape(-1)
    err = depth_error(gt, rd)
    med = lower_median(err)
    with np.errstate(invalid="ignore"):
        behind = (rd > gt) & (err > np.float32(50) * med)
    non_presence = (sil < np.float32(frame['sil_thres'])) | behind
    pick = non_presence & (gt > 0)
    w2c = np.eye(4)
    w2c[:3, :3] = quat_rotation64(frame['params']['cam_unnorm_rots'].numpy()[0, :, frame['time_idx']])
    w2c[:3, 3] = frame['params']['cam_trans'].numpy()[0, :, frame['time_idx']]
    out = appended(frame, pick, w2c, bool(non_presence.any()), frame['time_idx'])
    out.update(median=med, non_presence=int(non_presence.sum()), behind=behind, err=err, pick=pick)
    return out


def valid_depth_frame(W, H, cols, n0):
    """add_valid_depth_points: ~30 % of the depths invalid (0, a few negative), a world-to-camera transform that is not the identity,
    on a map of ``n0`` rows (0: the first frame of a run)."""
    rng = _rng("valid", W, H, cols, n0)
    frame, _ = add_frame(W, H, "all", cols)
    if n0 == 0:
        for g in ('params', 'exp_avg', 'exp_avg_sq'):
            frame[g] = {k: (v[:0].clone() if k in GAUSSIAN_KEYS else v) for k, v in frame[g].items()}
        frame['variables'] = {k: v[:0].clone() for k, v in frame['variables'].items()}
    gt = frame['depth'].numpy().reshape(-1).copy()
    u = rng.random(W * H)
    gt[u < 0.25] = 0.0
    gt[(u >= 0.25) & (u < 0.30)] = -1.0
    frame['depth'] = _t(gt.reshape(1, H, W))
    w2c = np.eye(4)
    w2c[:3, :3] = quat_rotation64([0.8, -0.3, 0.2, 0.1])
    w2c[:3, 3] = (-0.5, 0.25, 0.75)
    frame['w2c'] = _t(w2c.astype(np.float32))
    return frame


def expected_valid_depth(frame, time_idx=0):
    pick = frame['depth'].numpy().reshape(-1) > 0
    return appended(frame, pick, frame['w2c'].numpy(), bool(pick.any()), time_idx)


# ---------------------------------------------------------------------------------------------------------------------
# pruning by opacity / size
# ---------------------------------------------------------------------------------------------------------------------
PRUNE_RADIUS, PRUNE_OPACITY = 3.0, 0.005
PRUNE_CASES = [(n, rule) for n in (1025, 262145) for rule in ("opacity", "opacity_size", "aniso")]


def prune_state(n, rule):
    """Opacities either side of PRUNE_OPACITY and scales either side of 0.1 PRUNE_RADIUS, each at least 9 % / 3 % away; "aniso": three
    scale columns of which at most one is the big one, in any column."""
    cols = 3 if rule == "aniso" else 1
    rng = _rng("prune", n, rule)
    st = map_state(n, cols, seed=("prune", rule))
    cut = np.log(PRUNE_OPACITY / (1 - PRUNE_OPACITY))
    faint = rng.random(n) < 0.3
    logit = np.where(faint, rng.uniform(cut - 3.0, cut - 0.1, n), rng.uniform(cut + 0.1, 4.0, n)).astype(np.float32)
    st['params']['logit_opacities'] = _t(logit.reshape(n, 1))
    big = rng.random(n) < 0.2
    scale = rng.uniform(0.01, 0.29, (n, cols))
    col = rng.integers(0, cols, n)
    scale[np.flatnonzero(big), col[big]] = rng.uniform(0.31, 0.5, int(big.sum()))
    st['params']['log_scales'] = _t(np.log(scale).astype(np.float32))
    st['props'] = {'faint': faint, 'big': big}
    return st


def expected_prune(st, remove_big):
    op = 1.0 / (1.0 + np.exp(-st['params']['logit_opacities'].numpy().astype(np.float64)[:, 0]))
    rem = op < PRUNE_OPACITY
    if remove_big:
        rem |= np.exp(st['params']['log_scales'].numpy().astype(np.float64)).max(axis=1) > 0.1 * PRUNE_RADIUS
    return rem


# ---------------------------------------------------------------------------------------------------------------------
# densification states
# ---------------------------------------------------------------------------------------------------------------------
DENSIFY_RADIUS, GRAD_THRESH = 2.0, 2e-4
DENSIFY_KINDS = {           # kind: (num_to_split_into, final prune)
    "nothing": (2, "keep"), "clone_only": (2, "keep"), "split_only": (2, "subset"), "mixed_1": (1, "keep"), "mixed_2": (2, "subset"),
    "mixed_3": (3, "keep"), "thresh_0": (2, "subset"), "double_growth": (3, "keep")}
DENSIFY_MASKED = ("last_of_64", "all_but_one_per_group", "all") + CARRY_PATTERNS     # the selection of one step laid on a boundary


def _kept_densify_cases():
    cases = [(n, "mixed_2") for n in SIZES]
    cases += [(n, k) for n in (1025, 262145) for k in DENSIFY_KINDS if k not in ("mixed_2", "double_growth")]
    cases += [(2049, "double_growth")]
    cases += [(1025, f"{step}:{p}") for step in ("clone", "split") for p in ("last_of_64", "all")]
    cases += [(262145, f"{step}:{p}") for step in ("clone", "split") for p in DENSIFY_MASKED]
    cases += [(263169, f"{step}:after_256_groups") for step in ("clone", "split")]
    return cases


# "mixed_2" at every size; every kind at 1025 and 262145 rows ("double_growth", the capacity test's state, at 2049); "clone:<pattern>" / "split:<pattern>": exactly the rows of a compaction
# pattern reach the threshold and are small / large, at 1025 and 262145 rows, the carry pattern also at 263169 (258 workgroups)
DENSIFY_CASES = _kept_densify_cases()


def densify_state(n, kind):
    """An isotropic map of ``n`` rows before densify(): mean gradients either side of GRAD_THRESH (>= 1 % away), with 0 / 0 rows and
    rows of gradient exactly 0; scales either side of 0.01 R (and, for "subset" prunes, of 0.1 R before AND after the split's division);
    a non-constant timestep; non-zero moments."""
    rng = _rng("densify", n, kind)
    st = map_state(n, 1, seed=("densify", kind))
    n_split, prune = DENSIFY_KINDS.get(kind, (2, "keep"))
    u, w = rng.random(n), rng.random(n)
    high = u < 0.5
    large = w < 0.5
    if kind == "nothing":
        high[:] = False
    elif kind == "clone_only":
        large[:] = False
    elif kind == "split_only":
        large[:] = True
    elif kind == "double_growth":                           # a few clones, then three times nearly the whole map from the split
        high[:] = True
        large = np.arange(n) % 100 != 0
    elif ":" in kind:
        step, pattern = kind.split(":")
        high = select_mask(n, pattern, seed="densify")
        large = high if step == "split" else ~high          # the unselected rows are of the other size: only the gradient holds them back
        large = large.copy()
    thr = 0.0 if kind == "thresh_0" else GRAD_THRESH
    denom = rng.integers(1, 5, n).astype(np.float32)
    g = np.where(high, rng.uniform(1.01, 5.0, n), rng.uniform(0.05, 0.99, n)) * GRAD_THRESH
    accum = (g * denom).astype(np.float32)
    idx = np.arange(n)
    free = ~high if ":" in kind else np.ones(n, dtype=bool)  # (a boundary pattern keeps exactly its rows above the threshold)
    accum[(idx % 11 == 1) & free] = 0.0                     # a gradient of exactly 0
    nan = (idx % 7 == 0) & free
    accum[nan], denom[nan] = 0.0, 0.0                       # 0 / 0 -> NaN -> 0
    small_cut = 0.01 * DENSIFY_RADIUS
    scale = np.where(large, rng.uniform(small_cut * 1.005, 0.1, n), rng.uniform(0.005, small_cut * 0.995, n))
    logit = rng.uniform(0.5, 3.0, n)
    if prune == "subset":
        big = large & (rng.random(n) < 0.15)                # beyond 0.1 R: 0.21 .. 0.3, children 0.0875 .. 0.1875 (n = 2, 3)
        scale[big] = rng.uniform(0.21, 0.3, int(big.sum()))
        logit[rng.random(n) < 0.2] = -2.0                   # opacity 0.119 against a threshold of 0.3; the others >= 0.62
    st['params']['log_scales'] = _t(np.log(scale).astype(np.float32).reshape(n, 1))
    st['params']['logit_opacities'] = _t(logit.astype(np.float32).reshape(n, 1))
    st['variables']['means2D_gradient_accum'], st['variables']['denom'] = _t(accum), _t(denom)
    st['variables']['timestep'] = _t((np.arange(n) % 5).astype(np.float32))
    st['dict'] = dict(start_after=0, remove_big_after=0, stop_after=100, densify_every=1, grad_thresh=thr, num_to_split_into=n_split,
                      removal_opacity_threshold=0.3 if prune == "subset" else 0.0,
                      final_removal_opacity_threshold=0.3 if prune == "subset" else 0.0, reset_opacities=False, reset_opacities_every=3000)
    st['radius'] = DENSIFY_RADIUS
    return st


def densify_selection(st):
    """(to_clone, to_split) over the original rows, in float64 from the float32 inputs."""
    v = st['variables']
    with np.errstate(invalid="ignore", divide="ignore"):
        g = v['means2D_gradient_accum'].numpy().astype(np.float64) / v['denom'].numpy().astype(np.float64)
    g[np.isnan(g)] = 0.0
    scale = np.exp(st['params']['log_scales'].numpy().astype(np.float64)[:, 0])
    reach = g >= st['dict']['grad_thresh']
    small = scale <= 0.01 * st['radius']
    return reach & small, reach & ~small, g, scale


def expected_densify(st, normals):
    """densify() on ``st`` with the split's standard-normal draws ``normals`` [n_split S, 3] (sample = draw * scale): clones appended
    in row order, then n_split blocks of the split rows (means3D + R(q) sample, scale / (0.8 n_split)), the three variables zeroed,
    timestep of a new row = its source's, the split originals removed, then the opacity / size prune.  float64 where computed."""
    d, R = st['dict'], st['radius']
    n_split = d['num_to_split_into']
    to_clone, to_split, _, scale = densify_selection(st)
    n = to_clone.size
    p = {k: st['params'][k].numpy() for k in GAUSSIAN_KEYS}
    S = int(to_split.sum())
    rot = quat_rotation64(p['unnorm_rotations'][to_split])
    rot = np.tile(rot, (n_split, 1, 1))
    sample = np.asarray(normals, dtype=np.float64).reshape(n_split * S, 3) * np.tile(scale[to_split], n_split)[:, None]
    out = {'params': {}, 'exp_avg': {}, 'exp_avg_sq': {}}
    for k in GAUSSIAN_KEYS:
        rows = np.tile(p[k][to_split], (n_split, 1)).astype(np.float64 if k in ('means3D', 'log_scales') else np.float32)
        if k == 'means3D':
            rows = rows + np.einsum('nij,nj->ni', rot, sample)
        if k == 'log_scales':
            rows = np.log(np.exp(rows) / (0.8 * n_split))
        out['params'][k] = np.concatenate([p[k].astype(rows.dtype), p[k][to_clone].astype(rows.dtype), rows])
        for m in ('exp_avg', 'exp_avg_sq'):
            out[m][k] = np.concatenate([st[m][k].numpy(), np.zeros((int(to_clone.sum()) + n_split * S,) + p[k].shape[1:], dtype=np.float32)])
    ts = st['variables']['timestep'].numpy()
    source = np.concatenate([np.arange(n), np.flatnonzero(to_clone), np.tile(np.flatnonzero(to_split), n_split)])
    total = source.size
    keep = np.ones(total, dtype=bool)
    keep[:n] = ~to_split
    opacity = 1.0 / (1.0 + np.exp(-out['params']['logit_opacities'].astype(np.float64)[:, 0]))
    final_scale = np.exp(out['params']['log_scales'].astype(np.float64)[:, 0])
    keep &= ~((opacity < d['removal_opacity_threshold']) | (final_scale > 0.1 * R))
    for g in ('params', 'exp_avg', 'exp_avg_sq'):
        out[g] = {k: v[keep] for k, v in out[g].items()}
    rows = int(keep.sum())
    out['variables'] = {k: np.zeros(rows, dtype=np.float32) for k in VAR_KEYS[:3]}
    out['variables']['timestep'] = ts[source][keep]
    out.update(cloned=int(to_clone.sum()), split=S, peak=total, source=source[keep], final_scale=final_scale, opacity=opacity,
               copied=(np.arange(total) < n + int(to_clone.sum()))[keep])      # rows that are copies: bit for bit
    return out
