"""Float64 numpy restatement of the view overlay (splatam_amd/csrc/viewoverlay_math.h, csrc/viewoverlay.hip), shared by
tests/test_viewoverlay_cpu.py and tests/test_gpu_view_overlay.py.  Inputs are what the kernels read (float32 points and matrices),
widened; every step is then float64, written from the definitions in include/splat_hip.h and not from the header's code.

``line64`` also says which pixels are FRAGILE: a float64 position within ``NEAR`` = 1e-4 px of the boundary at which it rounds to
another pixel.  There the header (also double, but with its own order of operations) may round the other way, and the tests excuse a
difference -- on at most ``MAX_EXCUSED`` = 1 % of a case's covered pixels, which the fixed inputs of the tests are chosen to respect.

``DEPTH_RTOL``: the depth of a step is 1 / w evaluated in double and rounded to float32 ONCE: half an ulp, 2^-24 relative.  The double
evaluation behind it (a dozen operations on positive terms, no cancellation: w lies between the ends' w) differs between the two
forms by a few 2^-53, which moves the float32 result only when it sits that close to a rounding boundary -- then by one more ulp of
float32 at most.  So |z - z64| <= 2^-24 z64 almost always and <= 3 * 2^-24 z64 always: the bound is 3 * 2^-24 relative."""
import math

import numpy as np

NEAR = 1e-4
MAX_EXCUSED = 0.01
DEPTH_RTOL = 3.0 * 2.0 ** -24
SEGMENT_BIT = 1 << 31
NO_KEY = (1 << 64) - 1
FRUSTUM_EDGES = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1))


def cool_lut64():
    """[256, 3] uint8: entry i of matplotlib's `cool` = (i / 255, 1 - i / 255, 1), as bytes rounded to nearest."""
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.rint(255.0 * np.stack([v, 1.0 - v, np.ones(256)], axis=1)).astype(np.uint8)


def cool64(x):
    return cool_lut64()[min(int(256.0 * x), 255)]


def run64(w2cs, w, h, fx, fy, cx, cy, scale, frusta=True, fixed=None):
    """(segments [., 6] float64, colors [., 3] uint8) of a run given as float64 w2c matrices: trajectory segments [0, n - 1), then
    eight per frame."""
    n = len(w2cs)
    centres, corners = [], []
    for M in w2cs:
        M = np.asarray(M, dtype=np.float64).reshape(4, 4)
        Rt, c = M[:3, :3].T, -(M[:3, :3].T @ M[:3, 3])
        centres.append(c)
        pts = [c]
        for u, v in ((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)):
            pts.append(Rt @ (np.array([(u - cx) / fx, (v - cy) / fy, 1.0]) * scale) + c)
        corners.append(pts)
    segs, cols = [], []
    for j in range(n - 1):
        segs.append(np.concatenate([centres[j], centres[j + 1]]))
        cols.append(cool64(0.5 * j / (n - 1) + 0.5) if fixed is None else np.asarray(fixed, np.uint8))
    if frusta:
        for t in range(n):
            for a, b in FRUSTUM_EDGES:
                segs.append(np.concatenate([corners[t][a], corners[t][b]]))
                cols.append(cool64(0.5 * t / n) if fixed is None else np.asarray(fixed, np.uint8))
    return np.array(segs, dtype=np.float64).reshape(-1, 6), np.array(cols, dtype=np.uint8).reshape(-1, 3)


def _near_boundary(x):
    """Whether floor(x + 0.5) could come out differently within NEAR."""
    f = (x + 0.5) - math.floor(x + 0.5)
    return min(f, 1.0 - f) <= NEAR


def line64(seg, w2c, W, H, fx, fy, cx, cy, near, width=1):
    """One segment (6 float32 world coordinates) through ``w2c`` (float32 4 x 4): ``(pixels, fragile, steps)`` -- ``pixels`` {(i, j): z}
    with the smallest float64 depth stamped on each pixel inside the image, ``fragile`` the set of pixels (inside or not) a rounding
    within NEAR of its boundary could add, drop or move, ``steps`` the centre line [(i, j, z)]."""
    seg = np.asarray(seg, dtype=np.float32).astype(np.float64)
    M = np.asarray(w2c, dtype=np.float32).astype(np.float64).reshape(4, 4)
    fx, fy, cx, cy, near = (float(np.float32(v)) for v in (fx, fy, cx, cy, near))
    a, b = seg[:3], seg[3:]
    if tuple(a) > tuple(b):
        a, b = b, a
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return {}, set(), []
    A, B = M[:3, :3] @ a + M[:3, 3], M[:3, :3] @ b + M[:3, 3]
    if not (np.isfinite(A).all() and np.isfinite(B).all()) or (A[2] < near and B[2] < near):
        return {}, set(), []
    if A[2] < near:
        A = B + (near - B[2]) / (A[2] - B[2]) * (A - B)
        A[2] = near
    elif B[2] < near:
        B = A + (near - A[2]) / (B[2] - A[2]) * (B - A)
        B[2] = near
    p0 = np.array([fx * A[0] / A[2] + cx, fy * A[1] / A[2] + cy, 1.0 / A[2]])
    p1 = np.array([fx * B[0] / B[2] + cx, fy * B[1] / B[2] + cy, 1.0 / B[2]])
    d = p1 - p0
    t0, t1 = 0.0, 1.0
    for p, q in ((-d[0], p0[0] + 0.5), (d[0], W - 0.5 - p0[0]), (-d[1], p0[1] + 0.5), (d[1], H - 0.5 - p0[1])):
        if p == 0.0:
            if q < 0.0:
                return {}, set(), []
            continue
        r = q / p
        if p < 0.0:
            if r > t1:
                return {}, set(), []
            t0 = max(t0, r)
        else:
            if r < t0:
                return {}, set(), []
            t1 = min(t1, r)
    q0, q1 = p0 + t0 * d, p0 + t1 * d
    lo, hi = np.array([-0.5, -0.5]), np.array([W - 0.5, H - 0.5])
    q0[:2], q1[:2] = np.clip(q0[:2], lo, hi), np.clip(q1[:2], lo, hi)
    steep = abs(q1[1] - q0[1]) > abs(q1[0] - q0[0])
    undecided = abs(abs(q1[1] - q0[1]) - abs(q1[0] - q0[0])) <= NEAR and not np.array_equal(q0[:2], q1[:2])
    ma, mi = (1, 0) if steep else (0, 1)
    if q0[ma] > q1[ma]:
        q0, q1 = q1, q0
    m0, m1 = math.ceil(q0[ma]), math.floor(q1[ma])          # the pixel centres the span covers ...
    none = m1 < m0
    if none:
        m0 = m1 = math.floor(q0[ma] + 0.5)                  # ... or, if it covers none, one step where it starts
    n = min(m1 - m0 + 1, max(W, H) + 1)
    pixels, fragile, steps = {}, set(), []
    span = q1[ma] - q0[ma]
    half = (width - 1) // 2

    def at(major, minor):
        return (minor, major) if steep else (major, minor)
    for k in range(n):
        m = m0 + k
        s = min(max((m - q0[ma]) / span, 0.0), 1.0) if span > 0.0 else 0.0
        pos = q0[mi] + s * (q1[mi] - q0[mi])
        minor = math.floor(pos + 0.5)
        z = 1.0 / (q0[2] + s * (q1[2] - q0[2]))
        steps.append(at(m, minor) + (z,))
        for q in range(minor - half, minor - half + width):
            i, j = at(m, q)
            if 0 <= i < W and 0 <= j < H:
                pixels[(i, j)] = min(z, pixels.get((i, j), np.inf))
        if _near_boundary(pos) or undecided:
            fragile.update(at(m, q) for q in range(minor - half - 1, minor - half + width + 1))
    # an end whose major coordinate is within NEAR of a pixel centre (the centre is a step or not), or of covering no centre at all: the
    # column there and the ones beside it
    for end, m in ((q0, m0), (q1, m1)):
        if abs(end[ma] - round(end[ma])) <= NEAR or (none and end is q0 and _near_boundary(end[ma])):
            minor = math.floor(end[mi] + 0.5)
            fragile.update(at(mm, q) for mm in (m - 1, m, m + 1) for q in range(minor - half - 1, minor - half + width + 1))
    return pixels, fragile, steps


def point64(p, w2c, W, H, fx, fy, cx, cy, near, size=1):
    """(pixels [(i, j)], z, fragile): the footprint of one centre, its float64 depth, and whether its pixel is within NEAR of rounding
    elsewhere (or its depth of the near plane)."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    M = np.asarray(w2c, dtype=np.float32).astype(np.float64).reshape(4, 4)
    pc = M[:3, :3] @ p + M[:3, 3]
    if not np.isfinite(pc).all() or not pc[2] > near:
        return [], None, False
    u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
    i0, j0 = math.floor(u + 0.5) - (size - 1) // 2, math.floor(v + 0.5) - (size - 1) // 2
    px = [(i, j) for j in range(j0, j0 + size) for i in range(i0, i0 + size) if 0 <= i < W and 0 <= j < H]
    # the header forms the pixel in float32: a few ulps of |u| around the boundary, far inside NEAR for a small image
    return px, pc[2], _near_boundary(u) or _near_boundary(v) or abs(pc[2] - near) <= 1e-6


def resolve64(keys, depth, occlude, fill, rgb_colors, segment_colors, bg, rgb8):
    """The resolve on the host in plain numpy (exact: comparisons of float32 values and a byte conversion of stated rounding): ``keys``
    [H, W] uint64, ``depth`` [H, W] float32 or None, ``rgb8`` [H, W, 3] the picture before; returns the picture after."""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.array(rgb8, dtype=np.uint8, copy=True)

    def byte(c):
        c = np.float32(c)
        c = np.float32(0.0) if np.isnan(c) else min(max(c, np.float32(0.0)), np.float32(1.0))
        return int(np.rint(np.float32(c * np.float32(255.0))))
    if fill:
        out[:] = [byte(c) for c in bg]
    H, W = keys.shape
    for j in range(H):
        for i in range(W):
            key = int(keys[j, i])
            if key == NO_KEY:
                continue
            z = np.array([key >> 32], dtype=np.uint32).view(np.float32)[0]
            d = np.float32(0.0) if depth is None else np.float32(depth[j, i])
            if occlude and not (d <= 0 or z <= d):
                continue
            ident = key & 0xFFFFFFFF
            if ident & SEGMENT_BIT:
                s = ident & ~SEGMENT_BIT
                if s < len(segment_colors):
                    out[j, i] = segment_colors[s]
            elif ident < len(rgb_colors):
                out[j, i] = [byte(c) for c in rgb_colors[ident]]
    return out


def split_keys(keys):
    """(z float32, id uint32, drawn bool) planes of a key plane given as uint64 or int64."""
    k = np.ascontiguousarray(keys).view(np.uint64)
    return (k >> np.uint64(32)).astype(np.uint32).view(np.float32), (k & np.uint64(0xFFFFFFFF)).astype(np.uint32), k != np.uint64(NO_KEY)


# ---------------------------------------------------------------------------------------------------------------- the header's host build
class Shim:
    """tests/viewoverlay_math_shim.cpp through ctypes: the header's loops on numpy arrays (what the kernels are compared with)."""

    def __init__(self):
        import ctypes as C
        from tests.util import host_shim
        self.C, self.lib = C, host_shim("viewoverlay_math_shim", "viewoverlay_math.h", "meshshade_math.h", "meshrender_math.h", "view_math.h")

    def _p(self, a, t=None):
        C = self.C
        return None if a is None else a.ctypes.data_as(C.POINTER(t or C.c_float))

    def cool(self, x):
        out = np.zeros(3, np.uint8)
        self.lib.vo_shim_cool(self.C.c_double(x), self._p(out, self.C.c_uint8))
        return out

    def run(self, num_frames, size, k4, scale=0.045, w2c_all=None, rots=None, trans=None, first_w2c=None, first=0, count=None, frusta=True,
            fixed=None, segments=None, colors=None):
        """Arrays of a block ([9 n - 1] segments with frusta, [n - 1] without); given arrays are written in place."""
        C, n = self.C, num_frames
        total = n - 1 + (8 * n if frusta else 0)
        segments = np.full((total, 6), np.nan, np.float32) if segments is None else segments
        colors = np.full((total, 3), 7, np.uint8) if colors is None else colors
        keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (w2c_all, rots, trans, first_w2c)]
        fixed = None if fixed is None else np.asarray(fixed, np.uint8)
        self.lib.vo_shim_run(n, first, n - first if count is None else count, *(self._p(a) for a in keep), int(size[0]), int(size[1]),
                             *(C.c_double(float(v)) for v in tuple(k4) + (scale,)), int(bool(frusta)), self._p(fixed, C.c_uint8),
                             self._p(segments), self._p(colors, C.c_uint8))
        return segments, colors

    def keys(self, W, H):
        return np.full((H, W), NO_KEY, np.uint64)

    def points(self, keys, k4, near, w2c, means, size=1):
        H, W = keys.shape
        means = np.ascontiguousarray(means, np.float32)
        self.lib.vo_shim_points(W, H, self._p(np.asarray(k4, np.float32)), self.C.c_float(near), self._p(np.ascontiguousarray(w2c, np.float32)),
                                self._p(means), len(means), int(size), self._p(keys, self.C.c_uint64))
        return keys

    def segments(self, keys, k4, near, w2c, segments, first=0, count=None, width=1):
        H, W = keys.shape
        segments = np.ascontiguousarray(segments, np.float32).reshape(-1, 6)
        count = len(segments) - first if count is None else count
        return self.lib.vo_shim_segments(W, H, self._p(np.asarray(k4, np.float32)), self.C.c_float(near), self._p(np.ascontiguousarray(w2c, np.float32)),
                                         self._p(segments), int(first), int(count), int(width), self._p(keys, self.C.c_uint64))

    def walk(self, W, H, k4, near, w2c, seg):
        cap = max(W, H) + 8
        ij, z = np.zeros((cap, 2), np.int32), np.zeros(cap, np.float32)
        n = self.lib.vo_shim_walk(W, H, self._p(np.asarray(k4, np.float32)), self.C.c_float(near), self._p(np.ascontiguousarray(w2c, np.float32)),
                                  self._p(np.ascontiguousarray(seg, np.float32)), cap, self._p(ij, self.C.c_int32), self._p(z))
        return n, ij[:min(n, cap)], z[:min(n, cap)]

    def finish(self, keys, depth, occlude, fill, rgb_colors, segment_colors, bg, rgb8):
        """The header's resolve applied to a copy of ``rgb8`` [H, W, 3]."""
        C = self.C
        H, W = keys.shape
        out = np.array(rgb8, dtype=np.uint8, copy=True)
        keys = np.ascontiguousarray(keys).view(np.uint64)
        depth = None if depth is None else np.ascontiguousarray(depth, np.float32)
        rgb_colors = None if rgb_colors is None or len(rgb_colors) == 0 else np.ascontiguousarray(rgb_colors, np.float32)
        segment_colors = None if segment_colors is None or len(segment_colors) == 0 else np.ascontiguousarray(segment_colors, np.uint8)
        self.lib.vo_shim_finish(W, H, self._p(keys, C.c_uint64), self._p(depth), int(bool(occlude)), int(bool(fill)), self._p(rgb_colors),
                                0 if rgb_colors is None else len(rgb_colors), self._p(segment_colors, C.c_uint8),
                                0 if segment_colors is None else len(segment_colors), self._p(np.asarray(bg, np.float32)), self._p(out, C.c_uint8))
        return out
