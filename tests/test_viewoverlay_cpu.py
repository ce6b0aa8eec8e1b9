"""The view overlay without a GPU: splatam_amd/csrc/viewoverlay_math.h compiled for the host (tests/viewoverlay_math_shim.cpp: plain-loop
models of the four kernels of csrc/viewoverlay.hip) against the float64 numpy restatement tests/viewoverlay_ref.py.

RUN (frusta, trajectory): every coordinate within ``view_ref.camera_bound`` = 4 * 2^-24 * (1 + |t|) of the float64 form -- the view
layer's camera bound, by the same argument: evaluated in double, rounded once.  Colours exactly.
SEGMENT: the covered pixels equal the restatement's except where it calls a pixel fragile (a float64 position within 1e-4 px of the
boundary at which it rounds elsewhere), which it may do on at most ``R.MAX_EXCUSED`` = 1 % of a case's covered pixels -- asserted: the
inputs are fixed and chosen so; depths of agreeing pixels within ``R.DEPTH_RTOL`` (derived in the ref file).
POINT, RESOLVE: exactly, on inputs away from rounding boundaries."""
import os
import subprocess

import numpy as np
import pytest

import view_ref
import viewoverlay_ref as R
from tests.test_view_math_cpu import POSES

SHAPES = ((72, 40), (70, 37), (16, 16), (1, 1))
NEAR_Z = 0.01
W2C = view_ref.rigid((1.0, 2.0, 3.0), 12.0, (0.15, -0.1, 0.6))


@pytest.fixture(scope="module")
def shim():
    return R.Shim()


def intrinsics(W, H):
    f = 0.8 * W
    return f, f + 1.5, W / 2 - 0.5, H / 2 - 0.25


def to_world(cam_points, w2c=W2C):
    """Camera-space points [., 3] as float32 world points through the float64 inverse of ``w2c``."""
    c2w = np.linalg.inv(np.asarray(w2c, np.float64))
    p = np.asarray(cam_points, np.float64).reshape(-1, 3)
    return (p @ c2w[:3, :3].T + c2w[:3, 3]).astype(np.float32)


def pixel_at(W, H, u, v, z):
    fx, fy, cx, cy = intrinsics(W, H)
    return ((u - cx) / fx * z, (v - cy) / fy * z, z)


def segment_cases(W, H):
    """name -> (segment as 6 float32 world coordinates, whether it must cover something on a picture larger than one pixel)."""
    def px(u0, v0, z0, u1, v1, z1):
        return to_world([pixel_at(W, H, u0, v0, z0), pixel_at(W, H, u1, v1, z1)]).reshape(6)
    nan = np.float32(np.nan)
    inside = px(0.37 * W + 0.21, 0.58 * H + 0.13, 1.7, 0.37 * W + 0.21, 0.58 * H + 0.13, 1.7)
    return {
        "along x": (px(0.1 * W + 0.37, 0.4 * H + 0.2, 2.0, 0.9 * W + 0.13, 0.4 * H + 0.2, 2.0), True),
        "along y": (px(0.3 * W + 0.27, 0.1 * H + 0.2, 1.5, 0.3 * W + 0.27, 0.9 * H + 0.17, 1.5), True),
        "diagonal": (px(0.1 * W + 0.13, 0.15 * H + 0.21, 1.2, 0.1 * W + 0.13 + 0.72 * H, 0.85 * H + 0.21, 3.1), True),     # (45 degrees but for a few percent: an exact tie of the extents is the next test's)
        "steep": (px(0.4 * W + 0.1, 0.05 * H + 0.3, 3.0, 0.55 * W + 0.2, 0.95 * H - 0.3, 1.1), True),
        "shallow": (px(0.05 * W + 0.23, 0.5 * H + 0.11, 1.0, 0.95 * W - 0.29, 0.6 * H + 0.17, 4.0), True),
        "across the near plane": (to_world([(-0.2, 0.1, -0.5), (0.31, -0.1, 2.0)]).reshape(6), True),
        "behind the near plane": (to_world([(-0.2, 0.1, -1.0), (0.3, -0.1, -2.0)]).reshape(6), False),
        "outside the image": (px(2.0 * W, 2.0 * H, 2.0, 3.0 * W, 2.5 * H, 2.0), False),
        "across a corner": (px(-0.2 * W - 0.13, 0.3 * H + 0.07, 2.0, 0.3 * W + 0.19, -0.2 * H - 0.11, 2.5), True),
        "zero length": (inside, True),
        "nan endpoint": (np.concatenate([inside[:3], [nan, inside[4], inside[5]]]).astype(np.float32), False),
    }


# ---------------------------------------------------------------------------------------------------------------- RUN
def _check_run(got_s, got_c, w2cs64, size, k4, what, frusta=True, fixed=None):
    want_s, want_c = R.run64(w2cs64, size[0], size[1], *k4, 0.045, frusta=frusta, fixed=fixed)
    n = len(w2cs64)
    t_norm = [np.linalg.norm(np.asarray(M, np.float64)[:3, 3]) for M in w2cs64]
    bound = np.array([view_ref.camera_bound(max(t_norm[j], t_norm[j + 1])) for j in range(n - 1)]
                     + ([view_ref.camera_bound(t_norm[t]) for t in range(n) for _ in range(8)] if frusta else []))
    err = np.abs(got_s.astype(np.float64) - want_s).max(axis=1)
    print(f"{what}: max |coordinate - float64| / bound {float((err / bound).max()) if len(err) else 0.0:.3f}")
    assert got_s.shape == want_s.shape and np.isfinite(got_s).all() and (err <= bound).all(), (what, err, bound)
    assert np.array_equal(got_c, want_c), what


def test_frusta_and_trajectory_of_the_three_poses(shim):
    size, k4 = (72, 40), (60.0, 58.0, 35.5, 19.25)
    mats = np.stack([POSES[name] for name in ("identity", "general", "far")])
    seg, col = shim.run(3, size, k4, w2c_all=mats)
    _check_run(seg, col, [m.astype(np.float64) for m in mats], size, k4, "identity, general, far")
    # the identity camera's frustum, from the definition: apex at the origin, corner (0, 0) at K^-1 (0, 0, 1) 0.045
    assert np.array_equal(seg[2, :3], np.zeros(3, np.float32))
    assert np.allclose(seg[2, 3:], [(0 - 35.5) / 60.0 * 0.045, (0 - 19.25) / 58.0 * 0.045, 0.045], rtol=1e-6)
    line, line_col = shim.run(3, size, k4, w2c_all=mats, frusta=False, fixed=(255, 255, 0))
    _check_run(line, line_col, [m.astype(np.float64) for m in mats], size, k4, "the trajectory alone", frusta=False, fixed=(255, 255, 0))
    assert np.array_equal(line, seg[:2])


def test_run_of_five_frames_from_pose_parameters(shim):
    size, k4, n = (72, 40), (60.0, 58.0, 35.5, 19.25), 5
    rng = np.random.default_rng(7)
    rots = (rng.normal(size=(1, 4, n)) * 1.7).astype(np.float32)
    trans = rng.uniform(-2, 2, size=(1, 3, n)).astype(np.float32)
    first = POSES["general"]
    w2cs = [first.astype(np.float64) @ view_ref.rel_w2c64(rots[0, :, t], trans[0, :, t]) for t in range(n)]
    seg, col = shim.run(n, size, k4, rots=rots, trans=trans, first_w2c=first)
    _check_run(seg, col, w2cs, size, k4, "five frames")
    assert len(seg) == 9 * n - 1
    # colours: the trajectory runs over the upper half of cool, the frusta over its lower half
    lut = R.cool_lut64()
    assert np.array_equal(col[:n - 1], lut[[128, 160, 192, 224]]) and np.array_equal(col[n - 1::8], lut[[0, 25, 51, 76, 102]])
    # a range rebuilds its own frames only, and a prefix of each part is the run up to t
    part_s, part_c = np.full_like(seg, 5.0), np.full_like(col, 9)
    shim.run(n, size, k4, rots=rots, trans=trans, first_w2c=first, first=2, count=2, segments=part_s, colors=part_c)
    written = np.zeros(len(seg), bool)
    written[[1, 2]] = True
    written[n - 1 + 16:n - 1 + 32] = True
    assert np.array_equal(part_s[written], seg[written]) and (part_s[~written] == 5.0).all() and (part_c[~written] == 9).all()
    for t in range(n):
        upto_s, _ = shim.run(n, size, k4, rots=rots, trans=trans, first_w2c=first, count=t + 1)
        assert np.array_equal(upto_s[:t], seg[:t]) and np.array_equal(upto_s[n - 1:n - 1 + 8 * (t + 1)], seg[n - 1:n - 1 + 8 * (t + 1)])
        assert np.isnan(upto_s[t:n - 1]).all() and np.isnan(upto_s[n - 1 + 8 * (t + 1):]).all()


def test_cool_table(shim):
    from splatam_amd.view import cool_lut
    lut = cool_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    i = np.arange(256)
    assert np.array_equal(lut, R.cool_lut64())
    assert np.array_equal(lut, np.stack([i, 255 - i, np.full(256, 255)], axis=1))
    for k in range(256):
        for x in (k / 256.0, (k + 0.5) / 256.0, np.nextafter((k + 1) / 256.0, 0.0)):
            assert np.array_equal(shim.cool(x), lut[k]), (k, x)
    assert np.array_equal(shim.cool(1.0), lut[255]) and np.array_equal(shim.cool(-0.5), lut[0]) and np.array_equal(shim.cool(np.nan), lut[0])
    try:
        from matplotlib import pyplot as plt
    except ImportError:
        return
    table = plt.get_cmap('cool')(np.arange(256))[:, :3]                 # (floats: its own bytes truncate, ours round like view_byte)
    assert np.abs(table - np.stack([i / 255, 1 - i / 255, np.ones(256)], axis=1)).max() <= 1e-15
    assert np.array_equal(lut, np.rint(table * 255).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- SEGMENT
def _segment_plane(shim, W, H, seg, width, index=0):
    keys = shim.keys(W, H)
    pad = np.zeros((index + 1, 6), np.float32)
    pad[index] = seg
    steps = shim.segments(keys, intrinsics(W, H), NEAR_Z, W2C, pad, first=index, count=1, width=width)
    return keys, steps


@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_segment_raster_against_the_float64_restatement(shim, W, H, width):
    for name, (seg, covers) in segment_cases(W, H).items():
        keys, steps = _segment_plane(shim, W, H, seg, width, index=3)
        z, ident, drawn = R.split_keys(keys)
        want, fragile, _ = R.line64(seg, W2C, W, H, *intrinsics(W, H), NEAR_Z, width)
        assert steps <= max(W, H) + 1
        assert (ident[drawn] == (R.SEGMENT_BIT | 3)).all()
        got = {(int(i), int(j)) for j, i in np.argwhere(drawn)}
        differ = got ^ set(want)
        excused = len(fragile & (got | set(want)))
        print(f"{W}x{H} width {width} {name}: {len(want)} pixels, {len(differ)} differ, {excused} fragile")
        assert differ <= fragile, (name, sorted(differ - fragile)[:5])
        assert excused <= R.MAX_EXCUSED * len(want), (name, excused, len(want))          # the condition on the INPUTS
        if covers and (W, H) != (1, 1):
            assert len(want) >= (1 if name == "zero length" else 3), name
        if not covers:
            assert not want and not got, name
        for (i, j) in got & set(want):
            if (i, j) not in fragile:
                assert abs(float(z[j, i]) - want[(i, j)]) <= R.DEPTH_RTOL * want[(i, j)], (name, i, j)
        if name == "zero length" and want:
            assert len(got) == min(width, W) * 1 or len(got) <= width
        if name == "across the near plane" and want:
            assert float(z[drawn].min()) >= NEAR_Z * (1 - 1e-6)


@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_segment_walks_have_no_gaps_stay_inside_and_do_not_depend_on_direction(shim, W, H):
    k4 = intrinsics(W, H)
    cases = segment_cases(W, H)
    rng = np.random.default_rng(W + H)
    extra = {f"random {n}": (to_world(rng.uniform((-1.5, -1.0, -0.5), (1.5, 1.0, 4.0), size=(2, 3))).reshape(6), None) for n in range(40)}
    exact45 = to_world([pixel_at(W, H, 2.0, 3.0, 2.0), pixel_at(W, H, 2.0 + 0.6 * min(W, H), 3.0 + 0.6 * min(W, H), 2.0)], np.eye(4)).reshape(6)
    for name, (seg, _) in dict(cases, **extra).items():
        n, ij, z = shim.walk(W, H, k4, NEAR_Z, W2C, seg)
        assert 0 <= n <= max(W, H) + 1, name
        if n > 1:
            assert np.abs(np.diff(ij, axis=0)).max() <= 1, name                       # no gaps
            assert (np.abs(np.diff(ij, axis=0)).max(axis=1) == 1).all(), name         # ... and one major pixel per step
        assert np.isfinite(z).all() and (z >= np.float32(NEAR_Z) * (1 - 1e-6)).all(), name
        rev = np.concatenate([seg[3:], seg[:3]])
        for width in (1, 3, 4):
            # the plane sits in a guarded buffer: a pixel outside the image would be a store outside the plane
            buf = np.full(H * W + 64, 0x1234, np.uint64)
            fwd = buf[32:32 + H * W].reshape(H, W)
            fwd[:] = R.NO_KEY
            shim.segments(fwd, k4, NEAR_Z, W2C, seg[None], width=width)
            assert (buf[:32] == 0x1234).all() and (buf[32 + H * W:] == 0x1234).all(), name
            back = shim.keys(W, H)
            shim.segments(back, k4, NEAR_Z, W2C, rev[None], width=width)
            assert np.array_equal(fwd, back), (name, width)                           # bit for bit
    # an exact diagonal through the identity camera: the tie goes to x, both directions alike
    fwd, back = shim.keys(W, H), shim.keys(W, H)
    shim.segments(fwd, k4, NEAR_Z, np.eye(4), exact45[None])
    shim.segments(back, k4, NEAR_Z, np.eye(4), np.concatenate([exact45[3:], exact45[:3]])[None])
    assert np.array_equal(fwd, back)


# ---------------------------------------------------------------------------------------------------------------- POINT
@pytest.mark.parametrize("W,H", SHAPES[:3], ids=lambda v: str(v))
def test_point_footprints(shim, W, H):
    k4 = intrinsics(W, H)
    spots = {"inside": (0.4 * W + 0.2, 0.6 * H + 0.37, 2.0), "left edge": (0.2, 0.5 * H + 0.1, 1.5), "corner": (W - 0.8, H - 0.7, 3.0),
             "top edge": (0.5 * W + 0.3, -0.3, 1.0), "just outside": (W + 0.2, 0.5 * H + 0.2, 2.0), "far outside": (5.0 * W, 0.2, 2.0)}
    for size in (1, 2, 5):
        for name, (u, v, zc) in spots.items():
            p = to_world([pixel_at(W, H, u, v, zc)])
            keys = shim.points(shim.keys(W, H), k4, NEAR_Z, W2C, np.concatenate([np.zeros((4, 3), np.float32) + 1e6, p]), size=size)
            z, ident, drawn = R.split_keys(keys)
            want, z64, fragile = R.point64(p[0], W2C, W, H, *k4, NEAR_Z, size)
            assert not fragile, (name, "a test input on a rounding boundary")
            got = {(int(i), int(j)) for j, i in np.argwhere(drawn & (ident == 4))}
            assert got == set(want), (size, name, got, want)
            if name in ("inside",):
                assert len(got) == size * size
            if name == "far outside":
                assert not got
            for i, j in got:
                assert abs(float(z[j, i]) - z64) <= 4 * 2.0 ** -24 * (1.0 + np.abs(W2C[2]).sum() * np.abs(p).max()), name     # four float32 roundings of mr_cam_coord
    # at and behind the near plane, non-finite centres: nothing
    nothing = np.concatenate([to_world([(0.0, 0.0, NEAR_Z * 0.5), (0.0, 0.0, -1.0)]),
                              np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [3e38, 3e38, 3e38]], np.float32)])
    assert (shim.points(shim.keys(W, H), k4, NEAR_Z, W2C, nothing, size=5) == R.NO_KEY).all()
    exactly_near = np.array([[0.0, 0.0, NEAR_Z]], np.float32)
    assert (shim.points(shim.keys(W, H), k4, np.float32(NEAR_Z), np.eye(4), exactly_near) == R.NO_KEY).all()       # z > near, not >=


def test_equal_depths_resolve_to_the_lowest_id_and_points_win(shim):
    W, H = 16, 16
    k4, eye = intrinsics(W, H), np.eye(4, dtype=np.float32)
    p = np.array(pixel_at(W, H, 5.0, 6.0, 2.0), np.float32)
    means = np.stack([p * 0 + 1e6, p, p, p])                   # rows 1, 2, 3 share a pixel and a depth
    for order in ((0, 1, 2, 3), (3, 2, 1, 0)):
        keys = shim.keys(W, H)
        for row in order:                                      # (entered one at a time in either order: a minimum)
            one = np.full((4, 3), 1e6, np.float32)
            one[row] = means[row]
            shim.points(keys, k4, NEAR_Z, eye, one)
        z, ident, drawn = R.split_keys(keys)
        assert drawn.sum() == 1 and ident[6, 5] == 1 and z[6, 5] == np.float32(2.0)
    # a segment through the same pixel at the same depth bits: the point keeps the pixel, the segment its others
    seg = np.concatenate([pixel_at(W, H, 2.0, 6.0, 2.0), pixel_at(W, H, 9.0, 6.0, 2.0)]).astype(np.float32)
    for first in ("points", "segments"):
        keys = shim.keys(W, H)
        if first == "points":
            shim.points(keys, k4, NEAR_Z, eye, means)
        shim.segments(keys, k4, NEAR_Z, eye, seg[None])
        if first == "segments":
            shim.points(keys, k4, NEAR_Z, eye, means)
        z, ident, drawn = R.split_keys(keys)
        assert z[6, 5] == np.float32(2.0) and z[6, 4] == np.float32(2.0), "the segment's depth bits are not the point's: the case shows nothing"
        assert ident[6, 5] == 1 and ident[6, 4] == R.SEGMENT_BIT and drawn[6].sum() == 8


# ---------------------------------------------------------------------------------------------------------------- RESOLVE
def _key(z, ident):
    return (int(np.array([z], np.float32).view(np.uint32)[0]) << 32) | ident


def test_resolve_visibility_and_bytes(shim):
    W, H = 8, 2
    keys = shim.keys(W, H)
    depth = np.zeros((H, W), np.float32)
    seg_colors = np.array([[10, 20, 30], [200, 100, 50]], np.uint8)
    colours = np.array([[0.25, 0.5, 1.0], [-0.5, 1.5, np.nan], [np.inf, -np.inf, 0.4]], np.float32)
    # row 0: a segment at z = 2 in front of, at, behind the scene, over no scene, over a NaN depth; then points
    for i, d in enumerate((3.0, 2.0, 1.0, 0.0, np.nan, -1.0)):
        keys[0, i], depth[0, i] = _key(2.0, R.SEGMENT_BIT | 1), d
    for i in range(3):
        keys[1, i], depth[1, i] = _key(2.0, i), 5.0
    keys[1, 3], keys[1, 4] = _key(2.0, 3), _key(2.0, R.SEGMENT_BIT | 2)          # ids past the end of their arrays
    before = np.full((H, W, 3), 77, np.uint8)
    for occlude in (True, False):
        for fill in (False, True):
            bg = (1.0, 0.0, 0.5)
            got = shim.finish(keys, depth, occlude, fill, colours, seg_colors, bg, before)
            assert np.array_equal(got, R.resolve64(keys, depth, occlude, fill, colours, seg_colors, bg, before)), (occlude, fill)
            rest = [255, 0, 128] if fill else [77, 77, 77]
            seen = [True, True, False, True, False, True] if occlude else [True] * 6
            for i, s in enumerate(seen):
                assert got[0, i].tolist() == ([200, 100, 50] if s else rest), (occlude, fill, i)
            assert got[1, 0].tolist() == [64, 128, 255] and got[1, 1].tolist() == [0, 255, 0] and got[1, 2].tolist() == [255, 0, 102]
            assert (got[1, 3:] == rest).all() and (got[0, 6:] == rest).all()
    # no scene at all (the centres picture): everything drawn
    got = shim.finish(keys, None, True, True, colours, seg_colors, (0.0, 0.0, 0.0), before)
    assert (got[0, :6] == [200, 100, 50]).all() and (got[0, 6:] == 0).all()
    # an empty plane changes nothing
    assert np.array_equal(shim.finish(shim.keys(W, H), depth, True, False, colours, seg_colors, (1.0, 1.0, 1.0), before), before)


# ---------------------------------------------------------------------------------------------------------------- sanitizers
def test_header_under_address_and_ub_sanitizers(tmp_path):
    """The shim's loops as a stand-alone program (its own main) built with -fsanitize=address,undefined: NaN, infinite and huge
    endpoints and centres, segments behind and across the near plane, every width and point size, the four sizes, keys that name rows
    and segments past the end, colours out of range, runs from pose parameters (a zero quaternion among them) and from matrices.  Any
    sanitizer report or failed expectation is a non-zero exit.  The runtimes are linked statically; nothing loaded into python is
    involved."""
    exe = str(tmp_path / "viewoverlay_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DVIEWOVERLAY_SHIM_MAIN", "-o", exe,
                           os.path.join(os.path.dirname(__file__), "viewoverlay_math_shim.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
