"""The view overlay on the device (csrc/viewoverlay.hip through ``FusedEngine.render_view(mode="centers" / overlay=...)``,
``view.RunOverlay``, ``SlamSession.render_view(cameras=True)``, ``python -m splatam_amd.view --cameras / --mode centers`` and the
entry points themselves), held to

  * the header the kernels are made of, compiled for the host (tests/viewoverlay_math_shim.cpp, which tests/test_viewoverlay_cpu.py
    holds to the float64 restatement): the key plane EXACTLY -- it is a minimum, no order of lanes or launches can matter --, the run's
    segment arrays bit for bit, the picture's bytes exactly as the header's resolve gives them from the downloaded planes;
  * itself: the same bits on a second run, a replay of the centres against an engine that holds only those rows, a view call with an
    overlay leaves the map, its Adam state, ``variables``, the current camera's planes and the pose parameters bit-equal and allocates
    nothing after its first call.

Shapes as tests/test_gpu_view.py: 72 x 40 (partial tiles; fill and planes on 16 bytes), 70 x 37, 16 x 16, and 1 x 1 for the entry
points alone, whose outputs sit in guarded flat buffers at a 16-byte-aligned and an unaligned lead."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import view_ref
import viewoverlay_ref as R
from tests.test_gpu_view import N_GAUSSIANS, SHAPES, VIEW_POSES, _engine, _intrinsics, _sequence

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NEAR_Z = 0.01
FIRST_W2C = view_ref.rigid((0.2, 1.0, 0.1), 9.0, (0.05, -0.04, 0.1))
GUARD_K, GUARD_B, GUARD_F = 0x0123456789ABCDEF, 77, 12345.0


@pytest.fixture(scope="module")
def shim():
    return R.Shim()


def _pose_block(n, seed=3):
    """Pose parameters of ``n`` frames that keep the cameras in front of the VIEW_POSES views: small rotations, steps of a few tenths."""
    rng = np.random.default_rng(seed)
    rots = np.concatenate([np.ones((1, 1, n)), 0.15 * rng.normal(size=(1, 3, n))], axis=1).astype(np.float32) * 1.3
    trans = rng.uniform(-0.35, 0.35, size=(1, 3, n)).astype(np.float32)
    return {'cam_unnorm_rots': torch.from_numpy(rots).cuda(), 'cam_trans': torch.from_numpy(trans).cuda()}


def _overlay(W, H, n=4, gt=False, seed=3):
    from splatam_amd.view import RunOverlay
    poses = _pose_block(n, seed)
    gt_w2c = None
    if gt:
        gt_w2c = np.stack([view_ref.rigid((0.1, 1.0, 0.3), 4.0 * t, (0.2 - 0.1 * t, 0.1 * t - 0.1, 0.05 * t)) for t in range(n)])
    return RunOverlay(poses, n, first_w2c=torch.from_numpy(FIRST_W2C).cuda(), frustum_size=0.25, intrinsics=_intrinsics(W, H), size=(W, H),
                      gt_w2c=gt_w2c), poses


def _host_keys(shim, eng, view, k, P, centers, point_size, overlay, ranges, line_width):
    """The key plane the header gives for what a render_view call drew (its camera downloaded)."""
    keys = shim.keys(view.W, view.H)
    k4, w2c = _k4(k), view.w2c.cpu().numpy()
    if centers:
        shim.points(keys, k4, NEAR_Z, w2c, eng.params['means3D'].detach()[:P].cpu().numpy(), size=point_size)
    if overlay is not None:
        segments = overlay.segments.cpu().numpy()
        for first, count in ranges:
            shim.segments(keys, k4, NEAR_Z, w2c, segments, first=first, count=count, width=line_width)
    return keys


def _k4(k):
    return (k[0][0], k[1][1], k[0][2], k[1][2])


# ---------------------------------------------------------------------------------------------------------------- kernel = header
@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_key_plane_equals_the_header(shim, W, H):
    eng, params, _, k = _engine(W, H, aniso=False, seed=W)
    view = eng.view_camera(W, H)
    overlay, _ = _overlay(W, H, gt=True)
    drawn = {"points": 0, "segments": 0}
    for name in ("general", "rolled, stepped back"):
        w2c = torch.from_numpy(VIEW_POSES[name]).cuda()
        for what, mode, ov in (("points", "centers", None), ("segments", "color", overlay), ("both", "centers", overlay)):
            for size in (1, 3):
                kw = dict(w2c=w2c, intrinsics=k, mode=mode, overlay=ov, point_size=size, line_width=size, frusta="all", overlay_planes=True, near=NEAR_Z)
                with torch.no_grad():
                    first = eng.render_view(view, **kw).key.clone()
                    again = eng.render_view(view, **kw).key
                torch.cuda.synchronize()
                assert first.dtype == torch.int64 and tuple(first.shape) == (H, W) and torch.equal(first, again), (name, what, size)
                want = _host_keys(shim, eng, view, k, eng.P, mode == "centers", size, ov, ov.ranges(None, "all") if ov else (), size)
                got = first.cpu().numpy().view(np.uint64)
                _, ident, on = R.split_keys(got)
                print(f"{W}x{H} {name} {what} size {size}: {int(on.sum())} pixels drawn, {int((got != want).sum())} differ from the header")
                assert np.array_equal(got, want), (name, what, size)
                if what != "both":
                    drawn[what] += int(on.sum())
                    assert ((ident[on] & R.SEGMENT_BIT) != 0).all() == (what == "segments")
    assert drawn["points"] > 40 and drawn["segments"] > 40, drawn            # (the cases show something)


def test_parts_of_a_run(shim):
    """overlay_upto / frusta select prefixes of the blocks; the key plane is the header's over exactly those ranges."""
    W, H = 72, 40
    eng, _, _, k = _engine(W, H, aniso=False, seed=1)
    view = eng.view_camera(W, H)
    overlay, _ = _overlay(W, H, n=5, gt=True)
    n = 5
    assert overlay.ranges(None, "all") == [(0, 4), (4, 40), (44, 4)] and overlay.ranges(2, "current") == [(0, 2), (4 + 16, 8), (44, 2)]
    assert overlay.ranges(0, None) == [] and overlay.ranges(0, "current") == [(4, 8)] and overlay.num_segments == 9 * n - 1 + n - 1
    w2c = torch.from_numpy(VIEW_POSES["rolled, stepped back"]).cuda()
    planes = {}
    for upto, frusta in ((4, "all"), (2, "all"), (2, "current"), (2, None)):
        with torch.no_grad():
            key = eng.render_view(view, w2c=w2c, intrinsics=k, overlay=overlay, overlay_upto=upto, frusta=frusta, overlay_planes=True).key
        got = key.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, _host_keys(shim, eng, view, k, eng.P, False, 1, overlay, overlay.ranges(upto, frusta), 1)), (upto, frusta)
        planes[(upto, frusta)] = R.split_keys(got)[2].sum()
    assert planes[(4, "all")] > planes[(2, "all")] > planes[(2, "current")] > planes[(2, None)] > 0
    with pytest.raises(ValueError):
        eng.render_view(view, w2c=w2c, intrinsics=k, overlay=overlay, overlay_upto=5)
    with pytest.raises(ValueError):
        eng.render_view(view, w2c=w2c, intrinsics=k, mode="centers", point_size=9)


# ---------------------------------------------------------------------------------------------------------------- the run's segments
def _run_segments_kernel(lead, n, size, k4, scale, first=0, count=None, w2c_all=None, poses=None, first_w2c=None, frusta=True, fixed=None):
    """splat_view_run_segments with both outputs in guarded flat buffers; returns (segments, colors) on the host."""
    from splatam_amd import _capi
    total = n - 1 + (8 * n if frusta else 0)
    floats = torch.full((lead + 6 * total + 64,), GUARD_F, dtype=torch.float32, device="cuda")
    bytes_ = torch.full((lead + 3 * total + 64,), GUARD_B, dtype=torch.uint8, device="cuda")
    r = _capi.SplatViewRun()
    r.num_frames, r.first, r.count = n, first, n - first if count is None else count
    keep = []
    if w2c_all is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(w2c_all, np.float32)).cuda())
        r.w2c_all = keep[0].data_ptr()
    else:
        keep.append(torch.from_numpy(np.ascontiguousarray(first_w2c, np.float32)).cuda())
        r.cam_unnorm_rots, r.cam_trans, r.first_w2c = poses['cam_unnorm_rots'].data_ptr(), poses['cam_trans'].data_ptr(), keep[0].data_ptr()
    r.width, r.height = size
    r.fx, r.fy, r.cx, r.cy = k4
    r.scale, r.frusta, r.fixed_color = scale, int(frusta), int(fixed is not None)
    if fixed is not None:
        r.color[:3] = fixed
    r.segments, r.colors = floats.data_ptr() + 4 * lead, bytes_.data_ptr() + lead
    _capi.check(_capi.lib().splat_view_run_segments(C.byref(r), torch.cuda.current_stream().cuda_stream), "splat_view_run_segments")
    torch.cuda.synchronize()
    hf, hb = floats.cpu().numpy(), bytes_.cpu().numpy()
    assert (hf[:lead] == np.float32(GUARD_F)).all() and (hf[lead + 6 * total:] == np.float32(GUARD_F)).all(), "a store left the segments"
    assert (hb[:lead] == GUARD_B).all() and (hb[lead + 3 * total:] == GUARD_B).all(), "a store left the colours"
    return hf[lead:lead + 6 * total].reshape(-1, 6), hb[lead:lead + 3 * total].reshape(-1, 3)


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
def test_run_segments_kernel_equals_the_header(shim, lead):
    n, size, k4 = 5, (72, 40), (60.0, 58.0, 35.5, 19.25)
    poses = _pose_block(n, seed=11)
    host = {key: v.cpu().numpy() for key, v in poses.items()}
    # from pose parameters, with a first-frame pose that is not the identity
    got_s, got_c = _run_segments_kernel(lead, n, size, k4, 0.045, poses=poses, first_w2c=FIRST_W2C)
    want_s, want_c = shim.run(n, size, k4, rots=host['cam_unnorm_rots'], trans=host['cam_trans'], first_w2c=FIRST_W2C)
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)) and np.array_equal(got_c, want_c)
    w2cs = [FIRST_W2C.astype(np.float64) @ view_ref.rel_w2c64(host['cam_unnorm_rots'][0, :, t], host['cam_trans'][0, :, t]) for t in range(n)]
    ref_s, ref_c = R.run64(w2cs, *size, *k4, 0.045)
    assert np.abs(got_s - ref_s).max() <= view_ref.camera_bound(max(np.linalg.norm(M[:3, 3]) for M in w2cs)) and np.array_equal(got_c, ref_c)
    # from explicit matrices (the three poses of the camera tests among them), a fixed colour, the trajectory alone
    mats = np.stack([view_ref.rigid((0, 1, 0), 0.0, (0, 0, 0)), view_ref.rigid((0.3, 1.0, -0.2), 37.0, (0.4, -0.25, 1.5)),
                     view_ref.rigid((1.0, 0.2, 0.5), -112.0, (6.1, -5.3, 5.9)), VIEW_POSES["general"], VIEW_POSES["rolled, stepped back"]])
    for frusta, fixed in ((True, None), (False, (255, 255, 0)), (True, (1, 2, 3))):
        got_s, got_c = _run_segments_kernel(lead, n, size, k4, 0.3, w2c_all=mats, frusta=frusta, fixed=fixed)
        want_s, want_c = shim.run(n, size, k4, scale=0.3, w2c_all=mats, frusta=frusta, fixed=fixed)
        assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)) and np.array_equal(got_c, want_c), (frusta, fixed)
    # a range writes its own frames and nothing else: "the run up to t" is a prefix of each part
    for t in range(n):
        got_s, got_c = _run_segments_kernel(lead, n, size, k4, 0.3, count=t + 1, w2c_all=mats)
        whole_s, whole_c = shim.run(n, size, k4, scale=0.3, w2c_all=mats)
        mine = np.zeros(9 * n - 1, bool)
        mine[:t] = mine[n - 1:n - 1 + 8 * (t + 1)] = True
        assert np.array_equal(got_s[mine].view(np.uint32), whole_s[mine].view(np.uint32)) and np.array_equal(got_c[mine], whole_c[mine])
        assert (got_s[~mine] == np.float32(GUARD_F)).all() and (got_c[~mine] == GUARD_B).all()


def test_run_overlay_follows_the_pose_parameters(shim):
    """RunOverlay.refresh reads the poses as they are NOW, on the device; frames past ``upto`` keep what they held."""
    W, H = 72, 40
    overlay, poses = _overlay(W, H, n=4, gt=True)
    k4 = _intrinsics(W, H)

    def want():
        return shim.run(4, (W, H), k4, scale=0.25, rots=poses['cam_unnorm_rots'].cpu().numpy(), trans=poses['cam_trans'].cpu().numpy(), first_w2c=FIRST_W2C)
    before_s, before_c = want()
    torch.cuda.synchronize()
    assert np.array_equal(overlay.segments[:35].cpu().numpy().view(np.uint32), before_s.view(np.uint32)) and np.array_equal(overlay.colors[:35].cpu().numpy(), before_c)
    assert (overlay.colors[35:].cpu().numpy() == (255, 255, 0)).all() and np.isfinite(overlay.segments[35:].cpu().numpy()).all()
    poses['cam_trans'] += 0.125                     # (in place: the loop's optimiser steps do the same)
    allocated = torch.cuda.memory_allocated()
    overlay.refresh(1)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    after_s, _ = want()
    got = overlay.segments[:35].cpu().numpy()
    moved = np.zeros(35, bool)
    moved[:1] = moved[3:3 + 16] = True
    assert np.array_equal(got[moved].view(np.uint32), after_s[moved].view(np.uint32)) and np.array_equal(got[~moved].view(np.uint32), before_s[~moved].view(np.uint32))
    assert not np.array_equal(after_s[moved], before_s[moved])


# ---------------------------------------------------------------------------------------------------------------- the entry points alone
def _run_overlay_kernels(shim, lead, W, H, w2c, means, point_size, segments, line_width, depth, occlude, fill, rgb_colors, seg_colors, bg):
    """clear, points, segments and finish with the key plane and rgb8 in guarded flat buffers; returns (keys, rgb8) and checks both
    against the header."""
    from splatam_amd import _capi
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    k4 = _intrinsics(W, H)
    words = torch.full((lead + H * W + 16,), GUARD_K, dtype=torch.int64, device="cuda")
    bytes_ = torch.full((lead + 3 * H * W + 64,), GUARD_B, dtype=torch.uint8, device="cuda")
    dev = {name: (None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda())
           for name, a in dict(w2c=np.asarray(w2c, np.float32), means=means, segments=segments, depth=depth, rgb_colors=rgb_colors, seg_colors=seg_colors).items()}
    o = _capi.SplatViewOverlay()
    o.width, o.height, o.near_z = W, H, NEAR_Z
    o.fx, o.fy, o.cx, o.cy = k4
    o.w2c, o.keys = dev['w2c'].data_ptr(), words.data_ptr() + 8 * lead
    _capi.check(L.splat_view_overlay_clear(C.byref(o), stream), "clear")
    if means is not None:
        _capi.check(L.splat_view_points(C.byref(o), dev['means'].data_ptr(), len(means), point_size, stream), "points")
    if segments is not None:
        _capi.check(L.splat_view_segments(C.byref(o), dev['segments'].data_ptr(), 1, len(segments) - 1, line_width, stream), "segments")
    f = _capi.SplatViewOverlayFinish()
    f.depth = None if depth is None else dev['depth'].data_ptr()
    f.occlude, f.fill = int(occlude), int(fill)
    if rgb_colors is not None:
        f.rgb_colors, f.num_rows = dev['rgb_colors'].data_ptr(), len(rgb_colors)
    if seg_colors is not None:
        f.segment_colors, f.num_segments = dev['seg_colors'].data_ptr(), len(seg_colors)
    f.bg[:] = bg
    f.rgb8 = bytes_.data_ptr() + lead
    _capi.check(L.splat_view_overlay_finish(C.byref(o), C.byref(f), stream), "finish")
    torch.cuda.synchronize()
    hk, hb = words.cpu().numpy(), bytes_.cpu().numpy()
    assert (hk[:lead] == GUARD_K).all() and (hk[lead + H * W:] == GUARD_K).all(), "a store left the key plane"
    assert (hb[:lead] == GUARD_B).all() and (hb[lead + 3 * H * W:] == GUARD_B).all(), "a store left rgb8"
    keys, rgb8 = hk[lead:lead + H * W].view(np.uint64).reshape(H, W), hb[lead:lead + 3 * H * W].reshape(H, W, 3)
    want = shim.keys(W, H)
    if means is not None:
        shim.points(want, k4, NEAR_Z, w2c, means, size=point_size)
    if segments is not None:
        shim.segments(want, k4, NEAR_Z, w2c, segments, first=1, width=line_width)
    assert np.array_equal(keys, want), "the key plane is not the header's"
    before = np.full((H, W, 3), GUARD_B, np.uint8)
    assert np.array_equal(rgb8, shim.finish(keys, depth, occlude, fill, rgb_colors, seg_colors, bg, before)), "rgb8 is not the header's resolve"
    return keys, rgb8


@pytest.mark.parametrize("lead", (8, 7), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("W,H", SHAPES + ((1, 1),), ids=lambda v: str(v))
def test_entry_points_in_guarded_buffers(shim, W, H, lead):
    """Random centres and segments, with NaN, infinite and huge ones and ones behind the camera among them (inputs the kernels SKIP),
    colours out of range, a depth plane with zeros and NaN: key plane and bytes are the header's, no store leaves the buffers."""
    from tests.test_viewoverlay_cpu import to_world
    rng = np.random.default_rng(100 * W + H + lead)
    w2c = VIEW_POSES["general"]
    means = to_world(rng.uniform((-1.2, -0.8, -0.5), (1.2, 0.8, 4.0), size=(300, 3)), w2c)
    means[::37] = np.nan
    means[5], means[6], means[7] = (np.inf, 0, 1), (0, 0, -np.inf), (3e38, 3e38, 3e38)
    segments = to_world(rng.uniform((-1.5, -1.0, -0.5), (1.5, 1.0, 4.0), size=(80, 3)), w2c).reshape(40, 6)
    segments[3, 4], segments[9, 0], segments[11] = np.nan, np.inf, 3e38
    segments[12, 3:] = segments[12, :3]                                           # zero length
    rgb_colors = rng.uniform(-0.2, 1.2, size=(300, 3)).astype(np.float32)
    rgb_colors[3] = (np.nan, np.inf, -np.inf)
    seg_colors = rng.integers(0, 256, size=(40, 3)).astype(np.uint8)
    depth = rng.uniform(0.5, 4.0, size=(H, W)).astype(np.float32)
    depth.reshape(-1)[::5] = 0.0
    depth.reshape(-1)[::11] = np.nan
    for point_size, line_width, occlude, fill, with_depth in ((1, 1, True, False, True), (3, 3, True, True, False), (8, 4, False, False, True), (2, 2, True, True, True)):
        keys, rgb8 = _run_overlay_kernels(shim, lead, W, H, w2c, means, point_size, segments, line_width, depth if with_depth else None, occlude, fill,
                                          rgb_colors, seg_colors, (0.25, 0.5, 1.0))
        if (W, H) != (1, 1):
            _, ident, on = R.split_keys(keys)
            assert (ident[on] & R.SEGMENT_BIT).astype(bool).any() and (~(ident[on] & R.SEGMENT_BIT).astype(bool)).any()
            assert fill or point_size > 3 or (rgb8 == GUARD_B).all(axis=2).any()   # (without fill, pixels nothing is drawn on keep what they held)
    # the resolve alone: nothing drawn, and ids past the end of their arrays
    _run_overlay_kernels(shim, lead, W, H, w2c, None, 1, None, 1, depth, True, False, None, None, (0.0, 0.0, 0.0))
    _run_overlay_kernels(shim, lead, W, H, w2c, means, 2, segments, 2, None, True, True, rgb_colors[:7], seg_colors[:5], (1.0, 1.0, 1.0))


# ---------------------------------------------------------------------------------------------------------------- the picture's bytes
@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_bytes_are_the_headers_resolve_of_the_downloaded_planes(shim, W, H):
    eng, _, _, k = _engine(W, H, aniso=False, seed=W + 1)
    view = eng.view_camera(W, H)
    overlay, _ = _overlay(W, H, gt=True)
    w2c = torch.from_numpy(VIEW_POSES["rolled, stepped back"]).cuda()
    seg_colors = overlay.colors.cpu().numpy()
    for mode in ("color", "depth", "sil", "centers"):
        for bg, occlude in (((1.0, 1.0, 1.0), True), ((0.1, 0.2, 0.3), False)):
            with torch.no_grad():
                before = None if mode == "centers" else eng.render_view(view, w2c=w2c, intrinsics=k, mode=mode, background=bg).rgb8.cpu().numpy()
                image = eng.render_view(view, w2c=w2c, intrinsics=k, mode=mode, background=bg, overlay=overlay, line_width=2, point_size=2,
                                        occlude=occlude, overlay_planes=True)
            torch.cuda.synchronize()
            keys, got = image.key.cpu().numpy().view(np.uint64), image.rgb8.cpu().numpy()
            if mode == "centers":
                want = shim.finish(keys, None, occlude, True, eng.params['rgb_colors'].detach().cpu().numpy(), seg_colors, bg, np.zeros((H, W, 3), np.uint8))
            else:
                want = shim.finish(keys, image.out6[3].cpu().numpy(), occlude, False, None, seg_colors, bg, before)
                assert (got != before).any(), "the overlay changed nothing: the case shows nothing"
            assert np.array_equal(got, want), (mode, bg, occlude)
            assert np.array_equal(got, R.resolve64(keys, None if mode == "centers" else image.out6[3].cpu().numpy(), occlude, mode == "centers",
                                                   eng.params['rgb_colors'].detach().cpu().numpy() if mode == "centers" else [], seg_colors, bg,
                                                   np.zeros((H, W, 3), np.uint8) if before is None else before)), (mode, "the plain numpy form")


def _wall_engine(W, H):
    """An opaque wall at z = 2 in front of the identity camera: a grid of fat Gaussians."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    fx, fy, cx, cy = _intrinsics(W, H)
    params, variables = slam.synthetic_params(N_GAUSSIANS, W, H, fx, fy, cx, cy, num_frames=3, seed=0, device="cuda")
    u, v = np.meshgrid(np.linspace(-4, W + 3, 25), np.linspace(-4, H + 3, 16))
    pts = np.stack([(u.ravel() - cx) / fx * 2.0, (v.ravel() - cy) / fy * 2.0, np.full(u.size, 2.0)], axis=1).astype(np.float32)
    with torch.no_grad():
        params['means3D'][:] = torch.from_numpy(pts).cuda()
        params['logit_opacities'][:] = 8.0
        params['log_scales'][:] = float(np.log(0.09))
    k = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
    cam = slam.setup_camera(W, H, k, np.eye(4, dtype=np.float32), device="cuda")
    with torch.no_grad():
        return FusedEngine(params, cam, variables=variables), k


def test_a_segment_through_a_wall_is_hidden_behind_it(shim):
    W, H = 72, 40
    assert N_GAUSSIANS == 25 * 16
    eng, k = _wall_engine(W, H)
    view = eng.view_camera(W, H)
    fx, fy, cx, cy = _intrinsics(W, H)
    overlay, _ = _overlay(W, H, n=2)
    a, b = ((8.3 - cx) / fx * 1.0, (30.2 - cy) / fy * 1.0, 1.0), ((63.6 - cx) / fx * 3.0, (9.4 - cy) / fy * 3.0, 3.0)
    with torch.no_grad():
        overlay.segments[0] = torch.tensor(a + b, device="cuda")
        overlay.colors[0] = torch.tensor([255, 0, 255], dtype=torch.uint8, device="cuda")
        w2c = torch.eye(4, device="cuda")
        plain = eng.render_view(view, w2c=w2c, intrinsics=k).rgb8.cpu().numpy()
        seen = {}
        for occlude in (True, False):
            image = eng.render_view(view, w2c=w2c, intrinsics=k, overlay=overlay, frusta=None, occlude=occlude, overlay_planes=True)
            seen[occlude] = (image.rgb8.cpu().numpy(), image.key.cpu().numpy().view(np.uint64), image.out6[3:5].cpu().numpy())
    rgb8, keys, (depth, sil) = seen[True]
    z, _, on = R.split_keys(keys)
    assert (sil[on] > 0.99).all() and np.abs(depth[on] - 2.0).max() < 0.05, "the wall is not opaque at z = 2 where the segment runs"
    assert 50 <= on.sum() <= 60 and z[on].min() < 1.1 and z[on].max() > 2.9
    magenta = (rgb8 == (255, 0, 255)).all(axis=2)
    want = on & ((z <= depth) | (depth <= 0))
    assert np.array_equal(magenta, want) and np.array_equal(rgb8[~want], plain[~want])
    assert 10 <= want.sum() <= on.sum() - 10                                     # part of it in front, part of it hidden (1 / z is linear: z = 2 lies three quarters along)
    rgb8_all, keys_all, _ = seen[False]
    assert np.array_equal(keys_all, keys) and np.array_equal((rgb8_all == (255, 0, 255)).all(axis=2), on)


# ---------------------------------------------------------------------------------------------------------------- replay
def test_centres_replay_shows_the_rows_up_to_a_time_step():
    from splatam_amd.fused import FusedEngine, PARAM_ORDER
    from tests.test_gpu_view import _map
    W, H = 72, 40
    params, variables, k, cam = _map(W, H, aniso=False, seed=9)
    variables['timestep'] = torch.tensor([0.0] * 150 + [1.0] * 130 + [3.0] * 120, device="cuda")
    w2c = torch.from_numpy(VIEW_POSES["general"]).cuda()
    with torch.no_grad():
        eng = FusedEngine(params, cam, variables=variables)
        view = eng.view_camera(W, H)
        pictures = []
        for t, rows in ((0, 150), (1, 280), (2, 280), (3, 400)):
            got = eng.render_view(view, w2c=w2c, intrinsics=k, mode="centers", max_timestep=t, point_size=2, overlay_planes=True)
            got = (got.rgb8.clone(), got.key.clone())
            part = {key: (v.detach()[:rows].contiguous() if key in PARAM_ORDER else v.detach()) for key, v in params.items()}
            small = FusedEngine(part, cam)
            want = small.render_view(small.view_camera(W, H), w2c=w2c, intrinsics=k, mode="centers", point_size=2, overlay_planes=True)
            torch.cuda.synchronize()
            assert torch.equal(got[0], want.rgb8) and torch.equal(got[1], want.key), t
            assert int((got[1] >= 0).sum()) > 100 and int(got[1][got[1] >= 0].bitwise_and(0xFFFFFFFF).max()) < rows
            pictures.append(got[0])
        assert torch.equal(pictures[1], pictures[2]) and not torch.equal(pictures[0], pictures[1]) and not torch.equal(pictures[2], pictures[3])


# ---------------------------------------------------------------------------------------------------------------- read-only, in place
def test_an_overlay_leaves_the_loop_as_it_was_and_allocates_once():
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine, PARAM_ORDER
    from splatam_amd.view import RunOverlay
    from tests.test_gpu_fused import _scene
    W, H = 72, 40
    params, variables, frame, cam = _scene(N_GAUSSIANS, W, H, seed=4)
    f = 0.5 * W
    k = [[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]]
    with torch.no_grad():
        eng = FusedEngine(params, cam, gaussian_capacity=1024, variables=variables)
        for _ in range(3):
            eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
        assert not eng.check_overflow()
        eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
        torch.cuda.synchronize()
        main = eng._camera

        def snapshot():
            s = {f"param {n}": eng.params[n].detach().clone() for n in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
            s.update({f"exp_avg {n}": eng.exp_avg[n].clone() for n in PARAM_ORDER})
            s.update({f"exp_avg_sq {n}": eng.exp_avg_sq[n].clone() for n in PARAM_ORDER})
            s.update({f"variables {n}": eng.variables[n].clone() for n in ('max_2D_radius', 'timestep', 'means2D_gradient_accum', 'denom')})
            s.update({f"main {n}": main.buf[n].clone() for n in ('out6', 'status', 'tile_order', 'd_cam')})
            return s
        before = snapshot()
        assert float(before["exp_avg means3D"].abs().max()) > 0
        view = eng.view_camera(W, H)
        w2c = torch.from_numpy(VIEW_POSES["general"]).cuda()
        overlay = RunOverlay(eng, eng.num_frames, frustum_size=0.3, intrinsics=k, size=(W, H))
        plain = eng.render_view(view, w2c=w2c, intrinsics=k).rgb8.clone()
        first = eng.render_view(view, w2c=w2c, intrinsics=k, overlay=overlay, overlay_planes=True)         # (allocates the key plane)
        torch.cuda.synchronize()
        assert not torch.equal(first.rgb8, plain)
        elsewhere = torch.from_numpy(VIEW_POSES["rolled, stepped back"]).cuda()          # (the caller's pose: made before the count is taken)
        allocated = torch.cuda.memory_allocated()
        ptrs = (first.rgb8.data_ptr(), first.key.data_ptr(), first.out6.data_ptr())
        for kw in (dict(mode="centers", point_size=3), dict(mode="depth", overlay=overlay, frusta="current", overlay_upto=1, line_width=3),
                   dict(mode="sil", overlay=overlay, occlude=False), dict(mode="centers", overlay=overlay.refresh(), background=(1.0, 1.0, 1.0))):
            again = eng.render_view(view, w2c=elsewhere, intrinsics=k, overlay_planes=True, **kw)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == allocated, kw
            assert (again.rgb8.data_ptr(), again.key.data_ptr(), again.out6.data_ptr()) == ptrs
        # an overlay with nothing to draw: the picture of the call without one
        empty = eng.render_view(view, w2c=w2c, intrinsics=k, overlay=overlay, overlay_upto=0, frusta=None, overlay_planes=True)
        torch.cuda.synchronize()
        assert torch.equal(empty.rgb8, plain) and bool((empty.key == -1).all())
        assert eng._camera is main
        after = snapshot()
        for name, t in before.items():
            bits = (lambda x: x.view(torch.int32)) if t.dtype == torch.float32 else (lambda x: x)
            assert torch.equal(bits(t), bits(after[name])), name
        eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)                # ... and the loop goes on
        torch.cuda.synchronize()
        assert not eng.check_overflow()


# ---------------------------------------------------------------------------------------------------------------- session, tool
def _cool_pixels(picture):
    p = np.asarray(picture).astype(int).reshape(-1, 3)
    return int(((p[:, 2] == 255) & (p[:, 0] + p[:, 1] == 255)).sum())


def test_session_draws_its_own_run():
    from splatam_amd.session import SlamSession
    ds, cfg = _sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    with SlamSession(cfg, len(ds)) as session:
        for t in range(len(ds)):
            session.add_frame(*ds[t])
            before = {n: session.params[n].detach().clone() for n in session.params}
            plain = session.render_view(follow=True, background=(1.0, 1.0, 1.0)).rgb8.clone()
            image = session.render_view(follow=True, background=(1.0, 1.0, 1.0), cameras=True, occlude=False, line_width=2)
            torch.cuda.synchronize()
            assert tuple(image.rgb8.shape) == (40, 72, 3) and int(image.truncated) == 0
            picture = image.rgb8.cpu().numpy()
            assert _cool_pixels(picture) > 0 and _cool_pixels(plain.cpu().numpy()) == 0, t      # the current frustum, half a metre ahead
            for n, p in before.items():
                assert torch.equal(p, session.params[n].detach()), n
        both = session.render_view(follow=True, cameras=True, frusta="all", occlude=False, mode="centers")
        assert _cool_pixels(both.rgb8.cpu().numpy()) > 0
        session.finish()


def test_the_tool_draws_centres_and_cameras(tmp_path):
    from PIL import Image
    from splatam_amd import pipeline
    ds, cfg = _sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    params, variables, stats = pipeline.rgbd_slam(ds, cfg, engine="fused")
    out = {n: v for n, v in params.items()}
    out['timestep'] = variables['timestep']
    out['intrinsics'] = ds[0][2][:3, :3].cpu().numpy()
    out['w2c'] = torch.linalg.inv(ds[0][3]).cpu().numpy()
    out['org_width'], out['org_height'] = 72, 40
    path = pipeline.save_params(out, str(tmp_path / "run"))
    pictures = tmp_path / "pictures"
    root = os.path.dirname(HERE)
    done = subprocess.run([sys.executable, "-m", "splatam_amd.view", path, "--out", str(pictures), "--mode", "centers", "--cameras", "--replay",
                           "--size", "36x20", "--point-size", "2", "--no-occlude"],
                          cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    assert sorted(os.listdir(pictures)) == [f"view_{t:04d}.png" for t in range(3)], done.stdout
    for name in os.listdir(pictures):
        picture = np.asarray(Image.open(pictures / name))
        assert picture.shape == (20, 36, 3) and picture.min() != picture.max()
        assert _cool_pixels(picture) > 0, name
