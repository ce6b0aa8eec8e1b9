"""The view layer on the device (csrc/view.hip through ``FusedEngine.view_camera`` / ``render_view``, ``fused.view_finish``,
``SlamSession.render_view``, ``evaluation.evaluate(save_frames=True)`` and ``python -m splatam_amd.view``), held to

  * the float64 restatement tests/view_ref.py: the camera at the bound of tests/test_view_math_cpu.py (4 * 2^-24 * (1 + |t|)), the
    bytes by its boundary rule, the cloud within TWICE the deviation of the torch float32 form of rgbd2pcd on the same planes;
  * the CPU oracle (oracle/raster_ref.c) for the planes of views that are NOT poses of the map: 1e-4 on colour, 1e-4 + 1e-4 |ref| on
    depth / silhouette / depth^2, every element beyond it explained by the float64 oracle's account of that pixel
    (tests/util.py assert_outliers_explained, as the fused iteration's planes are checked);
  * itself: a replay at ``max_timestep = t`` against an engine that holds only those rows, bit for bit; a view render leaves the
    map, its Adam state, ``variables`` and the current camera's planes bit-equal and allocates nothing after the first call.

Shapes: 72 x 40 (5 x 3 tiles, partial right and bottom tiles, 16-byte path), 70 x 37 (scalar path), 16 x 16 (one tile), and 1 x 1 for
the finish kernel alone.  Outputs of the two kernels sit in guarded flat buffers at a 16-byte-aligned and an unaligned lead."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import view_ref
from tests.util import assert_outliers_explained, oracle_flip_bounds

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((72, 40), (70, 37), (16, 16))
N_GAUSSIANS = 400
GUARD_F, GUARD_B = 12345.0, 77
# views that are not poses of the map (world-to-camera; the map was made in front of the identity camera at z in 1..4)
VIEW_POSES = {
    "turned 30 degrees about y": view_ref.rigid((0, 1, 0), 30.0, (0.3, 0.0, 0.4)),           # the scene partly outside the image
    "general": view_ref.rigid((1.0, 2.0, 3.0), 12.0, (0.15, -0.1, 0.6)),
    "rolled, stepped back": view_ref.rigid((0.1, -0.2, 1.0), -25.0, (-0.1, 0.05, 1.2)),
}


def _intrinsics(W, H):
    f = 0.8 * W
    return f, f + 1.5, W / 2 - 0.5, H / 2 - 0.25


def _map(W, H, aniso, seed=0, num_frames=3):
    from splatam_amd import slam
    fx, fy, cx, cy = _intrinsics(W, H)
    params, variables = slam.synthetic_params(N_GAUSSIANS, W, H, fx, fy, cx, cy, num_frames=num_frames, seed=seed, device="cuda", anisotropic=aniso)
    k = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
    cam = slam.setup_camera(W, H, k, np.eye(4, dtype=np.float32), device="cuda")
    return params, variables, k, cam


def _engine(W, H, aniso, **kw):
    from splatam_amd.fused import FusedEngine
    params, variables, k, cam = _map(W, H, aniso, **kw)
    with torch.no_grad():
        return FusedEngine(params, cam, variables=variables), params, variables, k


# ---------------------------------------------------------------------------------------------------------------- the camera
def _run_view_camera(lead, W, H, intr, w2c=None, pose=None, offset=None):
    """splat_view_camera with its four outputs inside ONE guarded flat buffer; returns them on the host."""
    import ctypes as C
    from splatam_amd import _capi
    dev = torch.device("cuda")
    flat = torch.full((lead + 16 + 4 + 16 + 4 + 16 + 4 + 3 + 64,), GUARD_F, dtype=torch.float32, device=dev)
    at = {'w2c': lead, 'viewmatrix': lead + 20, 'projmatrix': lead + 40, 'campos': lead + 60}
    a = _capi.SplatViewArgs()
    a.width, a.height = W, H
    a.fx, a.fy, a.cx, a.cy, a.near_z, a.far_z = *intr, 0.01, 100.0
    keep = []
    if w2c is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(w2c, np.float32)).to(dev))
        a.w2c_in = keep[0].data_ptr()
    else:
        rots, trans, t, first = pose
        keep += [rots, trans, torch.from_numpy(np.ascontiguousarray(first, np.float32)).to(dev)]
        a.cam_unnorm_rots, a.cam_trans, a.num_frames, a.time_idx, a.first_w2c = rots.data_ptr(), trans.data_ptr(), rots.shape[-1], t, keep[2].data_ptr()
    if offset is not None:
        off = (C.c_double * 16)(*np.asarray(offset, np.float64).reshape(-1))
        a.offset = off
    for name, o in at.items():
        setattr(a, name, flat.data_ptr() + 4 * o)
    _capi.check(_capi.lib().splat_view_camera(C.byref(a), torch.cuda.current_stream().cuda_stream), "splat_view_camera")
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    out = {name: host[o:o + (3 if name == 'campos' else 16)].copy() for name, o in at.items()}
    mask = np.ones(host.size, bool)
    for name, o in at.items():
        mask[o:o + out[name].size] = False
    assert np.all(host[mask] == np.float32(GUARD_F)), "a store left the camera's buffers"
    return out


def _assert_camera(got, want, bound, what):
    for k in ('w2c', 'viewmatrix', 'projmatrix', 'campos'):
        err = np.abs(got[k].astype(np.float64) - want[k]).max()
        print(f"{what} {k}: max |entry - float64| {err:.3e} (bound {bound:.3e})")
        assert np.isfinite(got[k]).all() and err <= bound, (what, k, err, bound)


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
def test_camera_kernel_against_the_float64_setup_camera(lead):
    W, H = 72, 40
    intr = _intrinsics(W, H)
    offset = np.eye(4)
    offset[2, 3] = 0.5
    poses = dict(VIEW_POSES, identity=np.eye(4, dtype=np.float32), far=view_ref.rigid((1.0, 0.2, 0.5), -112.0, (6.1, -5.3, 5.9)))
    for name, w2c in poses.items():
        for off in (None, offset):
            want = view_ref.camera64(w2c, W, H, *intr, offset=off)
            bound = view_ref.camera_bound(np.linalg.norm(want['w2c'].reshape(4, 4)[:3, 3]))
            _assert_camera(_run_view_camera(lead, W, H, intr, w2c=w2c, offset=off), want, bound, f"{name}{' + offset' if off is not None else ''}")
    # the map-pose form: first_w2c . rel_w2c[t] from un-normalised quaternions, against the float64 product AND against the matrix form
    rng = np.random.default_rng(5)
    rots = torch.from_numpy((rng.normal(size=(1, 4, 4)) * 1.7).astype(np.float32)).cuda()
    trans = torch.from_numpy(rng.uniform(-2, 2, size=(1, 3, 4)).astype(np.float32)).cuda()
    first = VIEW_POSES["general"]
    for t in range(4):
        M = first.astype(np.float64) @ view_ref.rel_w2c64(rots[0, :, t].cpu().numpy(), trans[0, :, t].cpu().numpy())
        want = view_ref.camera64(M, W, H, *intr, offset=offset)
        bound = view_ref.camera_bound(np.linalg.norm(want['w2c'].reshape(4, 4)[:3, 3]))
        got = _run_view_camera(lead, W, H, intr, pose=(rots, trans, t, first), offset=offset)
        _assert_camera(got, want, bound, f"map pose {t}")
        by_matrix = _run_view_camera(lead, W, H, intr, w2c=M.astype(np.float32), offset=offset)
        for k in got:
            assert np.abs(got[k].astype(np.float64) - by_matrix[k]).max() <= bound, (t, k)


# ---------------------------------------------------------------------------------------------------------------- the planes of a view
def _oracle_planes(params, k, W, H, w2c):
    """The CPU oracle's two renders (float32 build) of the map's Gaussians at the camera of ``w2c``, the float64 oracle's flip bounds for
    them, as [6, H, W] arrays in out6's order (r, g, b, depth, silhouette, depth^2)."""
    from oracle import c_ref
    from splatam_amd import slam
    p = {key: v.detach().cpu() for key, v in params.items()}
    p['cam_unnorm_rots'] = torch.tensor([1.0, 0.0, 0.0, 0.0]).view(1, 4, 1)
    p['cam_trans'] = torch.zeros(1, 3, 1)
    w2c_t = torch.from_numpy(np.ascontiguousarray(w2c, np.float32))
    cam = slam.setup_camera(W, H, k, w2c_t, device="cpu")
    with torch.no_grad():
        tg = slam.transform_to_frame(p, 0, gaussians_grad=False, camera_grad=False)
        rv, dv = slam.transformed_params2rendervar(p, tg), slam.transformed_params2depthplussilhouette(p, w2c_t, tg)
        im, _, _ = c_ref.CRasterizer(cam)(**rv)
        ds, _, _ = c_ref.CRasterizer(cam)(**dv)
        b_im, _, _, _, n_im = oracle_flip_bounds(rv, cam)
        b_ds, _, _, _, n_ds = oracle_flip_bounds(dv, cam)
    return (np.concatenate([im.numpy(), ds.numpy()]), np.concatenate([b_im[:3], b_ds[:3]]), np.concatenate([n_im[:3], n_ds[:3]]))


@pytest.mark.parametrize("aniso", [False, True], ids=["isotropic", "anisotropic"])
@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_view_planes_at_poses_the_map_does_not_hold(W, H, aniso):
    eng, params, _, k = _engine(W, H, aniso, seed=W)
    view = eng.view_camera(W, H)
    for name, w2c in VIEW_POSES.items():
        with torch.no_grad():
            image = eng.render_view(view, w2c=torch.from_numpy(w2c).cuda(), intrinsics=k)
        torch.cuda.synchronize()
        assert int(image.truncated) == 0 and not view.check_overflow(grow=False)
        got = image.out6.cpu().numpy()
        ref, bound, noise = _oracle_planes(params, k, W, H, w2c)
        what = f"{W}x{H} {'aniso' if aniso else 'iso'} {name}"
        assert (ref[4] > 0.5).mean() > 0.2, "the view sees too little of the map to show anything"
        assert_outliers_explained(got[:3], ref[:3], bound[:3], 1e-4, noise=noise[:3], what=f"{what} colour")
        assert_outliers_explained(got[3:], ref[3:], bound[3:], 1e-4, rtol=1e-4, noise=noise[3:], what=f"{what} depth/sil/depth^2")
    assert (ref[4] < 0.5).mean() > 0.02 or W == 16                  # (the last, stepped-back view leaves part of the image empty)


# ---------------------------------------------------------------------------------------------------------------- the finish kernel
def _run_finish(out6, mode, lead, bg=(0.0, 0.0, 0.0), vmin=0.0, vmax=6.0, lut=None, w2c=None, intr=None):
    """``fused.view_finish`` with rgb8 inside a guarded byte buffer and points / colors inside ONE guarded float buffer."""
    from splatam_amd import fused
    dev = torch.device("cuda")
    H, W = out6.shape[1:]
    n = 3 * H * W
    bytes_ = torch.full((lead + n + 64,), GUARD_B, dtype=torch.uint8, device=dev)
    floats = torch.full((lead + n + 8 + n + 64,), GUARD_F, dtype=torch.float32, device=dev)
    rgb8, pts, col = bytes_[lead:lead + n], floats[lead:lead + n], floats[lead + n + 8:lead + 2 * n + 8]
    cloud = w2c is not None
    planes = torch.from_numpy(out6).to(dev)
    fused.view_finish(planes, mode, background=bg, depth_range=(vmin, vmax), lut=None if lut is None else torch.from_numpy(lut).to(dev),
                      rgb8=rgb8, points=pts if cloud else None, colors=col if cloud else None, intrinsics=intr,
                      w2c=None if w2c is None else torch.from_numpy(np.ascontiguousarray(w2c, np.float32)).to(dev))
    torch.cuda.synchronize()
    hb, hf = bytes_.cpu().numpy(), floats.cpu().numpy()
    assert np.all(hb[:lead] == GUARD_B) and np.all(hb[lead + n:] == GUARD_B), "a store left rgb8"
    inside = np.zeros(hf.size, bool)
    if cloud:
        inside[lead:lead + n] = inside[lead + n + 8:lead + 2 * n + 8] = True
    assert np.all(hf[~inside] == np.float32(GUARD_F)), "a store left the cloud's views"
    return hb[lead:lead + n].reshape(H, W, 3), hf[lead:lead + n].reshape(-1, 3), hf[lead + n + 8:lead + 2 * n + 8].reshape(-1, 3)


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("W,H", SHAPES + ((1, 1),), ids=lambda v: str(v))
def test_finish_kernel_against_the_float64_restatement(W, H, lead):
    from splatam_amd.view import jet_lut
    intr = _intrinsics(W, H)
    out6 = view_ref.seeded_planes(W, H, seed=100 * W + H, depth_lo=-0.5, depth_hi=7.0)
    w2c = view_ref.rigid((1.0, 0.2, 0.5), -112.0, (6.1, -5.3, 5.9))
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1).copy()
    path = "16-byte path" if (W % 4 == 0 and lead % 16 == 0) else "scalar path"
    # the yardstick of the cloud, once: how far the torch float32 form of rgbd2pcd on these planes is from float64
    want_p, _ = view_ref.cloud64(out6, w2c, *intr)
    torch_err = np.abs(view_ref.cloud_torch32(torch.from_numpy(out6).cuda(), torch.from_numpy(w2c).cuda(), *intr).cpu().numpy().astype(np.float64) - want_p).max()
    for bg in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
        _, want_c = view_ref.cloud64(out6, w2c, *intr, bg=bg)
        for mode, luts in (("color", (None,)), ("depth", (grey, np.ascontiguousarray(jet_lut()))), ("sil", (None,))):
            for lut in luts:
                rgb8, pts, col = _run_finish(out6, mode, lead, bg=bg, lut=lut, w2c=w2c, intr=intr)
                view_ref.check_bytes(rgb8, out6, mode, bg=bg, lut=lut, what=f"{W}x{H} lead {lead} ({path})")
                err = np.abs(pts.astype(np.float64) - want_p).max()
                print(f"{W}x{H} lead {lead} ({path}) cloud: max |point - float64| {err:.3e}, torch float32 rgbd2pcd {torch_err:.3e}")
                assert err <= 2.0 * torch_err, (err, torch_err)
                assert np.abs(col.astype(np.float64) - want_c).max() <= 2.0 ** -23
    # bytes alone (no cloud asked for), the fixed cases
    rgb8, _, _ = _run_finish(np.zeros((6, H, W), np.float32), "color", lead, bg=(1.0, 1.0, 1.0))
    assert (rgb8 == 255).all()                                      # a white background behind an empty silhouette
    bad = out6.copy()
    bad.reshape(6, -1)[:, ::3] = np.nan
    bad.reshape(6, -1)[:, 1::7] = np.inf
    bad.reshape(6, -1)[:, 2::5] = -np.inf
    for mode in ("color", "depth", "sil"):
        rgb8, _, _ = _run_finish(bad, mode, lead, bg=(1.0, 1.0, 1.0), lut=grey)
        want, _ = view_ref.bytes64(bad, mode, bg=(1.0, 1.0, 1.0))
        special = ~np.isfinite(bad[:5]).all(axis=0)
        got = rgb8[..., 0] if mode == "depth" else rgb8
        assert np.array_equal(got[special], want[special]), mode    # NaN and the infinities land where the definitions put them
    rgb8, _, _ = _run_finish(out6, "depth", lead, vmin=2.0, vmax=2.0, lut=grey)
    assert np.array_equal(rgb8[..., 0], np.where(out6[3] > 2.0, 255, 0))


# ---------------------------------------------------------------------------------------------------------------- replay
def test_replay_renders_the_rows_up_to_a_time_step():
    from splatam_amd.fused import FusedEngine, PARAM_ORDER
    W, H = 72, 40
    params, variables, k, cam = _map(W, H, aniso=False, seed=9)
    steps = torch.tensor([0.0] * 150 + [1.0] * 130 + [3.0] * 120, device="cuda")
    variables['timestep'] = steps
    w2c = torch.from_numpy(VIEW_POSES["general"]).cuda()
    with torch.no_grad():
        eng = FusedEngine(params, cam, variables=variables)
        view = eng.view_camera(W, H)
        for t, rows in ((0, 150), (1, 280), (2, 280), (3, 400)):
            got = eng.render_view(view, w2c=w2c, intrinsics=k, max_timestep=t).out6.clone()
            part = {key: (v.detach()[:rows].contiguous() if key in PARAM_ORDER else v.detach()) for key, v in params.items()}
            small = FusedEngine(part, cam)
            want = small.render_view(small.view_camera(W, H), w2c=w2c, intrinsics=k).out6
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), t
            assert float(got[4].max()) > 0.5
        whole = eng.render_view(view, w2c=w2c, intrinsics=k).out6.clone()
        assert torch.equal(whole.view(torch.int32), got.view(torch.int32))
        # a map whose time steps are not in row order is refused before anything is launched
        shuffled = dict(variables, timestep=steps[torch.randperm(400, generator=torch.Generator().manual_seed(1)).cuda()])
        eng2 = FusedEngine(params, cam, variables=shuffled)
        view2 = eng2.view_camera(W, H)
        before = (view2.camera.buf['out6'].clone(), view2.mats.clone(), view2.rgb8.clone())
        with pytest.raises(RuntimeError, match="not non-decreasing"):
            eng2.render_view(view2, w2c=w2c, intrinsics=k, max_timestep=1)
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731  (planes nobody has written may hold NaN)
        assert torch.equal(bits(before[0]), bits(view2.camera.buf['out6'])) and torch.equal(before[1], view2.mats) and torch.equal(before[2], view2.rgb8)
        assert float(eng2.render_view(view2, w2c=w2c, intrinsics=k).out6[4].max()) > 0.5       # (without a replay it renders)


# ---------------------------------------------------------------------------------------------------------------- read-only, in place
def test_a_view_render_leaves_the_loop_as_it_was_and_allocates_once():
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine, PARAM_ORDER
    from tests.test_gpu_fused import _scene
    W, H = 72, 40
    params, variables, frame, cam = _scene(N_GAUSSIANS, W, H, seed=4)
    f = 0.5 * W
    k = [[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]]
    with torch.no_grad():
        eng = FusedEngine(params, cam, gaussian_capacity=1024, variables=variables)
        for _ in range(3):
            eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)      # moments, max_2D_radius and the main camera's planes are not zero
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
        assert float(before["exp_avg means3D"].abs().max()) > 0 and float(before["variables max_2D_radius"].max()) > 0
        stats = (main.tile_stride, main.max_list_hint, eng.num_cameras, set(main._orders))
        view = eng.view_camera(W, H)
        first = eng.render_view(view, w2c=torch.from_numpy(VIEW_POSES["general"]).cuda(), intrinsics=k, points=True)
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_allocated()
        ptrs = (first.rgb8.data_ptr(), first.points.data_ptr(), first.out6.data_ptr())
        zoom = [[1.7 * f, 0, W / 2 + 3.0], [0, 1.6 * f, H / 2 - 2.0], [0, 0, 1]]
        for w2c, kk, mode in ((VIEW_POSES["turned 30 degrees about y"], zoom, "depth"), (VIEW_POSES["rolled, stepped back"], k, "sil")):
            again = eng.render_view(view, w2c=torch.from_numpy(w2c).cuda(), intrinsics=kk, mode=mode, background=(1.0, 1.0, 1.0), points=True)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == allocated
            assert (again.rgb8.data_ptr(), again.points.data_ptr(), again.out6.data_ptr()) == ptrs
        assert eng._camera is main and eng.num_cameras == stats[2]
        assert (main.tile_stride, main.max_list_hint, eng.num_cameras, set(main._orders)) == stats
        after = snapshot()
        for name, t in before.items():
            assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, after[name].view(torch.int32) if t.dtype == torch.float32 else after[name]), name
        assert eng.rendered()[0].data_ptr() == main.buf['out6'].data_ptr()
        # ... and the loop goes on: its next iteration is not flagged
        eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
        torch.cuda.synchronize()
        assert not eng.check_overflow()


# ---------------------------------------------------------------------------------------------------------------- session, evaluation, tool
def _sequence(num_frames=3, W=72, H=40):
    from splatam_amd import pipeline
    f = 0.9 * W
    ds = pipeline.SyntheticRGBDSequence(1500, W, H, f, f, W / 2 - 0.5, H / 2 - 0.5, num_frames=num_frames, seed=2, step_m=0.012, step_deg=0.4).preload()
    cfg = pipeline.replica_config(tracking_iters=4, mapping_iters=6, keyframe_every=2)
    return ds, cfg


def test_session_follow_view_after_every_frame():
    from splatam_amd.session import SlamSession
    ds, cfg = _sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    with SlamSession(cfg, len(ds)) as session:
        for t in range(len(ds)):
            session.add_frame(*ds[t])
            before = {n: session.params[n].detach().clone() for n in session.params}
            array, event, truncated = session.render_view(follow=True, to_host=True, background=(1.0, 1.0, 1.0))
            event.synchronize()
            assert int(truncated[0]) == 0 and not session.view_check_overflow()
            assert array.shape == (40, 72, 3) and array.dtype == np.uint8 and array.min() != array.max()
            view = session._view['view']
            assert np.array_equal(array, view.rgb8.cpu().numpy())
            for n, p in before.items():
                assert torch.equal(p, session.params[n].detach()), n
            # the follow camera is the latest pose seen from half a metre behind
            M = session.first_frame_w2c.double().cpu().numpy() @ view_ref.rel_w2c64(session.params['cam_unnorm_rots'][0, :, t].detach().cpu().numpy(),
                                                                                      session.params['cam_trans'][0, :, t].detach().cpu().numpy())
            M[2, 3] += 0.5
            assert np.abs(view.w2c.cpu().numpy().astype(np.float64) - M).max() <= view_ref.camera_bound(np.linalg.norm(M[:3, 3]))
        session.finish()
        image = session.render_view(time_idx=1, mode="depth")           # after finish(), on the device
        assert tuple(image.rgb8.shape) == (40, 72, 3) and int(image.truncated) == 0


def test_saved_frames_decode_to_the_kernels_bytes(tmp_path):
    from PIL import Image
    from splatam_amd import evaluation, fused, pipeline
    from splatam_amd.view import jet_lut
    ds, cfg = _sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    params, variables, stats = pipeline.rgbd_slam(ds, cfg, engine="fused")
    args = (ds, params, len(ds), cfg['mapping']['sil_thres'], cfg['mapping']['num_iters'], cfg['mapping']['add_new_gaussians'])
    plain = evaluation.evaluate(*args, ms_ssim=False)
    planes = {}
    orig = evaluation._FrameSaver.save

    def save(self, t, out6, im, depth):
        planes[t] = (out6.clone(), im.clone(), depth.clone())
        return orig(self, t, out6, im, depth)
    evaluation._FrameSaver.save = save
    try:
        saved = evaluation.evaluate(*args, ms_ssim=False, save_frames=True, eval_dir=str(tmp_path))
    finally:
        evaluation._FrameSaver.save = orig
    for key in ('psnr', 'depth_rmse', 'depth_l1', 'ms_ssim', 'valid_pixels'):
        assert np.array_equal(plain[key], saved[key], equal_nan=True), key
    assert plain['ate_rmse'] == saved['ate_rmse'] and plain['frames'] == saved['frames'] == [0, 1, 2]
    assert sorted(os.listdir(tmp_path)) == sorted(["rendered_rgb", "rendered_depth", "rgb", "depth", "psnr.txt", "rmse.txt", "l1.txt", "ssim.txt"])
    lut = torch.from_numpy(jet_lut()).cuda()
    for t in saved['frames']:
        out6, im, depth = planes[t]
        gt6 = torch.cat([im, depth, torch.ones_like(depth)])
        for folder, stem, src, mode in (("rendered_rgb", "gs", out6, "color"), ("rendered_depth", "gs", out6, "depth"),
                                        ("rgb", "gt", gt6, "color"), ("depth", "gt", gt6, "depth")):
            want = torch.zeros(40, 72, 3, dtype=torch.uint8, device="cuda")
            fused.view_finish(src.contiguous(), mode, lut=lut, rgb8=want)
            got = np.asarray(Image.open(os.path.join(tmp_path, folder, f"{stem}_{t:04d}.png")).convert("RGB"))
            assert np.array_equal(got, want.cpu().numpy()), (folder, t)
            assert got.min() != got.max()
        assert len(os.listdir(os.path.join(tmp_path, "rgb"))) == 3


@pytest.mark.parametrize("mode,shrink", (("color", False), ("centers", False), ("color", True)), ids=("color", "centers", "color-retry"))
def test_render_trajectory_writes_the_bytes_of_render_view(tmp_path, monkeypatch, mode, shrink):
    """``view.render_trajectory`` on a run's file (400 Gaussians, 3 poses, recorded at 96 x 64, pictured at 48 x 32): every PNG holds the
    bytes of a direct ``render_view`` at that pose with the intrinsics halved, on an engine that takes the same steps (render, digest).
    ``centers`` mode uses no lists: it must not digest (``ViewCamera.check_overflow`` is never called); ``color`` digests once a frame.
    ``color-retry`` forces the loop's retry on the device: after the first digest has learnt the buckets they are shrunk to 16 entries
    a tile (as tests/test_gpu_novel_view.py forces its repeated rows), so the second frame's first render is flagged and goes again."""
    from PIL import Image
    from splatam_amd import fused, slam, view as V
    W, H = 48, 32
    params, variables, k, _ = _map(W, H, aniso=False, seed=4)
    with torch.no_grad():                                    # three distinct poses: a step, then a step with a small rotation
        params['cam_trans'][0, :, 1] = torch.tensor([0.05, -0.02, 0.1])
        params['cam_trans'][0, :, 2] = torch.tensor([-0.04, 0.03, 0.2])
        params['cam_unnorm_rots'][0, :, 2] = torch.tensor([1.0, 0.02, -0.05, 0.03])
    k0 = np.array(k, dtype=np.float64)
    k0[:2] *= 2.0                                            # (the run's frames were twice the pictures' size: halving is exact)
    path = str(tmp_path / "params.npz")
    np.savez(path, **{n: v.detach().cpu().numpy() for n, v in params.items()}, timestep=variables['timestep'].cpu().numpy(), intrinsics=k0,
             w2c=np.eye(4, dtype=np.float32), org_width=2 * W, org_height=2 * H)
    orig = fused.ViewCamera.check_overflow

    def digest(view, log):
        log.append(orig(view))
        if shrink and len(log) == 1:
            assert view.camera.tile_stride > 16
            view.camera.tile_stride = 16
        return log[-1]
    digests = []
    with monkeypatch.context() as patched:
        patched.setattr(fused.ViewCamera, "check_overflow", lambda self: digest(self, digests))
        written = V.render_trajectory(path, str(tmp_path / "out"), mode=mode, size=(W, H), verbose=False)
    assert [os.path.basename(p) for p in written] == [f"view_{t:04d}.png" for t in range(3)]
    assert digests == ([] if mode == "centers" else [False, True, False, False] if shrink else [False] * 3), digests
    loaded, lvars, lk, first_w2c, size0 = V.load_map(path, torch.device("cuda"))
    assert size0 == (2 * W, 2 * H)
    steps = []
    with torch.no_grad():
        eng = fused.FusedEngine(loaded, slam.setup_camera(2 * W, 2 * H, lk, first_w2c.cpu().numpy(), device="cuda"), variables=lvars)
        view = eng.view_camera(W, H)
        for t, name in enumerate(written):
            for _ in range(3):
                want = eng.render_view(view, time_idx=t, first_w2c=first_w2c.contiguous(), intrinsics=_intrinsics(W, H), mode=mode).rgb8
                if mode == "centers" or not digest(view, steps):
                    break
            want = want.cpu().numpy()
            got = np.asarray(Image.open(name))
            assert got.shape == (H, W, 3) and got.dtype == np.uint8 and np.array_equal(got, want), (mode, t)
            assert want.min() != want.max()
    assert steps == digests


def test_the_tool_writes_a_picture_per_pose(tmp_path):
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
    done = subprocess.run([sys.executable, "-m", "splatam_amd.view", path, "--out", str(pictures), "--replay", "--white", "--size", "36x20"],
                          cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    assert sorted(os.listdir(pictures)) == [f"view_{t:04d}.png" for t in range(3)], done.stdout
    for name in os.listdir(pictures):
        picture = np.asarray(Image.open(pictures / name))
        assert picture.shape == (20, 36, 3) and picture.min() != picture.max()
