"""One managed ``FusedEngine``, one ~8 000-Gaussian synthetic map, three cameras -- 96 x 64, 72 x 48 (a partial tile column), 48 x 32 --
as the frame loop uses them when tracking and densification have resolutions of their own: what belongs to the map exists once, what
belongs to a camera (planes, tile arrays, lists, list statistics) once per camera.  The parity target everywhere is a fresh
SINGLE-camera engine built for that camera on a copy of the map."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, N, SEED = 96, 64, 8000, 5
SIZES = ((64, 96), (48, 72), (32, 48))                 # (height, width)
PARAM_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
# bytes a managed single-camera engine on this map holds after construction, one probe render, one mapping iteration and two
# check_overflow() calls (`single_camera_footprint` below, in a fresh process) on the parent commit a3b06ec
PARENT_COMMIT, PARENT_FOOTPRINT_BYTES = "a3b06ec", 15440896


def make_scene():
    """(params, variables, w2c, {size: cam}, {size: frame of time index 1})"""
    from splatam_amd import slam
    f, cx, cy = 0.5 * W, W / 2 - 0.5, H / 2 - 0.5
    params, variables = slam.synthetic_params(N, W, H, f, f, cx, cy, num_frames=4, seed=SEED, device="cuda")
    k = torch.tensor([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    w2c = torch.eye(4, device="cuda")
    cams, frames = {}, {}
    for h, w in SIZES:
        kk = k.clone()                                   # (scale_intrinsics, spelt out: this helper also measures the parent commit)
        kk[0] *= w / W
        kk[1] *= h / H
        cams[(h, w)] = slam.setup_camera(w, h, kk.numpy(), np.eye(4, dtype=np.float32), device="cuda")
        im, depth = slam.synthetic_frame(params, cams[(h, w)], w2c, 1, rot_deg=0.4, trans_m=0.01)
        frames[(h, w)] = {'cam': cams[(h, w)], 'im': im, 'depth': depth, 'id': 1, 'w2c': w2c, 'intrinsics': kk.cuda()}
    with torch.no_grad():                                # a pose that is not the identity
        params['cam_unnorm_rots'][0, :, 1] = torch.tensor([0.999, 0.004, -0.006, 0.003], device="cuda")
        params['cam_trans'][0, :, 1] = torch.tensor([0.004, -0.006, 0.005], device="cuda")
    return params, variables, w2c, cams, frames


def copy_map(params, variables):
    return ({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()},
            {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in variables.items()})


def managed(params, variables, cam, cap=3 * N, **kw):
    from splatam_amd.fused import FusedEngine
    p, v = copy_map(params, variables)
    return FusedEngine(p, cam, gaussian_capacity=cap, variables=v, **kw)


def planes(eng, frame, t=1):
    return [x.clone() for x in eng.render(frame, t)]


def assert_renders_like_single_camera_engines(eng, frames, what, build=None):
    """``build(cam)``: the fresh single-camera engine (default: a managed one on a copy of ``eng``'s map)."""
    for size, frame in frames.items():
        single = build(frame['cam']) if build else managed(eng.params, eng.variables, frame['cam'])
        a, b = planes(single, frame), planes(single, frame)
        got = planes(eng, frame)
        assert (eng.H, eng.W) == size and tuple(got[0].shape) == (3,) + size
        exact = all(torch.equal(x, y) for x, y in zip(a, b))
        for x, y in zip(got, a):
            if exact:
                assert torch.equal(x, y), (what, size)
            else:
                assert float((x - y).abs().max()) <= 1e-4, (what, size)
        print(f"{what}: {size}: render equals the single-camera engine's ({'bit-equal' if exact else 'within 1e-4'})")


def test_render_at_every_camera_equals_a_single_camera_engine():
    params, variables, w2c, cams, frames = make_scene()
    eng = managed(params, variables, cams[SIZES[0]])
    for size in SIZES[1:]:
        eng.add_camera(cams[size])
    assert eng.num_cameras == 3
    assert_renders_like_single_camera_engines(eng, frames, "three cameras")
    assert_renders_like_single_camera_engines(eng, dict(reversed(list(frames.items()))), "three cameras, again, other order")
    assert eng.num_cameras == 3                        # equal settings select, they do not register again


def one_pair(eng, frame):
    """One tracking and one mapping iteration at ``frame``'s camera from fresh optimizer states: what they left."""
    from splatam_amd import _capi, slam
    eng.begin_tracking(1)
    eng.tracking_iteration(frame, slam.REPLICA_TRACKING)
    rep = eng.buf['d_cam'].clone()
    out = {'track_loss': rep[_capi.SPLAT_REPORT_LOSS].clone(), 'pose_grad': rep[:7].clone(), 'pose_state': eng.buf['pose_state'].clone(),
           'cam_unnorm_rots': eng.params['cam_unnorm_rots'].detach().clone(), 'cam_trans': eng.params['cam_trans'].detach().clone()}
    assert float(rep[_capi.SPLAT_REPORT_FLAG]) == 0.0
    eng.reset_map_optimizer()
    eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
    rep = eng.buf['d_cam'].clone()
    assert float(rep[_capi.SPLAT_REPORT_FLAG]) == 0.0
    out['map_loss'] = rep[_capi.SPLAT_REPORT_LOSS].clone()
    for k in PARAM_KEYS:
        out[k] = eng.params[k].detach().clone()
    return out


def test_iterations_at_every_camera_equal_a_single_camera_engines():
    """Interleaved: tracking + mapping at 96 x 64, then at 72 x 48, then at 48 x 32, on ONE evolving map.  Before each pair the map
    is copied and a single-camera engine runs the same pair on the copy, five times: the largest difference between those runs (the
    float atomics of the backward composite) times four is the bound for the multi-camera engine against the first of them."""
    params, variables, w2c, cams, frames = make_scene()
    eng = managed(params, variables, cams[SIZES[0]])
    eng.auto_cameras = True                              # the other two register on first use, from curr_data['cam']
    for size in SIZES:
        frame = frames[size]
        runs = [one_pair(managed(eng.params, eng.variables, frame['cam']), frame) for _ in range(5)]
        got = one_pair(eng, frame)
        assert (eng.H, eng.W) == size
        for k in runs[0]:
            spread = max(float((r[k] - runs[0][k]).abs().max()) for r in runs[1:])
            diff = float((got[k] - runs[0][k]).abs().max())
            print(f"{size}: {k}: single-camera spread over 5 runs {spread:.3e}, multi-camera engine vs run 0 {diff:.3e} (bound {4 * spread:.3e})")
            assert diff <= 4 * spread, (size, k, diff, spread)
    assert eng.num_cameras == 3


def test_growth_and_list_statistics_per_camera():
    from splatam_amd import slam
    params, variables, w2c, cams, frames = make_scene()
    eng = managed(params, variables, cams[SIZES[0]], cap=N + 200)
    for size in SIZES[1:]:
        eng.add_camera(cams[size])
    for size in SIZES:                                   # first use: every camera learns its own statistics
        assert not eng.lists_known(frames[size])
        eng.render(frames[size], 1)
        assert not eng.check_overflow()
        assert eng.lists_known(frames[size])
    learnt = {}
    for size in SIZES:
        eng.select_camera(cams[size])
        learnt[size] = (eng.tile_stride, eng.max_list_hint)
    assert len(set(learnt.values())) > 1                 # (statistics are a camera's own: they differ between the sizes)
    # frame 2 looks past the map: every pixel of the 48 x 32 frame has depth and none is explained -> 1 536 new rows, more than the
    # capacity leaves room for (the rows grow) and more than 10 % of the map (every camera's statistics are dropped)
    with torch.no_grad():
        eng.params['cam_trans'][0, :, 2] = torch.tensor([40.0, 0.0, 0.0], device="cuda")
    small = dict(frames[SIZES[2]], id=2, depth=torch.full_like(frames[SIZES[2]]['depth'], 2.0))
    cap0 = eng.Pcap
    added = eng.add_new_gaussians(small, 0.5, 2, "projective", "isotropic")
    assert added == 32 * 48 and eng.P == N + added and eng.Pcap > cap0 and eng.params['means3D'].shape[0] == eng.P
    assert (eng.H, eng.W) == SIZES[2]
    for size in SIZES:
        assert not eng.lists_known(frames[size]), size
    for i, size in enumerate(SIZES):
        eng.render(frames[size], 1)
        assert not eng.check_overflow()
        assert eng.lists_known(frames[size])
        for other in SIZES[i + 1:]:
            assert not eng.lists_known(frames[other]), (size, other)     # nothing carries over from one camera to another
    assert_renders_like_single_camera_engines(eng, frames, "after the rows grew")


def loop_round(eng, frames, t):
    from splatam_amd import slam
    track, dens, full = frames[SIZES[1]], frames[SIZES[2]], frames[SIZES[0]]
    eng.begin_tracking(t)
    for _ in range(3):
        eng.tracking_iteration(dict(track, id=t), slam.REPLICA_TRACKING)
    assert not eng.check_overflow()
    eng.end_tracking()
    eng.add_new_gaussians(dict(dens, id=t), 0.5, t, "projective", "isotropic")
    if not eng.lists_known(full):
        eng.relearn_lists(full, t)
    eng.reset_map_optimizer()
    for _ in range(3):
        eng.mapping_iteration(dict(full, id=t), t, slam.REPLICA_MAPPING)
    assert not eng.check_overflow()


def test_switching_cameras_allocates_nothing_in_the_steady_state():
    params, variables, w2c, cams, frames = make_scene()
    eng = managed(params, variables, cams[SIZES[0]])
    for size in SIZES[1:]:
        eng.add_camera(cams[size])
    loop_round(eng, frames, 1)
    gc.collect()                                         # (tensors other tests left in reference cycles are not this engine's)
    torch.cuda.synchronize()
    before, rows = torch.cuda.memory_allocated(), eng.P
    loop_round(eng, frames, 1)
    gc.collect()
    torch.cuda.synchronize()
    print(f"allocated after the first round {before} B, after the second {torch.cuda.memory_allocated()} B; rows {rows} -> {eng.P}")
    assert torch.cuda.memory_allocated() == before


def test_overflow_protocol_is_per_camera():
    """The capacity protocol of tests/test_gpu_fused.py::test_list_overflow_is_flagged_not_fatal at ONE camera of three: lists far too
    small for the 96 x 64 camera alone.  The iteration there is flagged and moves nothing, the other cameras keep their statistics
    and their lists, and after check_overflow() the repeat succeeds.  (A flag, not a fault: the kernels never write past a list.)"""
    from splatam_amd import _capi, slam
    params, variables, w2c, cams, frames = make_scene()
    eng = managed(params, variables, cams[SIZES[0]], capacity=100)          # far too small
    others = {}
    for size in SIZES[1:]:
        eng.add_camera(cams[size])
        eng.render(frames[size], 1)
        assert not eng.check_overflow()
        others[size] = (eng.tile_stride, eng.max_list_hint, eng.capacity, eng.buf['keys'].data_ptr())
    before = {k: eng.params[k].detach().clone() for k in PARAM_KEYS}
    eng.reset_map_optimizer()
    eng.mapping_iteration(frames[SIZES[0]], 1, slam.REPLICA_MAPPING)
    torch.cuda.synchronize()
    assert (eng.H, eng.W) == SIZES[0] and eng.capacity == 100
    assert all(torch.equal(before[k], eng.params[k].detach()) for k in PARAM_KEYS)          # no Adam step on truncated lists
    assert eng.settle("map") == 1 and eng.skipped_iterations == 1 and eng.capacity > 100 and eng.map_step == 0
    for size in SIZES[1:]:
        eng.select_camera(cams[size])
        assert (eng.tile_stride, eng.max_list_hint, eng.capacity, eng.buf['keys'].data_ptr()) == others[size], size
        assert float(eng.buf['d_cam'][_capi.SPLAT_REPORT_FLAG]) == 0.0
    eng.mapping_iteration(frames[SIZES[0]], 1, slam.REPLICA_MAPPING)
    torch.cuda.synchronize()
    assert not eng.check_overflow()
    assert not torch.equal(before['means3D'], eng.params['means3D'].detach())              # the repeat took its step


def learn_lists(eng, frames):
    """First use of every camera of ``frames``: a render on exact lists, then check_overflow() learns the camera's statistics."""
    for frame in frames.values():
        eng.render(frame, 1)
        assert not eng.check_overflow()
        assert eng.lists_known(frame)


def list_statistics(eng, cams):
    out = {}
    for size, cam in cams.items():
        eng.select_camera(cam)
        out[size] = (eng.tile_stride, eng.max_list_hint)
    return out


def test_a_refused_camera_changes_nothing():
    """A camera the fused path cannot render (non-zero background) raises from add_camera; the engine, its two cameras, the current
    camera and the bytes allocated are what they were."""
    params, variables, w2c, cams, frames = make_scene()
    eng = managed(params, variables, cams[SIZES[0]])
    eng.add_camera(cams[SIZES[1]])
    two = {size: frames[size] for size in SIZES[:2]}
    learn_lists(eng, two)
    refused = cams[SIZES[2]]._replace(bg=torch.ones(3, device="cuda"))

    def current():
        return (eng.H, eng.W, eng.tile_stride, eng.max_list_hint, eng.capacity, eng.buf['keys'].data_ptr(), eng.buf['out6'].data_ptr())
    gc.collect()
    torch.cuda.synchronize()
    before, allocated = current(), torch.cuda.memory_allocated()
    assert before[:2] == SIZES[1] and before[2] > 0 and before[3] > 0
    with pytest.raises(RuntimeError, match="zero background"):
        eng.add_camera(refused)
    assert eng.num_cameras == 2
    assert current() == before
    gc.collect()
    torch.cuda.synchronize()
    print(f"allocated before the refused camera {allocated} B, after {torch.cuda.memory_allocated()} B")
    assert torch.cuda.memory_allocated() == allocated
    assert_renders_like_single_camera_engines(eng, two, "after a refused camera")


def test_a_small_edit_keeps_every_cameras_list_statistics():
    """Five rows removed of 8 000 (the rule keeps statistics within 10 % of the rows they were learnt on): all three cameras keep
    theirs, and a fourth that has never rendered has none to keep.  (The large edit that drops them all:
    test_growth_and_list_statistics_per_camera.)"""
    from splatam_amd import slam
    params, variables, w2c, cams, frames = make_scene()
    eng = managed(params, variables, cams[SIZES[0]])
    for size in SIZES[1:]:
        eng.add_camera(cams[size])
    learn_lists(eng, frames)
    learnt = list_statistics(eng, cams)
    assert all(stride > 0 and longest > 0 for stride, longest in learnt.values()), learnt
    k = frames[SIZES[0]]['intrinsics'].cpu().clone()
    k[0] *= 40 / W
    k[1] *= 24 / H
    fourth = slam.setup_camera(40, 24, k.numpy(), np.eye(4, dtype=np.float32), device="cuda")
    assert eng.add_camera(fourth) == 3 and (eng.H, eng.W) == (24, 40)
    to_remove = torch.zeros(eng.P, dtype=torch.bool, device="cuda")
    to_remove[[3, 1000, 2500, 4000, N - 1]] = True
    assert eng.remove_points(to_remove) == 5 and eng.P == N - 5
    assert list_statistics(eng, cams) == learnt
    for size in SIZES:
        assert eng.lists_known(frames[size]), size
    eng.select_camera(fourth)
    assert (eng.tile_stride, eng.max_list_hint) == (0, 0) and not eng.lists_known()


def test_rebind_applies_its_rule_to_every_camera():
    """An engine on caller-owned tensors with two cameras: ``rebind`` to a map of 5 % more rows keeps both cameras' statistics (and fits
    the row headroom), to one of 50 % more rows drops both; each camera then learns again and renders what a fresh engine renders."""
    from splatam_amd.fused import FusedEngine
    params, variables, w2c, cams, frames = make_scene()
    two = {size: frames[size] for size in SIZES[:2]}
    two_cams = {size: cams[size] for size in SIZES[:2]}
    eng = FusedEngine(copy_map(params, variables)[0], cams[SIZES[0]], row_headroom=0.125)
    eng.add_camera(cams[SIZES[1]])
    learn_lists(eng, two)
    learnt = list_statistics(eng, two_cams)
    assert all(stride > 0 and longest > 0 for stride, longest in learnt.values()), learnt

    def with_more_rows(extra):
        return {k: (torch.cat([v.detach(), v.detach()[:extra]]) if k in PARAM_KEYS else v.detach().clone()).contiguous()
                for k, v in params.items()}
    eng.rebind(with_more_rows(N // 20))
    assert eng.P == N + N // 20 and eng.Pcap == int(N * 1.125)
    assert list_statistics(eng, two_cams) == learnt
    eng.rebind(with_more_rows(N // 2))
    assert eng.P == N + N // 2 and eng.Pcap >= eng.P
    assert list_statistics(eng, two_cams) == {size: (0, 0) for size in two}
    learn_lists(eng, two)

    def fresh(cam):
        return FusedEngine({k: v.detach().clone() for k, v in eng.params.items()}, cam)
    assert_renders_like_single_camera_engines(eng, two, "after rebind", build=fresh)


def single_camera_footprint():
    """Bytes a managed single-camera engine holds on this map after a probe render and one mapping iteration (uses nothing newer
    than the parent commit's interface, so that the same function measures the parent)."""
    from splatam_amd import slam
    params, variables, w2c, cams, frames = make_scene()
    frame = frames[SIZES[0]]
    p, v = copy_map(params, variables)
    del params, variables
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    from splatam_amd.fused import FusedEngine
    eng = FusedEngine(p, frame['cam'], gaussian_capacity=3 * N, variables=v)
    eng.render(frame, 1)
    eng.check_overflow()
    eng.reset_map_optimizer()
    eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
    eng.check_overflow()
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated() - base


def test_single_camera_footprint_is_the_parent_commits():
    """Measured in a process of its own, as the parent's figure was: ``torch.cuda.memory_allocated()`` counts whole cached blocks where
    the allocator hands one out unsplit, so inside a long test session the same tensors can weigh differently (seen: + 407 040 B in the
    middle of the whole suite)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import test_gpu_multires_engine as t; "
            "print('FOOTPRINT', t.single_camera_footprint())")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = int([line for line in out.stdout.splitlines() if line.startswith("FOOTPRINT")][-1].split()[1])
    print(f"single-camera footprint {got} B (parent {PARENT_COMMIT}: {PARENT_FOOTPRINT_BYTES} B)")
    assert got == PARENT_FOOTPRINT_BYTES
