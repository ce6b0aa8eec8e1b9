"""``session.SlamSession`` on the CPU (``engine="dropin"`` with the C oracle behind the ``Renderer`` name): the recording of the
REFERENCE'S OWN ``rgbd_slam`` (tests/golden/loop_reference.npz) driven frame by frame through ``add_frame`` and compared the way
tests/test_loop_golden.py compares ``pipeline.rgbd_slam`` -- its assertions are called on the session's run, with their bounds;
the raw path (``add_raw_frame``: bytes and float32 depth through ``datasets.ingest_planes_cpu``) against the item path on the same
frames; an early ``finish()``; a frame too many; the keyframe rule for a pose with NaN; the constructor's errors."""
import copy

import numpy as np
import pytest
import torch

import loop_trace as LT
import test_loop_golden as TLG
from test_loop_golden import GOLD, seed_everything


class oracle_renderer:
    def __enter__(self):
        from oracle import c_ref
        from splatam_amd import slam
        self.saved, slam.Renderer = slam.Renderer, c_ref.CRasterizer

    def __exit__(self, *exc):
        from splatam_amd import slam
        slam.Renderer = self.saved


def frames_as_bytes(ds, t):
    """Frame ``t`` as a sensor would deliver it -- colour bytes ``round(colour)``, float32 depth [H, W] -- and as the dataset item
    that holds the same bytes as floats."""
    color, depth, k, pose = ds[t]
    rgb = torch.round(color).clamp(0, 255).to(torch.uint8)
    return (rgb.numpy().copy(), depth[..., 0].numpy().copy()), (rgb.to(torch.float32), depth, k, pose)


@pytest.fixture(scope="module")
def base_through_the_session():
    from splatam_amd import pipeline, session, slam
    cfg = LT.load_config(GOLD, "base")
    ds = LT.RecordedRGBDSequence(GOLD, "base")
    results = []
    with oracle_renderer():
        rec = LT.LoopRecorder().wrap(slam).wrap(pipeline)
        try:
            seed_everything(cfg['seed'])
            with session.SlamSession(cfg, len(ds), engine="dropin") as s:
                for t in range(len(ds)):
                    results.append(s.add_frame(*ds[t]))
                    results[-1]['w2c'] = results[-1]['w2c'].clone()
                params, variables, stats = s.finish()
        finally:
            rec.restore()
    return ("base", cfg, rec, params, variables, stats), results


def test_the_session_makes_the_reference_loops_calls(base_through_the_session):
    run, _ = base_through_the_session
    TLG.test_call_sequence_equals_the_reference_loop(run)
    TLG.test_losses_follow_the_reference_loop(run)
    TLG.test_final_state_equals_the_reference_loop(run)
    TLG.test_decisions_view(run)


def test_every_frames_result(base_through_the_session):
    from splatam_amd import pipeline
    (case, cfg, rec, params, variables, stats), results = base_through_the_session
    assert stats['frames_seen'] == len(results) == GOLD["base/frames/color"].shape[0]
    for t, r in enumerate(results):
        assert set(r) == {'time_idx', 'w2c', 'tracking_iters', 'num_gaussians', 'keyframe', 'phase_ms'}
        assert r['time_idx'] == t and r['keyframe'] == (t in stats['keyframe_time_indices'])
        assert r['tracking_iters'] == stats['decisions'][t]['tracking_iters'] and r['num_gaussians'] == stats['num_gaussians'][t]
        assert r['phase_ms'] is stats['phase_ms'][t] and 'tracking' in r['phase_ms'] and 'prepare_frames' in r['phase_ms']
        assert torch.equal(r['w2c'], pipeline._est_w2c(params, t))
    assert params['cam_trans'].shape[-1] == params['cam_unnorm_rots'].shape[-1] == len(results)


def test_rgbd_slam_is_the_driver_over_the_session(monkeypatch):
    """One definition of the loop body: ``rgbd_slam`` hands every frame to ``SlamSession.add_frame``."""
    from splatam_amd import pipeline, session
    seen = []
    real = session.SlamSession.add_frame

    def counted(self, *a, **k):
        seen.append(self.frames_seen)
        return real(self, *a, **k)
    monkeypatch.setattr(session.SlamSession, "add_frame", counted)
    cfg = LT.load_config(GOLD, "gtposes")
    with oracle_renderer():
        seed_everything(cfg['seed'])
        _, _, stats = pipeline.rgbd_slam(LT.RecordedRGBDSequence(GOLD, "gtposes"), cfg, engine="dropin", num_frames=2)
    assert seen == [0, 1] and stats['keyframe_time_indices'] == [0, 1] and len(stats['frame_s']) == 2


def run_four_frames(raw, scribble=False):
    from splatam_amd import session
    cfg = LT.load_config(GOLD, "base")
    ds = LT.RecordedRGBDSequence(GOLD, "base")
    planes = []
    with oracle_renderer():
        seed_everything(cfg['seed'])
        with session.SlamSession(cfg, 4, engine="dropin", device="cpu") as s:
            for t in range(4):
                (rgb, depth), item = frames_as_bytes(ds, t)
                if raw:
                    r = s.add_raw_frame(rgb, depth, item[2].numpy(), pose=None)
                    if scribble:
                        rgb[:], depth[:] = 255 - rgb, np.float32(-7.0)
                else:
                    r = s.add_frame(item[0], item[1], item[2], None)
                assert r['time_idx'] == t
                planes.append(tuple(p.clone() for p in s.last_frame['full']))
            return s.finish() + (planes,)


def test_raw_frames_on_the_cpu_run_the_mirror_and_equal_the_item_path():
    pa, _, sa, planes_a = run_four_frames(raw=False)
    pb, _, sb, planes_b = run_four_frames(raw=True, scribble=True)
    for (ia, da), (ib, db) in zip(planes_a, planes_b):
        assert tuple(ib.shape) == (3, 64, 96) and tuple(db.shape) == (1, 64, 96)
        assert torch.equal(ia, ib) and torch.equal(da, db)
    assert sa['decisions'] == sb['decisions'] and sa['keyframe_time_indices'] == sb['keyframe_time_indices'] == [0, 1, 2, 3]
    for k in ('cam_unnorm_rots', 'cam_trans'):
        assert float((pa[k] - pb[k]).detach().abs().max()) < 2e-4
    # pose=None: the first frame is the world frame
    assert torch.equal(pb['cam_trans'][..., 0], torch.zeros(1, 3)) and sb['frames_seen'] == 4


def tiny_session(num_frames, **kw):
    from splatam_amd import session
    cfg = LT.load_config(GOLD, "gtposes")                # (ground-truth poses: no tracking iterations, the cheapest frames)
    return cfg, LT.RecordedRGBDSequence(GOLD, "gtposes"), session.SlamSession(cfg, num_frames, engine="dropin", **kw)


def test_an_early_finish_cuts_the_pose_arrays_and_a_frame_too_many_raises():
    with oracle_renderer():
        cfg, ds, s = tiny_session(5)
        seed_everything(cfg['seed'])
        for t in range(2):
            s.add_frame(*ds[t])
        params, _, stats = s.finish()
        assert stats['frames_seen'] == 2 and params['cam_trans'].shape == (1, 3, 2) and params['cam_unnorm_rots'].shape == (1, 4, 2)
        assert stats['keyframe_time_indices'] == [t for t in range(2) if t == 0 or (t + 1) % cfg['keyframe_every'] == 0 or t == 3]
        with pytest.raises(RuntimeError):
            s.add_frame(*ds[2])                         # finished
        cfg, ds, s = tiny_session(2)
        seed_everything(cfg['seed'])
        for t in range(2):
            s.add_frame(*ds[t])
        with pytest.raises(RuntimeError, match="num_frames = 2"):
            s.add_frame(*ds[2])
        assert s.finish()[0]['cam_trans'].shape == (1, 3, 2)


def test_a_pose_with_nan_on_a_keyframe_frame_stores_no_keyframe():
    with oracle_renderer():
        cfg, ds, s = tiny_session(3)
        cfg['tracking']['use_gt_poses'] = False
        cfg['tracking']['num_iters'] = 1
        seed_everything(cfg['seed'])
        assert s.add_frame(*ds[0])['keyframe']
        color, depth, k, pose = ds[1]
        bad = pose.clone()
        bad[0, 3] = float("nan")
        assert not s.add_frame(color, depth, k, bad)['keyframe']         # (num_frames - 2: a keyframe frame by the rule)
        _, _, stats = s.finish()
        assert stats['keyframe_time_indices'] == [0] and [d['keyframe'] for d in stats['decisions']] == [True, False]
        cfg, ds, s = tiny_session(3)
        cfg['tracking']['use_gt_poses'] = False
        cfg['tracking']['num_iters'] = 1
        seed_everything(cfg['seed'])
        color, depth, k, _ = ds[0]
        s.add_frame(color, depth, k)
        color, depth, k, _ = ds[1]
        assert s.add_frame(color, depth, k, None)['keyframe']            # every frame with pose=None is stored


def test_the_constructors_errors():
    from splatam_amd import session
    cfg = LT.load_config(GOLD, "base")
    with pytest.raises(ValueError):
        session.SlamSession(cfg, 4, engine="eager")
    for n in (0, -1, 2.5):
        with pytest.raises(ValueError):
            session.SlamSession(cfg, n, engine="dropin")
    bad = copy.deepcopy(cfg)
    bad['mapping']['use_gaussian_splatting_densification'] = True
    with pytest.raises(NotImplementedError):
        session.SlamSession(bad, 4, engine="dropin")
    bad = copy.deepcopy(cfg)
    bad['gaussian_distribution'] = "spherical"
    with pytest.raises(ValueError):
        session.SlamSession(bad, 4, engine="dropin")
    bad = copy.deepcopy(cfg)
    bad['mean_sq_dist_method'] = "knn"
    with pytest.raises(ValueError):
        session.SlamSession(bad, 4, engine="fused")
    # use_gt_poses needs poses: a frame without one is refused before anything is done with it
    gt = LT.load_config(GOLD, "gtposes")
    ds = LT.RecordedRGBDSequence(GOLD, "gtposes")
    s = session.SlamSession(gt, 4, engine="dropin")
    with pytest.raises(ValueError, match="use_gt_poses"):
        s.add_frame(*ds[0][:3])
    assert s.frames_seen == 0 and s.params is None
    with pytest.raises(RuntimeError):
        s.finish()                                      # no frame, no map
    s = session.SlamSession(cfg, 4, engine="dropin", device="cpu")
    with pytest.raises(ValueError):
        s.add_raw_frame(np.zeros((8, 8, 3), np.float32), np.zeros((8, 8), np.float32), np.eye(3))      # a float colour
    with pytest.raises(ValueError):
        s.add_raw_frame(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint16), np.eye(3))         # uint16 depth without its divisor
    with pytest.raises(ValueError):
        s.add_raw_frame(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.float32), np.eye(3), depth_scale=1000.0)


def test_rgbd_slam_stores_no_keyframe_for_a_pose_with_nan():
    """The batch driver through the same rule, with the poses on the host as the loaders keep them (``dataset.poses``) and without."""
    from splatam_amd import pipeline

    class WithABadPose(LT.RecordedRGBDSequence):
        def __init__(self, host_copy):
            super().__init__(GOLD, "gtposes")
            self.pose = self.pose.clone()
            self.pose[1, 2, 3] = float("inf")
            if host_copy:
                self.poses = self.pose

    for host_copy in (True, False):
        cfg = LT.load_config(GOLD, "gtposes")
        cfg['tracking']['use_gt_poses'] = False
        cfg['tracking']['num_iters'] = 1
        with oracle_renderer():
            seed_everything(cfg['seed'])
            _, _, stats = pipeline.rgbd_slam(WithABadPose(host_copy), cfg, engine="dropin", num_frames=3)
        assert stats['keyframe_time_indices'] == [0] + ([2] if (2 + 1) % cfg['keyframe_every'] == 0 else [])
        assert [d['keyframe'] for d in stats['decisions']][:2] == [True, False]
