"""``session.SlamSession`` on the fused engine.

  * The recording of the REFERENCE'S OWN ``rgbd_slam`` (tests/golden/loop_reference.npz, cases "base" and "gtposes") driven frame by
    frame through ``add_frame`` from ``loop_trace.RecordedRGBDSequence`` and checked with ``check_decisions`` / ``check_trajectory``
    of tests/test_gpu_loop_golden.py: that test's ``ROW_TOL`` and 2e-4, the reference's recorded run as the yardstick.
  * The raw path against the item path on the same frames at the loop's own size (colour bytes ``round(colour)``, float32 depth; the
    items hold the same bytes as floats): the planes handed to the loop bit-equal on every frame, decisions equal under
    ``close_rows``, poses within 2e-4 (two runs of one loop whose backward composites add floats atomically: the tolerance the
    golden test gives a run against the recording); the caller's arrays are overwritten right after every call.  Run at the
    seed of ``SEED`` below, where no frame's best tracking candidate is a tie (see there).
  * A densification size of its own: those planes are ``fused.ingest_planes`` of the RAW frame at that size.
  * An early ``finish()``, a frame too many, a pose with NaN on a keyframe frame."""
import numpy as np
import pytest
import torch

import loop_trace as LT
from test_gpu_loop_golden import check_decisions, check_trajectory, close_rows
from test_loop_golden import GOLD, seed_everything

pytestmark = pytest.mark.gpu

# The seed of the raw-against-item comparison (it draws the mapping views and the keyframe samples; the frames are the "base" frames
# rounded to bytes either way).  Tracking ends on the BEST CANDIDATE, the pose of the iteration with the lowest loss
# (scripts/splatam.py:704-711, 741-744).  At the configuration's own seed 0 that choice is a tie on frame 3 of these frames: iterations 6 and 7
# have losses 271.5203 and 271.5205, 1e-7 to 9e-7 apart relatively, while the float atomics of the backward composites move a loss of
# that frame by 2.3e-4 from run to run -- so the pick flips between runs (6, 6, 7, 6, 7, 7, 6, 7, 7, 6 in ten runs) and with it the pose
# by 9.1e-4, one Adam step.  ``pipeline.rgbd_slam`` of the parent commit does the same on the same frames (7, 6, 6, 7, 7, 7, 7, 7, 7, 7;
# 9.1e-4): it is the loop's, not the session's, and two runs of ONE entry miss 2e-4 there as often as raw against item.  Measured on
# an MI355X, ten runs per seed, smallest (gap between the two lowest losses) / (largest run-to-run change of a loss) over frames 3
# and 4 (frames 1 and 2: > 3000 at every seed) -- seed 0: 0.0004 (the tie), 1: 1.4, 2: 1.3, 3: 1.5, 4: 3.9, 5: 7.8.  Seed 5 has the
# widest margin of those measured; its ten runs picked the same iteration on every frame and agreed to 1.5e-5 in cam_trans
# (profiles/live.md section 6).  With it: 30 raw-against-item pairs in a row passed every assertion below, largest pose difference 2.2e-05.
SEED = 5


def frames_as_bytes(ds, t):
    """Frame ``t`` as a sensor would deliver it (host arrays: colour bytes, float32 depth [H, W]) and as the dataset item that holds
    the same bytes as floats."""
    color, depth, k, pose = ds[t]
    rgb = torch.round(color).clamp(0, 255).to(torch.uint8)
    return (rgb.cpu().numpy().copy(), depth[..., 0].cpu().numpy().copy()), (rgb.to(torch.float32), depth, k, pose)


@pytest.mark.parametrize("case", ["base", "gtposes"])
def test_the_golden_loop_frame_by_frame(case):
    from splatam_amd import pipeline, session
    cfg = LT.load_config(GOLD, case)
    ds = LT.RecordedRGBDSequence(GOLD, case, device="cuda")
    seed_everything(cfg['seed'])
    results = []
    with session.SlamSession(cfg, len(ds), engine="fused") as s:
        for t in range(len(ds)):
            r = s.add_frame(*ds[t])
            assert r['w2c'].device.type == "cuda" and tuple(r['w2c'].shape) == (4, 4)
            results.append(dict(r, w2c=r['w2c'].clone()))
        params, variables, stats = s.finish()
    torch.cuda.synchronize()
    check_decisions(case, cfg, stats, f"{case}/session")
    check_trajectory(case, params, f"{case}/session")
    assert stats['frames_seen'] == len(ds)
    for t, r in enumerate(results):
        assert r['time_idx'] == t and r['keyframe'] == stats['decisions'][t]['keyframe'] and r['num_gaussians'] == stats['num_gaussians'][t]
        assert r['tracking_iters'] == stats['decisions'][t]['tracking_iters'] and r['phase_ms'] is stats['phase_ms'][t]
        assert torch.equal(r['w2c'], pipeline._est_w2c(params, t)), t


def run_base(raw, num_frames=None, frames=None, config=None, watch=None):
    """The "base" frames as bytes through one of the two entries; the planes handed to the loop are cloned after every frame (after the
    caller's arrays were overwritten, on the raw path)."""
    from splatam_amd import session
    cfg = LT.load_config(GOLD, "base") if config is None else config
    ds = LT.RecordedRGBDSequence(GOLD, "base", device="cuda")
    n = len(ds) if num_frames is None else num_frames
    planes, results = [], []
    seed_everything(cfg['seed'])
    with session.SlamSession(cfg, n, engine="fused", device="cuda") as s:
        for t in range(n if frames is None else frames):
            (rgb, depth), item = frames_as_bytes(ds, t)
            if raw:
                results.append(s.add_raw_frame(rgb, depth, item[2].cpu().numpy(), pose=None))
                rgb[:], depth[:] = 255 - rgb, np.float32(-7.0)          # the caller's arrays are its own again
            else:
                results.append(s.add_frame(item[0], item[1], item[2], None))
            if watch is not None:
                watch(s, t, frames_as_bytes(ds, t)[0])
            planes.append(tuple(p.clone() for p in s.last_frame['full']))
        params, variables, stats = s.finish()
    torch.cuda.synchronize()
    return params, stats, planes, results


def seeded_config():
    cfg = LT.load_config(GOLD, "base")
    cfg['seed'] = SEED
    return cfg


@pytest.fixture(scope="module")
def raw_and_item():
    return run_base(raw=False, config=seeded_config()), run_base(raw=True, config=seeded_config())


def test_raw_frames_hand_the_loop_the_planes_of_the_item_path(raw_and_item):
    (_, _, planes_item, _), (_, _, planes_raw, _) = raw_and_item
    ds = LT.RecordedRGBDSequence(GOLD, "base")
    assert len(planes_item) == len(planes_raw) == len(ds)
    for t, ((ia, da), (ib, db)) in enumerate(zip(planes_item, planes_raw)):
        assert tuple(ib.shape) == (3, 64, 96) and tuple(db.shape) == (1, 64, 96)
        assert torch.equal(ia.view(torch.int32), ib.view(torch.int32)), t
        assert torch.equal(da.view(torch.int32), db.view(torch.int32)), t
        rgb = torch.round(ds[t][0]).numpy().astype(np.float32)
        assert np.array_equal(ib.cpu().numpy(), rgb.transpose(2, 0, 1) / np.float32(255))       # ... and they are byte / 255
        assert np.array_equal(db.cpu().numpy()[0], ds[t][1][..., 0].numpy())


def test_raw_frames_take_the_item_paths_decisions(raw_and_item):
    (pa, sa, _, _), (pb, sb, _, results) = raw_and_item
    assert sa['keyframe_time_indices'] == sb['keyframe_time_indices'] and sa['redone_iterations'] == sb['redone_iterations'] == 0
    for a, b in zip(sa['decisions'], sb['decisions']):
        for k in ('time_idx', 'tracking_iters', 'selected', 'views', 'keyframe'):
            assert a[k] == b[k], (a['time_idx'], k)
        assert [p[0] for p in a['prunes']] == [p[0] for p in b['prunes']]
        pairs = [(a['rows_after_add'], b['rows_after_add']), (a['rows_end'], b['rows_end'])]
        pairs += [(x, y) for pa_, pb_ in zip(a['prunes'], b['prunes']) for x, y in zip(pa_[1:], pb_[1:])]
        assert all(close_rows(x, y) for x, y in pairs), (a, b)
    assert [r['time_idx'] for r in results] == list(range(len(results)))


def test_raw_frames_reach_the_item_paths_poses(raw_and_item):
    """Poses of the raw run against the item run within 2e-4, the bound the golden test gives a run against the recording, at a seed
    where no best-candidate pick is a tie (``SEED``)."""
    (pa, _, _, _), (pb, _, _, _) = raw_and_item
    worst = {k: float((pa[k] - pb[k]).detach().abs().max()) for k in ('cam_unnorm_rots', 'cam_trans')}
    per_frame = [round(float((pa['cam_trans'][..., t] - pb['cam_trans'][..., t]).detach().abs().max()), 7) for t in range(pa['cam_trans'].shape[-1])]
    print(f"raw against item: max |difference| {worst}; cam_trans per frame {per_frame}")
    for k, d in worst.items():
        assert d < 2e-4, (k, d, per_frame)


@pytest.mark.parametrize("map_every,adding", [(1, [0, 1, 2, 3]), (2, [0, 1, 3])])
def test_a_densification_size_of_its_own_is_written_from_the_raw_frame(map_every, adding):
    """... and only on the first frame and on frames that add Gaussians: with ``map_every=2`` frame 2 adds nothing."""
    from splatam_amd import fused, pipeline
    cfg = pipeline.splatam_s_config(width=96, height=64, tracking_iters=4, mapping_iters=4, keyframe_every=2, mapping_window_size=4,
                                    map_every=map_every)
    seen = []

    def watch(s, t, raw):
        got = s.last_frame['densify']
        assert s.last_frame['tracking'] is None                     # (SplaTAM-S tracks at the full size)
        if t not in adding:
            assert got is None
            return
        want = fused.ingest_planes(torch.from_numpy(raw[0]).cuda(), torch.from_numpy(raw[1]).cuda(), size=(32, 48))
        assert tuple(got[0].shape) == (3, 32, 48) and tuple(got[1].shape) == (1, 32, 48)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
        seen.append(t)
    params, stats, _, _ = run_base(raw=True, num_frames=4, config=cfg, watch=watch)
    assert seen == adding and stats['frames_seen'] == 4 and stats['redone_iterations'] == 0
    assert [d['rows_after_add'] is not None for d in stats['decisions']] == [t in adding and t > 0 for t in range(4)]
    assert stats['num_gaussians'][0] <= 32 * 48                    # the first point cloud came from the densification frame


def test_a_flagged_phase_is_run_again_by_the_frame_loop():
    """Per-tile buckets forced far too small between two frames (stride 64, longest list 40, on a map of one Gaussian per pixel: the
    means of test_gpu_fused.py::test_flagged_iterations_take_no_adam_step_and_are_counted -- a flag, not a fault): every tracking
    iteration of frame 1 is flagged and takes no Adam step, ``FusedEngine.settle`` takes the pose optimizer's step count back, and the
    loop runs the phase again on exact lists.  The frame then reports the configured number of iterations, both step counts stand
    where an undisturbed frame leaves them, and no flag is left behind.  (The mapping optimizer's count of such a frame is 3, not 4:
    iteration 0 is on the Replica pruning schedule -- ``start_after=0, prune_every=20`` -- and an iteration that prunes takes no Adam
    step; frame 0, which nothing disturbs, is held to the same number.)"""
    from splatam_amd import pipeline, session
    W, H, f = 256, 192, 224.0
    ds = pipeline.SyntheticRGBDSequence(12000, W, H, f, f, W / 2 - 0.5, H / 2 - 0.5, num_frames=2, seed=2, step_m=0.012, step_deg=0.4)
    cfg = pipeline.replica_config(tracking_iters=4, mapping_iters=4)
    seed_everything(cfg['seed'])
    with session.SlamSession(cfg, 2, engine="fused") as s:
        s.add_frame(*ds[0])
        eng = s.engine
        assert s.stats['redone_iterations'] == 0 and eng.map_step == 3
        eng.tile_stride, eng.max_list_hint = 64, 40
        r = s.add_frame(*ds[1])
        stats = s.stats
        print(f"redone iterations {stats['redone_iterations']}, pose_step {eng.pose_step}, map_step {eng.map_step}")
        assert stats['redone_iterations'] > 0                       # the premise: a phase of the loop was flagged and run again
        assert r['tracking_iters'] == 4 and stats['decisions'][1]['tracking_iters'] == 4
        assert eng.pose_step == 4 and eng.map_step == 3
        assert not eng.check_overflow(grow=False)
        s.finish()


def test_an_early_finish_and_a_frame_too_many():
    n = GOLD["base/frames/color"].shape[0]
    params, stats, _, _ = run_base(raw=True, num_frames=n, frames=n - 3)
    cfg = LT.load_config(GOLD, "base")
    assert stats['frames_seen'] == n - 3
    assert params['cam_unnorm_rots'].shape == (1, 4, n - 3) and params['cam_trans'].shape == (1, 3, n - 3)
    assert stats['keyframe_time_indices'] == [t for t in range(n - 3) if t == 0 or (t + 1) % cfg['keyframe_every'] == 0 or t == n - 2]
    from splatam_amd import session
    ds = LT.RecordedRGBDSequence(GOLD, "gtposes", device="cuda")
    with session.SlamSession(LT.load_config(GOLD, "gtposes"), 2, engine="fused") as s:
        s.add_frame(*ds[0])
        s.add_frame(*ds[1])
        with pytest.raises(RuntimeError, match="num_frames = 2"):
            s.add_frame(*ds[2])
        assert s.finish()[2]['frames_seen'] == 2


def test_a_pose_with_nan_on_a_keyframe_frame_stores_no_keyframe():
    from splatam_amd import session
    cfg = LT.load_config(GOLD, "base")
    cfg['tracking']['num_iters'] = cfg['mapping']['num_iters'] = 2
    ds = LT.RecordedRGBDSequence(GOLD, "base", device="cuda")
    seed_everything(cfg['seed'])
    with session.SlamSession(cfg, 3, engine="fused") as s:
        assert s.add_frame(*ds[0])['keyframe']
        color, depth, k, pose = ds[1]
        bad = pose.clone()
        bad[1, 3] = float("nan")
        assert not s.add_frame(color, depth, k, bad)['keyframe']     # (time index num_frames - 2: a keyframe frame by the rule)
        assert s.add_frame(*ds[2])['keyframe'] == ((2 + 1) % cfg['keyframe_every'] == 0)
        _, _, stats = s.finish()
    assert 1 not in stats['keyframe_time_indices'] and stats['keyframe_time_indices'][0] == 0
