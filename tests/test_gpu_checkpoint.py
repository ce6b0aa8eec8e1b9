"""Checkpoints on the fused engine (HIP).

  * ``load_checkpoint`` from the files the REFERENCE wrote (tests/golden/loop_resume_reference.npz) against the recording of the
    reference's own resumed run, with ``check_decisions`` / ``check_trajectory`` of tests/test_gpu_loop_golden.py -- its ``ROW_TOL``, its
    pose bound, its share of differing ``timestep`` rows: the functions themselves are called, on the resumed recording.
  * The exact form: a run saved after frame 2, restored and continued, against the straight run within those same bounds (two runs of
    one loop whose backward composites add floats atomically are not bit-equal), with ``redone_iterations`` and the views of every
    mapping iteration EQUAL -- the random stream went on where it stopped.
  * A live session (``add_raw_frame``) of four small frames saved with its keyframes and restored without a dataset.
  * A frame that does not checkpoint allocates nothing."""
import copy
import gc
import os

import numpy as np
import pytest
import torch

import loop_trace as LT
import test_gpu_loop_golden as G
from test_loop_golden import GOLD, seed_everything
from test_resume_golden import CASES, RESUME, T, reference_files

pytestmark = pytest.mark.gpu


class _Overlay:
    """``GOLD`` with some entries replaced: what ``check_decisions`` / ``check_trajectory`` read as the yardstick."""

    def __init__(self, over):
        self.over = over

    def __getitem__(self, key):
        return self.over[key] if key in self.over else GOLD[key]


def against(monkeypatch, case, over):
    monkeypatch.setattr(G, "GOLD", _Overlay({f"{case}/{k}": v for k, v in over.items()}))


@pytest.mark.parametrize("case", CASES)
def test_fused_engine_resumes_from_the_references_files(case, tmp_path, monkeypatch):
    from splatam_amd import pipeline
    reference_files(str(tmp_path), case)
    cfg = LT.load_config(RESUME, case)
    ds = LT.RecordedRGBDSequence(GOLD, case, device="cuda")
    seed_everything(cfg['seed'])
    params, variables, stats = pipeline.rgbd_slam(ds, cfg, engine="fused", checkpoint_dir=str(tmp_path))
    torch.cuda.synchronize()
    against(monkeypatch, case, {k[len(case) + 1:]: RESUME[k] for k in RESUME.files if k.startswith(case + "/")})
    table = G.gold_decisions(case, cfg)
    assert [d['time_idx'] for d in stats['decisions']] == list(range(T, len(ds)))
    # (the recording starts at frame 2: the frames before it are the table's own rows, so that only the resumed frames are compared)
    G.check_decisions(case, cfg, dict(stats, decisions=table[:T] + stats['decisions']), f"{case}/fused resumed at {T}")
    G.check_trajectory(case, params, f"{case}/fused resumed at {T}")
    assert stats['keyframe_time_indices'] == ([0, 2, 2, 4, 5] if case == "variant" else [0, 1, 3])
    want = RESUME[f"{case}/final/timestep"]
    n = min(variables['timestep'].shape[0], want.shape[0])
    assert float((variables['timestep'][:n].cpu().numpy() != want[:n]).mean()) < 2e-2
    assert float(variables['timestep'][:n // 2].max()) == 0.0                       # zeroed by the load, like the reference's


def fused_session(cfg, n, **kw):
    from splatam_amd.session import SlamSession
    return SlamSession(copy.deepcopy(cfg), n, engine="fused", gaussian_capacity=20000, return_pose=False, reference_division=True, **kw)


def compare_runs(monkeypatch, case, cfg, straight, again, what):
    """``again`` against ``straight`` with the golden test's own comparisons: the straight run's decisions and poses as the yardstick."""
    (pa, va, sa), (pb, vb, sb) = straight, again
    assert sa['redone_iterations'] == sb['redone_iterations'] == 0
    assert [d['views'] for d in sa['decisions']] == [d['views'] for d in sb['decisions']]
    assert [d['selected'] for d in sa['decisions']] == [d['selected'] for d in sb['decisions']]
    against(monkeypatch, case, {'final/cam_unnorm_rots': pa['cam_unnorm_rots'].detach().cpu().numpy(),
                                'final/cam_trans': pa['cam_trans'].detach().cpu().numpy(),
                                'final/keyframe_time_indices': np.array(sa['keyframe_time_indices'])})
    monkeypatch.setattr(G, "gold_decisions", lambda case_, cfg_: sa['decisions'])
    G.check_decisions(case, cfg, sb, what)
    G.check_trajectory(case, pb, what)
    n = min(va['timestep'].shape[0], vb['timestep'].shape[0])
    assert float((va['timestep'][:n] != vb['timestep'][:n]).float().mean()) < 2e-2


def test_exact_checkpoint_continues_the_fused_run(tmp_path, monkeypatch):
    from splatam_amd.session import SlamSession
    case = "base"
    cfg = LT.load_config(GOLD, case)
    ds = LT.RecordedRGBDSequence(GOLD, case, device="cuda")
    directory = str(tmp_path)
    seed_everything(cfg['seed'])
    with fused_session(cfg, len(ds)) as s:
        for t in range(len(ds)):
            s.add_frame(*ds[t])
            if t == T:
                s.save_checkpoint(directory)
                sizing = s.engine.list_sizing()
        straight = s.finish()
    assert straight[2]['redone_iterations'] == 0                 # the premise: at this capacity the straight run alone flags nothing
    assert sorted(os.listdir(directory)) == [f"keyframe_time_indices{T}.npy", f"params{T}.npz", f"session{T}.npz"]
    seed_everything(987654)
    torch.rand(7, device="cuda"), np.random.rand(3)
    s = SlamSession.restore(copy.deepcopy(cfg), directory, T, dataset=ds, engine="fused", return_pose=False)
    assert s.frames_seen == T + 1 and s.engine.list_sizing() == sizing and s.reference_division is True
    with s:
        for t in range(T + 1, len(ds)):
            s.add_frame(*ds[t])
        again = s.finish()
    torch.cuda.synchronize()
    assert again[2]['decisions'][:T + 1] == straight[2]['decisions'][:T + 1] and len(again[2]['frame_s']) == len(ds)
    compare_runs(monkeypatch, case, cfg, straight, again, "base/fused continued")
    # ... and, for scale, the straight run itself against the reference's recording
    monkeypatch.undo()
    G.check_trajectory(case, straight[0], "base/fused straight")


def raw_frame(ds, t):
    from test_gpu_session import frames_as_bytes
    (rgb, depth), item = frames_as_bytes(ds, t)
    return rgb, depth, item[2].cpu().numpy()


def test_a_live_session_survives_a_save_and_restore(tmp_path, monkeypatch):
    from splatam_amd import _capi
    from splatam_amd.session import SlamSession
    from test_gpu_session import seeded_config
    cfg, n, at = seeded_config(), 4, 1
    ds = LT.RecordedRGBDSequence(GOLD, "base", device="cuda")
    directory = str(tmp_path)

    def session():
        return SlamSession(copy.deepcopy(cfg), n, engine="fused", device="cuda", gaussian_capacity=20000, return_pose=False)
    seed_everything(cfg['seed'])
    with session() as s:
        for t in range(n):
            s.add_raw_frame(*raw_frame(ds, t), pose=None)
            if t == at:
                s.save_checkpoint(directory)                     # (keyframes: the default of a raw session)
                assert s.join_checkpoint()['keyframes'] > 2 * 16 * 64 * 96
        originals = [dict(kf) for kf in s.keyframe_list]
        straight = s.finish()
    assert f"keyframes{at}.npz" in os.listdir(directory)
    seed_everything(13579)
    s = SlamSession.restore(copy.deepcopy(cfg), directory, at, engine="fused", device="cuda", return_pose=False)     # no dataset
    assert [kf['id'] for kf in s.keyframe_list] == [0, 1]
    for kf, orig in zip(s.keyframe_list, originals):
        for k in ('color', 'depth', 'est_w2c'):
            assert kf[k].dtype == torch.float32 and torch.equal(kf[k].view(torch.int32), orig[k].view(torch.int32)), (kf['id'], k)
    with s:
        for t in range(at + 1, n):
            s.add_raw_frame(*raw_frame(ds, t), pose=None)
        image = s.render_view(follow=True)
        assert tuple(image.rgb8.shape) == (64, 96, 3) and int(image.rgb8.max()) > 0
        row = torch.zeros(_capi.SPLAT_EVAL_ROW, dtype=torch.float64, device="cuda")
        im, depth = s.last_frame['full']
        s.engine.evaluate_frame(s._curr_data(n - 1, im, depth), n - 1, row, cfg['mapping']['sil_thres'], ms_ssim=False)
        row = row.cpu().numpy()
        print(f"restored live session: PSNR of the last frame {row[_capi.SPLAT_EVAL_PSNR]:.2f} dB, {int(row[_capi.SPLAT_EVAL_VALID])} valid pixels")
        assert np.isfinite(row[_capi.SPLAT_EVAL_PSNR]) and row[_capi.SPLAT_EVAL_VALID] > 0 and row[_capi.SPLAT_EVAL_FLAGGED] == 0
        again = s.finish()
    assert again[2]['frames_seen'] == n
    compare_runs(monkeypatch, "base", cfg, straight, again, "base/raw continued")


def test_a_frame_that_does_not_checkpoint_allocates_nothing(tmp_path, monkeypatch):
    """Frames 0 and 1 warm the session up (1 is a keyframe frame), a checkpoint is written, frame 2 -- no keyframe, no checkpoint -- must
    leave ``torch.cuda.memory_allocated`` where it was, and the checkpoint's host buffers untouched.  The loop's own one allocation per
    NEW view, the launch order a camera keeps for it (``_Camera.select_order``: 512 B at this size, measured as the whole difference of
    this frame), is switched off for the session, so that the comparison is exact."""
    monkeypatch.setenv("SPLAT_TILE_ORDER_PER_VIEW", "0")
    cfg = LT.load_config(GOLD, "base")
    ds = LT.RecordedRGBDSequence(GOLD, "base", device="cuda")
    seed_everything(cfg['seed'])
    with fused_session(cfg, len(ds), device="cuda") as s:
        for t in (0, 1):
            s.add_raw_frame(*raw_frame(ds, t), pose=None)
        s.save_checkpoint(str(tmp_path))
        s.join_checkpoint()
        pinned = {k: v.data_ptr() for k, v in s._host._pinned.items()}
        frame = raw_frame(ds, 2)
        gc.collect()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        r = s.add_raw_frame(*frame, pose=None)
        gc.collect()
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
        print(f"allocated before frame 2: {before} B, after: {after} B")
        assert not r['keyframe'] and s._writer._thread is None
        assert after == before
        assert {k: v.data_ptr() for k, v in s._host._pinned.items()} == pinned and len(s._kf_host) == 2
        s.finish()
