"""The exact checkpoint of a session (``SlamSession.save_checkpoint`` / ``restore``) on the CPU: ``engine="dropin"`` with the C oracle
behind ``Renderer``, on the frames of tests/golden/loop_reference.npz, set up as tests/test_loop_golden.py.  On the CPU the loop is
deterministic, so "as if the run had never stopped" is checked BIT FOR BIT: first the premise (two straight runs are equal), then a
run saved after frame 2, restored in a process state reseeded to other values and continued, against the straight run --
``params``, ``variables``, ``keyframe_time_indices`` and ``stats['decisions']`` with ``torch.equal`` / ``==``."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import loop_trace as LT
from test_loop_golden import GOLD, seed_everything

T = 2


def dataset(case="base"):
    return LT.RecordedRGBDSequence(GOLD, case)


def small_s_config(case="base"):
    """``splatam_s_config`` scaled to the case: densification at half the frame's size, as SplaTAM-S has it, and tracking at half size
    too (a tracking size of its own), few iterations."""
    from splatam_amd import pipeline
    H, W = GOLD[f"{case}/frames/color"].shape[1:3]
    cfg = pipeline.splatam_s_config(width=W, height=H, tracking_iters=4, mapping_iters=4, keyframe_every=2, mapping_window_size=4)
    cfg['data'].update(tracking_image_height=H // 2, tracking_image_width=W // 2)
    return cfg


def feed(session, ds, frames, save_at=None, directory=None, keyframes=None):
    for t in frames:
        session.add_frame(*ds[t])
        if t == save_at:
            session.save_checkpoint(directory, keyframes=keyframes)
    return session.finish()


def straight(cfg, ds, n, seed, **save):
    from oracle import c_ref
    from splatam_amd import slam
    from splatam_amd.session import SlamSession
    saved, slam.Renderer = slam.Renderer, c_ref.CRasterizer
    try:
        seed_everything(seed)
        session = SlamSession(copy.deepcopy(cfg), n, engine="dropin", return_pose=False, reference_division=True)
        return feed(session, ds, range(n), **save) + (session,)
    finally:
        slam.Renderer = saved


def continued(cfg, ds, directory, frames, **kw):
    from oracle import c_ref
    from splatam_amd import slam
    from splatam_amd.session import SlamSession
    saved, slam.Renderer = slam.Renderer, c_ref.CRasterizer
    try:
        seed_everything(987654)                  # another process state: the restore sets the streams itself
        random.random(), np.random.rand(3), torch.rand(5)
        session = SlamSession.restore(copy.deepcopy(cfg), directory, T, engine="dropin", return_pose=False, **kw)
        assert session.frames_seen == T + 1
        return feed(session, ds, frames) + (session,)
    finally:
        slam.Renderer = saved


def assert_same_run(a, b):
    pa, va, sa = a[:3]
    pb, vb, sb = b[:3]
    assert set(pa) == set(pb)
    for k in pa:
        assert torch.equal(pa[k].detach(), pb[k].detach()), k
    keys = set(va) - {'means2D'}
    assert keys == set(vb) - {'means2D'} and {'timestep', 'max_2D_radius', 'scene_radius'} <= keys
    for k in keys:
        assert torch.equal(va[k].detach(), vb[k].detach()), k
    assert sa['keyframe_time_indices'] == sb['keyframe_time_indices']
    assert sa['decisions'] == sb['decisions'] and sa['num_gaussians'] == sb['num_gaussians']
    assert sa['tracking_iters'] == sb['tracking_iters'] and sa['mapping_iters'] == sb['mapping_iters'] and sa['frames_seen'] == sb['frames_seen']


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """(config, frames, directory of the checkpoint of frame 2, the straight run that wrote it)."""
    cfg, ds = LT.load_config(GOLD, "base"), dataset()
    directory = str(tmp_path_factory.mktemp("exact_base"))
    run = straight(cfg, ds, len(ds), cfg['seed'], save_at=T, directory=directory)
    return cfg, ds, directory, run


def test_premise_two_straight_runs_are_bit_equal(base):
    cfg, ds, directory, run = base
    assert_same_run(run, straight(cfg, ds, len(ds), cfg['seed']))         # (... and saving a checkpoint on the way changed nothing)
    assert run[2]['keyframe_time_indices'] == GOLD["base/final/keyframe_time_indices"].tolist()


def test_continued_run_is_the_straight_run(base):
    cfg, ds, directory, run = base
    assert sorted(os.listdir(directory)) == [f"keyframe_time_indices{T}.npy", f"params{T}.npz", f"session{T}.npz"]    # keyframes: off for add_frame
    again = continued(cfg, ds, directory, range(T + 1, len(ds)), dataset=ds)
    assert_same_run(run, again)
    assert len(again[2]['phase_ms']) == len(again[2]['frame_s']) == len(ds)              # finish() reports the whole run


def test_nothing_is_pickled(base):
    cfg, ds, directory, run = base
    with np.load(os.path.join(directory, f"session{T}.npz"), allow_pickle=False) as z:
        entries = {k: z[k] for k in z.files}
    assert all(v.dtype != object for v in entries.values())
    assert {'meta', 'var/timestep', 'var/scene_radius', 'first_frame_w2c', 'intrinsics', 'keyframe_est_w2c', 'rng/python', 'rng/numpy',
            'rng/torch_cpu'} <= set(entries)
    import json
    meta = json.loads(str(entries['meta']))
    assert meta['frames_seen'] == T + 1 and meta['frame_size'] == list(GOLD["base/frames/color"].shape[1:3])
    assert len(meta['stats']['decisions']) == T + 1 and meta['reference_division'] is True
    # the reference's pair beside it is the reference's format: every entry of params, nothing else
    with np.load(os.path.join(directory, f"params{T}.npz"), allow_pickle=False) as z:
        assert set(z.files) == {'means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales', 'cam_unnorm_rots', 'cam_trans'}


def test_sizes_of_their_own_and_keyframes_from_the_checkpoint(tmp_path):
    """Tracking and densification at sizes of their own, ``keyframes=True``, restored WITHOUT a dataset: the planes come back bit for
    bit and the continued run is the straight one."""
    cfg, ds = small_s_config(), dataset()
    directory = str(tmp_path / "ckpt")
    run = straight(cfg, ds, len(ds), 5, save_at=T, directory=directory, keyframes=True)
    assert f"keyframes{T}.npz" in os.listdir(directory)
    assert run[3]._tracking_frames is not None and run[3]._densify_frames is not None
    again = continued(cfg, ds, directory, range(T + 1, len(ds)))
    assert_same_run(run, again)
    originals = {kf['id']: kf for kf in run[3].keyframe_list}
    restored = [kf for kf in again[3].keyframe_list if kf['id'] <= T]
    assert [kf['id'] for kf in restored] == [0, 1]
    for kf in restored:
        for k in ('color', 'depth', 'est_w2c'):
            assert kf[k].dtype == torch.float32 and torch.equal(kf[k], originals[kf['id']][k]), (kf['id'], k)
    with np.load(os.path.join(directory, f"keyframes{T}.npz"), allow_pickle=False) as z:
        assert int(z['count']) == 2 and z['color0'].dtype == np.float32 and z['depth1'].shape == (1,) + GOLD["base/frames/color"].shape[1:3]
    # the reduced sizes are part of what a restore compares
    other = copy.deepcopy(cfg)
    other['data'].update(tracking_image_height=16, tracking_image_width=24)
    with pytest.raises(ValueError, match="tracking_size"):
        continued(other, ds, directory, ())
    other = copy.deepcopy(cfg)
    del other['data']['densification_image_height'], other['data']['densification_image_width']
    with pytest.raises(ValueError, match="densification_size"):
        continued(other, ds, directory, ())


def test_a_finished_map_is_continued_with_more_frames(tmp_path):
    """A session declared with three frames, finished and saved; restored with ``num_frames=5`` and fed two more: the straight run
    declared with five from the start (``keyframe_every=2``: the ``num_frames - 2`` rule names frames that are keyframes anyway)."""
    cfg, ds = LT.load_config(GOLD, "base"), dataset()
    directory = str(tmp_path / "ckpt")
    short = straight(cfg, ds, T + 1, cfg['seed'], save_at=T, directory=directory)
    assert short[0]['cam_trans'].shape[-1] == T + 1
    full = straight(cfg, ds, len(ds), cfg['seed'])
    again = continued(cfg, ds, directory, range(T + 1, len(ds)), dataset=ds, num_frames=len(ds))
    assert again[0]['cam_trans'].shape[-1] == len(ds)
    assert_same_run(full, again)


def test_refusals_name_the_entry(base, tmp_path):
    from splatam_amd.session import SlamSession
    cfg, ds, directory, run = base
    with pytest.raises(ValueError, match="num_frames"):
        SlamSession.restore(cfg, directory, T, num_frames=T, dataset=ds, engine="dropin")
    with pytest.raises(ValueError, match="engine_family"):
        SlamSession.restore(cfg, directory, T, dataset=ds, engine="fused")
    with pytest.raises(NotImplementedError, match="plugin"):
        SlamSession.restore(cfg, directory, T, dataset=ds, engine="plugin")
    other = copy.deepcopy(cfg)
    other['gaussian_distribution'] = "anisotropic"
    with pytest.raises(ValueError, match="gaussian_distribution"):
        SlamSession.restore(other, directory, T, dataset=ds, engine="dropin")
    other = copy.deepcopy(cfg)
    other['data'].update(desired_image_height=32, desired_image_width=48)
    with pytest.raises(ValueError, match="frame_size"):
        SlamSession.restore(other, directory, T, dataset=ds, engine="dropin")
    with pytest.raises(ValueError, match="reference_division"):
        SlamSession.restore(cfg, directory, T, dataset=ds, engine="dropin", reference_division=False)
    with pytest.raises(ValueError, match=f"keyframes{T}.npz"):                 # neither the planes' file nor a dataset
        SlamSession.restore(cfg, directory, T, engine="dropin")
    with pytest.raises(FileNotFoundError, match="session4.npz"):
        SlamSession.restore(cfg, directory, 4, dataset=ds, engine="dropin")
    with pytest.raises(RuntimeError, match="first frame"):
        SlamSession(cfg, 3, engine="dropin").save_checkpoint(str(tmp_path))


def test_a_failed_write_raises_where_the_writer_is_joined(tmp_path):
    from oracle import c_ref
    from splatam_amd import slam
    from splatam_amd.session import SlamSession
    cfg, ds = LT.load_config(GOLD, "base"), dataset()
    blocked = tmp_path / "file"
    blocked.write_text("not a directory")
    saved, slam.Renderer = slam.Renderer, c_ref.CRasterizer
    try:
        seed_everything(0)
        session = SlamSession(cfg, 2, engine="dropin")
        session.add_frame(*ds[0])
        session.save_checkpoint(str(blocked / "sub"))
        with pytest.raises(RuntimeError, match="writing a checkpoint failed"):
            session.finish()
    finally:
        slam.Renderer = saved


def test_rgbd_slam_resume_exact(base):
    from oracle import c_ref
    from splatam_amd import pipeline, slam
    cfg, ds, directory, run = base
    saved, slam.Renderer = slam.Renderer, c_ref.CRasterizer
    try:
        seed_everything(4242)
        again = pipeline.rgbd_slam(ds, copy.deepcopy(cfg), engine="dropin", checkpoint_dir=directory, resume_exact=T)
        with pytest.raises(ValueError, match="checkpoint_dir"):
            pipeline.rgbd_slam(ds, pipeline.replica_config(), engine="dropin", resume_exact=T)
    finally:
        slam.Renderer = saved
    assert_same_run(run, again)
