"""The reference's checkpoint keys held to a recording of the REFERENCE'S OWN resumed ``rgbd_slam`` (tests/golden/loop_resume_reference.npz:
/root/reference/scripts/splatam.py executed by tests/golden/make_golden_resume.py on the C oracle, first with ``save_checkpoints``,
then with ``load_checkpoint=True, checkpoint_time_idx=2``).  CPU, ``engine="dropin"`` with the same oracle behind ``Renderer``, set up
as tests/test_loop_golden.py; its comparisons and tolerances are the ones applied here.

  * resuming FROM THE FILES THE REFERENCE WROTE makes the reference's resumed calls in its order (the loop restarts AT frame 2; in
    ``variant`` that frame is a keyframe and its index ends up in ``keyframe_time_indices`` twice), with its losses and final state;
  * a straight run here with the keys on writes files with the reference's names, keys, shapes and dtypes;
  * ``run.run()`` over a sequence on disk honours all four keys.
"""
import os

import numpy as np
import pytest
import torch

import dataset_files as files
import loop_trace as LT
from test_loop_golden import GOLD, seed_everything

RESUME = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_resume_reference.npz"))
CASES = ("base", "variant")
T = 2
MAP_KEYS = ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales')


def reference_files(directory, case):
    """The two files the reference wrote at ``t = 2``, written again from the recorded arrays."""
    os.makedirs(directory, exist_ok=True)
    prefix = f"{case}/ckpt/params/"
    np.savez(os.path.join(directory, f"params{T}.npz"), **{k[len(prefix):]: RESUME[k] for k in RESUME.files if k.startswith(prefix)})
    np.save(os.path.join(directory, f"keyframe_time_indices{T}.npy"), RESUME[f"{case}/ckpt/keyframe_time_indices"])


def run_on_oracle(cfg, case, directory, record=True, **kw):
    from oracle import c_ref
    from splatam_amd import pipeline, slam
    ds = LT.RecordedRGBDSequence(GOLD, case)
    saved = slam.Renderer
    slam.Renderer = c_ref.CRasterizer
    rec = LT.LoopRecorder().wrap(slam).wrap(pipeline) if record else None
    try:
        seed_everything(cfg['seed'])
        params, variables, stats = pipeline.rgbd_slam(ds, cfg, engine="dropin", checkpoint_dir=directory, **kw)
    finally:
        if rec is not None:
            rec.restore()
        slam.Renderer = saved
    return rec, params, variables, stats


@pytest.fixture(scope="module", params=CASES)
def resumed(request, tmp_path_factory):
    case = request.param
    directory = str(tmp_path_factory.mktemp(f"reference_{case}"))
    reference_files(directory, case)
    cfg = LT.load_config(RESUME, case)
    assert cfg['load_checkpoint'] is True and cfg['checkpoint_time_idx'] == T
    return (case, cfg) + run_on_oracle(cfg, case, directory)


def test_resumed_call_sequence_equals_the_reference(resumed):
    case, cfg, rec, params, variables, stats = resumed
    events, values, selected = rec.arrays()
    diff = LT.first_difference(RESUME[f"{case}/events"], events)
    assert diff is None, f"{case}: reference vs pipeline, resumed at {T}: {diff[1]}"
    assert selected.tolist() == RESUME[f"{case}/selected"].tolist()
    want = RESUME[f"{case}/final/keyframe_time_indices"].tolist()
    assert stats['keyframe_time_indices'] == want
    # the restart AT t: frame 2 ran again; where it is a keyframe frame its index is in the list twice
    assert [d['time_idx'] for d in stats['decisions']] == list(range(T, GOLD[f"{case}/frames/color"].shape[0]))
    assert want == ([0, 2, 2, 4, 5] if case == "variant" else [0, 1, 3])
    n = GOLD[f"{case}/frames/color"].shape[0]
    table = LT.per_frame_decisions(RESUME[f"{case}/events"], RESUME[f"{case}/selected"], sorted(set(want)), n, cfg['mapping']['pruning_dict'])
    assert stats['decisions'] == table[T:]


def test_resumed_losses_follow_the_reference(resumed):
    """The bounds of tests/test_loop_golden.py::test_losses_follow_the_reference_loop."""
    case, cfg, rec, params, variables, stats = resumed
    events, values, _ = rec.arrays()
    gold_v = RESUME[f"{case}/values"]
    is_loss = events[:, 0] == LT.LOSS
    rel = np.abs(values[is_loss] - gold_v[is_loss]) / np.abs(gold_v[is_loss])
    print(f"{case}: {int(is_loss.sum())} losses, relative difference: first three {rel[:3].max():.1e}, median {np.median(rel):.1e}, max {rel.max():.1e}")
    assert rel[:3].max() < 1e-6 and np.median(rel) < 2e-5 and rel.max() < 2e-3


def check_state(case, cfg, want, got, steps, what):
    """The bounds of tests/test_loop_golden.py::test_final_state_equals_the_reference_loop; ``want`` / ``got``: arrays by name."""
    for k in MAP_KEYS:
        assert want[k].shape == got[k].shape and want[k].dtype == got[k].dtype, (what, k)
        d, lr = np.abs(want[k] - got[k]), cfg['mapping']['lrs'][k]
        q50, q99 = np.quantile(d, [0.5, 0.99])
        print(f"{case}: {what}: {k}: |difference| / lr: median {q50 / lr:.1e}, 99 % {q99 / lr:.2f}, max {d.max() / lr:.2f} ({steps} mapping steps)")
        assert q50 <= 0.01 * lr and q99 <= 2 * lr and d.max() <= steps * lr, (what, k)
    for k in ('cam_unnorm_rots', 'cam_trans'):
        assert want[k].shape == got[k].shape and want[k].dtype == got[k].dtype, (what, k)
        d = np.abs(want[k] - got[k])
        print(f"{case}: {what}: {k}: max |difference| {d.max():.1e}")
        assert d.max() < 5e-5, (what, k)


def test_resumed_final_state_equals_the_reference(resumed):
    case, cfg, rec, params, variables, stats = resumed
    prefix = f"{case}/final/"
    want = {k[len(prefix):]: RESUME[k] for k in RESUME.files if k.startswith(prefix)}
    check_state(case, cfg, want, {k: v.detach().numpy() for k, v in params.items()}, stats['mapping_iters'], "resumed")
    # `timestep` was zeroed by the load: the rows of the checkpoint carry 0, the rows added since their frame
    assert np.array_equal(want['timestep'], variables['timestep'].numpy())
    assert (want['timestep'][:RESUME[f"{case}/ckpt/params/means3D"].shape[0] // 2] == 0).all()


@pytest.mark.parametrize("case", CASES)
def test_a_straight_run_writes_the_references_files(case, tmp_path):
    cfg = LT.load_config(GOLD, case)
    cfg.update(save_checkpoints=True, checkpoint_interval=2, load_checkpoint=False)
    directory = str(tmp_path / "run")
    _, params, variables, stats = run_on_oracle(cfg, case, directory, record=False)
    n = GOLD[f"{case}/frames/color"].shape[0]
    names = [f"{stem}{t}.{ext}" for t in range(0, n, 2) for stem, ext in (("params", "npz"), ("keyframe_time_indices", "npy"))]
    assert sorted(os.listdir(directory)) == sorted(names)
    prefix = f"{case}/ckpt/params/"
    want = {k[len(prefix):]: RESUME[k] for k in RESUME.files if k.startswith(prefix)}
    got = dict(np.load(os.path.join(directory, f"params{T}.npz"), allow_pickle=True))              # (as the reference's loader reads it)
    assert set(got) == set(want) and 'timestep' not in got and 'intrinsics' not in got
    steps = sum(len(d['views']) for d in stats['decisions'][:T + 1])
    check_state(case, cfg, want, got, steps, f"params{T}.npz")
    kf = np.load(os.path.join(directory, f"keyframe_time_indices{T}.npy"))
    want_kf = RESUME[f"{case}/ckpt/keyframe_time_indices"]
    assert kf.dtype == want_kf.dtype and kf.tolist() == want_kf.tolist()
    # ... and the last pair holds the final state of this run
    last = n - 1 - (n - 1) % 2
    if last == n - 1:
        final = np.load(os.path.join(directory, f"params{last}.npz"))
        assert all(np.array_equal(final[k], params[k].detach().numpy()) for k in final.files)


def test_refusals_name_the_key_and_a_missing_file_its_path(tmp_path):
    from splatam_amd import pipeline
    cfg = LT.load_config(RESUME, "base")
    ds = LT.RecordedRGBDSequence(GOLD, "base")
    with pytest.raises(FileNotFoundError, match=f"params{T}.npz"):
        pipeline.rgbd_slam(ds, cfg, engine="dropin", checkpoint_dir=str(tmp_path))
    reference_files(str(tmp_path), "base")
    os.remove(str(tmp_path / f"keyframe_time_indices{T}.npy"))
    with pytest.raises(FileNotFoundError, match=f"keyframe_time_indices{T}.npy"):
        pipeline.rgbd_slam(ds, cfg, engine="dropin", checkpoint_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="load_checkpoint"):
        pipeline.rgbd_slam(ds, cfg, engine="plugin", checkpoint_dir=str(tmp_path))
    cfg.update(load_checkpoint=False, save_checkpoints=True, checkpoint_interval=2)
    with pytest.raises(NotImplementedError, match="save_checkpoints"):
        pipeline.rgbd_slam(ds, cfg, engine="plugin", checkpoint_dir=str(tmp_path))


def test_run_honours_the_four_keys(tmp_path):
    """``splatam_amd.run.run`` over the ``base`` frames written to disk as a dataset stores them (8-bit colour, 16-bit depth, Replica
    layout): ``save_checkpoints`` + ``checkpoint_interval`` write the pairs under ``workdir/run_name``; ``load_checkpoint`` +
    ``checkpoint_time_idx`` restart at that frame from them; a checkpoint that was never written is named."""
    from oracle import c_ref
    from splatam_amd import pipeline, run, slam
    scale, root = 6553.5, str(tmp_path / "data")
    color, depth = GOLD["base/frames/color"], GOLD["base/frames/depth"]
    n, H, W = color.shape[:3]
    frames = [(np.rint(color[t]).clip(0, 255).astype(np.uint8), np.rint(depth[t, ..., 0].astype(np.float64) * scale).astype(np.uint16))
              for t in range(n)]
    files.write_replica(root, "room", frames, GOLD["base/frames/poses"].astype(np.float64))
    k = GOLD["base/frames/intrinsics"]
    yaml_path = os.path.join(root, "synthetic.yaml")
    with open(yaml_path, "w") as f:
        f.write(f"dataset_name: 'replica'\ncamera_params:\n  image_height: {H}\n  image_width: {W}\n  fx: {float(k[0, 0])}\n  fy: {float(k[1, 1])}\n"
                f"  cx: {float(k[0, 2])}\n  cy: {float(k[1, 2])}\n  png_depth_scale: {scale}\n")
    cfg = pipeline.replica_config(tracking_iters=3, mapping_iters=3, keyframe_every=2, mapping_window_size=4)
    cfg.update(workdir=str(tmp_path / "experiments"), run_name="room_0", use_wandb=False, eval_every=1, primary_device="cpu",
               save_checkpoints=True, checkpoint_interval=2, load_checkpoint=False, checkpoint_time_idx=0,
               data=dict(basedir=root, gradslam_data_cfg=yaml_path, sequence="room", desired_image_height=H, desired_image_width=W,
                         start=0, end=-1, stride=1, num_frames=-1))
    directory = os.path.join(cfg['workdir'], cfg['run_name'])
    saved, slam.Renderer = slam.Renderer, c_ref.CRasterizer
    try:
        run.seed_everything(cfg['seed'])
        _, _, stats, _ = run.run(cfg, engine="dropin", evaluate=False, prefetch=0)
        pairs = sorted(x for x in os.listdir(directory) if x != "params.npz")
        assert pairs == sorted([f"{stem}{t}.{ext}" for t in (0, 2, 4) for stem, ext in (("params", "npz"), ("keyframe_time_indices", "npy"))])
        assert stats['keyframe_time_indices'] == [0, 1, 3] and len(stats['decisions']) == n
        at_t = dict(np.load(os.path.join(directory, f"params{T}.npz")))
        cfg.update(save_checkpoints=False, load_checkpoint=True, checkpoint_time_idx=T)
        before = {x: os.path.getmtime(os.path.join(directory, x)) for x in pairs}
        run.seed_everything(cfg['seed'])
        params, variables, again, _ = run.run(cfg, engine="dropin", evaluate=False, prefetch=0)
        assert [d['time_idx'] for d in again['decisions']] == list(range(T, n))
        assert again['keyframe_time_indices'] == np.load(os.path.join(directory, f"keyframe_time_indices{T}.npy")).tolist() + [3]
        assert before == {x: os.path.getmtime(os.path.join(directory, x)) for x in pairs}        # save_checkpoints off: nothing written
        # the poses of the frames before the restart are the file's (the mapping learning rates of the poses are 0)
        for key in ('cam_unnorm_rots', 'cam_trans'):
            assert np.array_equal(params[key].detach().numpy()[..., :T], at_t[key][..., :T])
        assert float(variables['timestep'][:at_t['means3D'].shape[0] // 2].max()) == 0.0
        cfg.update(checkpoint_time_idx=3)
        with pytest.raises(FileNotFoundError, match="params3.npz"):
            run.run(cfg, engine="dropin", evaluate=False, prefetch=0)
        # the exact form through the same entry: checkpoints written as exact ones, then continued at T + 1 in another random state
        cfg.update(run_name="room_exact", save_checkpoints=True, load_checkpoint=False)
        run.seed_everything(cfg['seed'])
        straight, _, straight_stats, _ = run.run(cfg, engine="dropin", evaluate=False, prefetch=0, exact_checkpoints=True)
        assert os.path.isfile(os.path.join(cfg['workdir'], "room_exact", f"session{T}.npz"))
        cfg.update(save_checkpoints=False)
        run.seed_everything(97531)
        params, _, again, _ = run.run(cfg, engine="dropin", evaluate=False, prefetch=0, resume_exact=T)
        assert all(torch.equal(straight[key].detach(), params[key].detach()) for key in straight)
        assert again['decisions'] == straight_stats['decisions'] and again['keyframe_time_indices'] == [0, 1, 3]
    finally:
        slam.Renderer = saved
