"""The frame loop with tracking and densification at resolutions of their own, on the HIP engines, held to the recording of the
REFERENCE'S OWN ``rgbd_slam`` run that way (tests/golden/loop_multires_reference.npz; the CPU half is
tests/test_loop_multires_golden.py).  Assertions and bounds are those of tests/test_gpu_loop_golden.py -- ROW_TOL on row counts, 2e-4
on poses, no redone iterations, one engine behind ``plugin_map_edits`` -- plus the frame size of every get_loss / add_new_gaussians
call of the statement engines.  ``fused`` runs once more with the full dataset alone: the sizes in ``config['data']`` then make the
loop derive the reduced frames with the frame-preparation kernel, and the same decisions must follow."""
import numpy as np
import pytest
import torch

import loop_trace as LT
import loop_trace_multires as LM
from test_gpu_loop_golden import ROW_TOL, close_rows
from test_loop_golden import seed_everything
from test_loop_multires_golden import CASES, GOLD

pytestmark = pytest.mark.gpu


def run_engine(case, engine, derive=False):
    from splatam_amd import pipeline, plugin, slam
    cfg = LT.load_config(GOLD, case)
    full, tracking, densify = LM.datasets(GOLD, case, device="cuda")
    rec = LM.SizeRecorder().wrap(slam).wrap(pipeline).wrap(plugin)
    try:
        seed_everything(cfg['seed'])
        if derive:
            params, variables, stats = pipeline.rgbd_slam(full, cfg, engine=engine)
        else:
            params, variables, stats = pipeline.rgbd_slam(full, cfg, engine=engine, tracking_dataset=tracking, densify_dataset=densify)
        torch.cuda.synchronize()
    finally:
        rec.restore()
    return cfg, rec, params, variables, stats


def check_decisions(case, cfg, stats, what):
    n = len(LM.dataset(GOLD, case, "frames"))
    want = LT.per_frame_decisions(GOLD[f"{case}/events"], GOLD[f"{case}/selected"], GOLD[f"{case}/final/keyframe_time_indices"], n,
                                  cfg['mapping']['pruning_dict'])
    got = stats['decisions']
    assert len(want) == len(got)
    worst = 0.0
    for w, g in zip(want, got):
        for k in ('time_idx', 'tracking_iters', 'selected', 'views', 'keyframe'):
            assert w[k] == g[k], (what, w['time_idx'], k, w[k], g[k])
        assert [p[0] for p in w['prunes']] == [p[0] for p in g['prunes']], (what, w['time_idx'], w['prunes'], g['prunes'])
        pairs = [(w['rows_after_add'], g['rows_after_add']), (w['rows_end'], g['rows_end'])]
        pairs += [(x, y) for pw, pg in zip(w['prunes'], g['prunes']) for x, y in zip(pw[1:], pg[1:])]
        for x, y in pairs:
            assert close_rows(x, y), (what, w['time_idx'], w, g)
            if x:
                worst = max(worst, abs(x - y) / x)
    print(f"{what}: decisions equal the reference loop's on {len(want)} frames; largest row-count difference {100 * worst:.3f} % (bound {100 * ROW_TOL} %)")
    assert stats['keyframe_time_indices'] == GOLD[f"{case}/final/keyframe_time_indices"].tolist()
    assert stats['redone_iterations'] == 0


def check_trajectory(case, params, what):
    for k, tol in (('cam_unnorm_rots', 2e-4), ('cam_trans', 2e-4)):
        d = np.abs(GOLD[f"{case}/final/{k}"] - params[k].detach().cpu().numpy())
        print(f"{what}: {k}: max |difference| to the reference loop {d.max():.1e}")
        assert d.max() < tol, (what, k, d.max())


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("engine", ["dropin", "plugin", "plugin_map_edits"])
def test_statement_engines_make_the_reference_loops_calls(case, engine):
    cfg, rec, params, variables, stats = run_engine(case, engine)
    events, values, selected = rec.arrays()
    diff = LT.first_difference(GOLD[f"{case}/events"], events, ignore_row_counts=True)
    assert diff is None, f"{case}/{engine}: reference vs pipeline: {diff[1]}"
    assert selected.tolist() == GOLD[f"{case}/selected"].tolist()
    LM.check_sizes(GOLD, case, rec.size_array())
    check_decisions(case, cfg, stats, f"{case}/{engine}")
    check_trajectory(case, params, f"{case}/{engine}")
    is_loss = events[:, 0] == LT.LOSS
    rel = np.abs(values[is_loss] - GOLD[f"{case}/values"][is_loss]) / np.abs(GOLD[f"{case}/values"][is_loss])
    print(f"{case}/{engine}: {int(is_loss.sum())} losses, relative difference to the reference loop: first {rel[0]:.1e}, median "
          f"{np.median(rel):.1e}, max {rel.max():.1e}")
    assert rel[0] < 1e-4 and np.median(rel) < 2e-3 and rel.max() < 3e-2
    if engine.startswith("plugin"):
        assert stats['plugin']['skipped_iterations'] == 0, stats['plugin']
    if engine == "plugin_map_edits":
        assert stats['plugin']['engines_built'] == 1, stats['plugin']


@pytest.mark.parametrize("derive", [False, True], ids=["recorded datasets", "frames derived by the kernel"])
@pytest.mark.parametrize("case", CASES)
def test_fused_engine_takes_the_reference_loops_decisions(case, derive):
    cfg, rec, params, variables, stats = run_engine(case, "fused", derive=derive)
    check_decisions(case, cfg, stats, f"{case}/fused")
    check_trajectory(case, params, f"{case}/fused")
    n = min(variables['timestep'].shape[0], GOLD[f"{case}/final/timestep"].shape[0])
    ts = variables['timestep'][:n].cpu().numpy()
    assert float((ts != GOLD[f"{case}/final/timestep"][:n]).mean()) < 2e-2
    assert all('prepare_frames' in fr for fr in stats['phase_ms'])


def test_several_ranks_with_separate_resolutions_raise_up_front(monkeypatch):
    from splatam_amd import dist as sdist
    from splatam_amd import pipeline
    full, tracking, densify = LM.datasets(GOLD, "phone", device="cuda")
    monkeypatch.setattr(sdist, "world_size", lambda: 2)
    monkeypatch.setattr(sdist, "get_rank", lambda: 0)
    before = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match="multi-rank"):
        pipeline.rgbd_slam(full, LT.load_config(GOLD, "phone"), engine="fused", tracking_dataset=tracking, densify_dataset=densify)
    assert torch.cuda.memory_allocated() == before                  # before any work
