"""Evaluation of a finished run on the device (csrc/evalmetrics.hip, FusedEngine.evaluate_frame / evaluate_metrics,
splatam_amd/evaluation.py): the metric kernels against the float64 restatement (tests/eval_ref.py), the render + metrics call
against the metrics of the returned planes and against the torch mirror, the workspace handed back clean, no host read per frame,
and the hook in ``pipeline.rgbd_slam``."""
import os

import numpy as np
import pytest
import torch

from tests import eval_ref

pytestmark = pytest.mark.gpu

SIL_THRES = 0.5


def _kernel_metrics(planes, sil_mask, ms_ssim=True):
    """(row [8], totals [SPLAT_EVAL_SUMS]) of evaluate_metrics on CPU planes."""
    from splatam_amd import fused
    rgb, depth, sil, gt_im, gt_depth = (t.cuda() for t in planes)
    row = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    sums = fused.evaluate_metrics(rgb, depth, sil, {'im': gt_im, 'depth': gt_depth}, row, SIL_THRES, sil_mask=sil_mask, ms_ssim=ms_ssim)
    torch.cuda.synchronize()
    assert float(sums[:-1].abs().max()) == 0.0          # the copies are handed back zeroed
    return row.cpu().numpy(), sums[-1].cpu().numpy()


@pytest.mark.parametrize("sil_mask", [False, True])
@pytest.mark.parametrize("W,H", [(320, 240), (233, 177), (1200, 680), (1752, 1168)])
def test_metric_kernels_match_the_float64_restatement(W, H, sil_mask):
    """Tolerances come from the reference's own rounding: the same restatement evaluated in float32 on the CPU gives
    d32 = |f32 - f64| per level mean and for the final number; the kernels must stay within 4 d32 + 16 float32 ulps of the value
    (margin 4: summation order, FMA contraction; floor: two torch builds can agree by accident).  PSNR / depth: rtol 1e-6 (double
    accumulation of float32 terms).  Every figure is printed before it is asserted (profiles/eval_metrics.md records them)."""
    from splatam_amd import _capi
    planes = eval_ref.seeded_planes(W, H, seed=100 + W + int(sil_mask))
    r64 = eval_ref.frame_metrics(*planes, SIL_THRES, sil_mask, dtype=torch.float64)
    r32 = eval_ref.frame_metrics(*planes, SIL_THRES, sil_mask, dtype=torch.float32)
    row, tot = _kernel_metrics(planes, sil_mask)
    ws, hs = eval_ref.level_sizes(W), eval_ref.level_sizes(H)
    worst = 0.0
    for level in range(5):
        n = (ws[level] - 10) * (hs[level] - 10)
        for ch in range(3):
            for k, name in ((0, "cs"), (1, "ss")):
                got = tot[8 + 6 * level + 2 * ch + k] / n
                want, f32 = float(r64[name][level, ch]), float(r32[name][level, ch])
                bound = 4 * abs(f32 - want) + eval_ref.f32_ulps(want)
                worst = max(worst, abs(got - want) / bound)
                print(f"EVALDIFF {W}x{H} sil_mask={int(sil_mask)} level={level} ch={ch} {name}: f64={want:.9f} |kernel-f64|={abs(got - want):.3e} "
                      f"|f32-f64|={abs(f32 - want):.3e} bound={bound:.3e}")
                assert abs(got - want) <= bound, (level, ch, name, got, want, f32)
    want, f32 = float(r64['ms_ssim']), float(r32['ms_ssim'])
    bound = 4 * abs(f32 - want) + eval_ref.f32_ulps(want)
    print(f"EVALDIFF {W}x{H} sil_mask={int(sil_mask)} ms_ssim: f64={want:.9f} |kernel-f64|={abs(row[3] - want):.3e} |f32-f64|={abs(f32 - want):.3e} "
          f"bound={bound:.3e} worst level ratio={worst:.3f}")
    assert abs(row[_capi.SPLAT_EVAL_MS_SSIM] - want) <= bound
    print(f"EVALDIFF {W}x{H} sil_mask={int(sil_mask)} psnr: f64={float(r64['psnr']):.9f} rel={abs(row[0] / float(r64['psnr']) - 1):.3e} "
          f"depth_l1: f64={float(r64['depth_l1']):.9f} rel={abs(row[2] / float(r64['depth_l1']) - 1):.3e}")
    np.testing.assert_allclose(row[_capi.SPLAT_EVAL_PSNR], float(r64['psnr']), rtol=1e-6)
    np.testing.assert_allclose(row[_capi.SPLAT_EVAL_DEPTH_L1], float(r64['depth_l1']), rtol=1e-6)
    assert row[_capi.SPLAT_EVAL_DEPTH_RMSE] == row[_capi.SPLAT_EVAL_DEPTH_L1]         # the reference's per-pixel root: the same number
    assert row[_capi.SPLAT_EVAL_VALID] == r64['valid'] and row[_capi.SPLAT_EVAL_FLAGGED] == 0


def test_metrics_without_ms_ssim_take_any_frame_size_and_ms_ssim_refuses_small_frames():
    from splatam_amd import _capi, fused
    planes = eval_ref.seeded_planes(160, 112, seed=7)
    r64 = eval_ref.frame_metrics(*planes, SIL_THRES, True, with_ms_ssim=False)
    row, _ = _kernel_metrics(planes, True, ms_ssim=False)
    np.testing.assert_allclose(row[0], float(r64['psnr']), rtol=1e-6)
    np.testing.assert_allclose(row[2], float(r64['depth_l1']), rtol=1e-6)
    assert np.isnan(row[_capi.SPLAT_EVAL_MS_SSIM]) and row[4] == r64['valid']
    rgb, depth, sil, gt_im, gt_depth = (t.cuda() for t in planes)
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="160"):
        fused.evaluate_metrics(rgb, depth, sil, {'im': gt_im, 'depth': gt_depth}, out, SIL_THRES, ms_ssim=True)


def test_nan_and_empty_masks_propagate_as_in_torch():
    """No special cases: a NaN in a rendered plane and a frame without valid depth give what the torch expressions give."""
    planes = list(eval_ref.seeded_planes(233, 177, seed=9))
    planes[0] = planes[0].clone()
    planes[0][1, 50, 60] = float("nan")
    row, _ = _kernel_metrics(planes, False)
    r64 = eval_ref.frame_metrics(*planes, SIL_THRES, False)
    assert np.isnan(row[0]) and np.isnan(float(r64['psnr'])) and np.isnan(row[3]) and np.isnan(float(r64['ms_ssim']))
    np.testing.assert_allclose(row[2], float(r64['depth_l1']), rtol=1e-6)
    planes = list(eval_ref.seeded_planes(233, 177, seed=9))
    planes[4] = torch.zeros_like(planes[4])
    row, _ = _kernel_metrics(planes, False)
    r64 = eval_ref.frame_metrics(*planes, SIL_THRES, False)
    assert row[4] == 0 and np.isnan(row[2]) and np.isnan(float(r64['depth_l1']))          # 0 / 0
    assert np.isinf(row[0]) and np.isinf(float(r64['psnr']))                              # all pixels masked: mse 0


# ---------------------------------------------------------------------------------------------------------------------------------
# render + metrics in one call
# ---------------------------------------------------------------------------------------------------------------------------------
def _scene(W=320, H=240, n=20000, seed=3):
    from tests.test_gpu_fused import _scene as fused_scene
    return fused_scene(n, W, H, seed=seed)


def _ref64(planes, gt, sil_mask):
    im, depth, sil = planes
    return eval_ref.frame_metrics(im.cpu(), depth.cpu(), sil.cpu(), gt['im'].cpu(), gt['depth'].cpu(), SIL_THRES, sil_mask)


@pytest.mark.parametrize("sil_mask", [False, True])
def test_evaluate_frame_equals_metrics_of_its_planes_and_the_mirror(sil_mask):
    """(a) evaluate_frame = evaluate_metrics on the planes ``render`` returns, to the rounding of <= 1e6 double additions in another
    order (rtol 1e-10).  (b) Against the mirror -- ``slam.eval_frame_metrics`` on the drop-in rasterizer's two renders B -- through
    the float64 restatement r on both sets of planes:  |kernel(A) - mirror(B)| <= |kernel(A) - r(A)| + |r(A) - r(B)| + |r(B) - mirror(B)|,
    the outer terms bounded as everywhere (kernel: 1e-6 relative for PSNR / L1, 4 |f32 - f64| + 16 ulps for MS-SSIM; mirror: float32
    torch, 1e-5 relative), the middle one MEASURED from the planes; for L1 without the silhouette it is itself at most mean |depth
    difference| over the valid pixels."""
    from splatam_amd import fused, slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene()
    eng = FusedEngine(params, cam)
    eng.relearn_lists(frame, 1)
    row = torch.zeros(8, dtype=torch.float64, device="cuda")
    eng.evaluate_frame(frame, 1, row, SIL_THRES, sil_mask=sil_mask)
    im, depth, sil, _ = (t.clone() for t in eng.rendered())
    row2 = torch.zeros(8, dtype=torch.float64, device="cuda")
    fused.evaluate_metrics(im, depth, sil, frame, row2, SIL_THRES, sil_mask=sil_mask)
    torch.cuda.synchronize()
    a, b = row.cpu().numpy(), row2.cpu().numpy()
    assert a[5] == 0 and a[4] == b[4] == float((frame['depth'] > 0).sum())
    np.testing.assert_allclose(a[:4], b[:4], rtol=1e-10)
    # (b)
    with torch.no_grad():
        p = {k: v.detach() for k, v in params.items()}
        tg = slam.transform_to_frame(p, 1, gaussians_grad=False, camera_grad=False)
        ds, _, _ = slam.Renderer(raster_settings=cam)(**slam.transformed_params2depthplussilhouette(p, frame['w2c'], tg))
        im_b, _, _ = slam.Renderer(raster_settings=cam)(**slam.transformed_params2rendervar(p, tg))
        m = slam.eval_frame_metrics(im_b, ds, frame, SIL_THRES, sil_mask)
    rA, rB = _ref64((im, depth, sil), frame, sil_mask), _ref64((im_b, ds[0:1], ds[1]), frame, sil_mask)
    rA32 = eval_ref.frame_metrics(im.cpu(), depth.cpu(), sil.cpu(), frame['im'].cpu(), frame['depth'].cpu(), SIL_THRES, sil_mask, dtype=torch.float32)
    for name, k, got in (("psnr", 0, float(m['psnr'])), ("depth_l1", 2, float(m['depth_l1']))):
        planes_term = abs(float(rA[name]) - float(rB[name]))
        bound = 1e-6 * abs(float(rA[name])) + planes_term + 1e-5 * abs(float(rB[name]))
        print(f"EVALMIRROR sil_mask={int(sil_mask)} {name}: kernel={a[k]:.9f} mirror={got:.9f} |diff|={abs(a[k] - got):.3e} planes term={planes_term:.3e} bound={bound:.3e}")
        assert abs(a[k] - got) <= bound, name
    kernel_term = 4 * abs(float(rA32['ms_ssim']) - float(rA['ms_ssim'])) + eval_ref.f32_ulps(float(rA['ms_ssim']))
    planes_term = abs(float(rA['ms_ssim']) - float(rB['ms_ssim']))
    bound = kernel_term + planes_term + 1e-5 * float(rB['ms_ssim'])
    print(f"EVALMIRROR sil_mask={int(sil_mask)} ms_ssim: kernel={a[3]:.9f} mirror={float(m['ms_ssim']):.9f} |diff|={abs(a[3] - float(m['ms_ssim'])):.3e} "
          f"planes term={planes_term:.3e} bound={bound:.3e}")
    assert abs(a[3] - float(m['ms_ssim'])) <= bound
    if not sil_mask:
        valid = frame['depth'] > 0
        mean_dd = float(((depth - ds[0:1]).abs() * valid).double().sum() / valid.sum())
        assert abs(float(rA['depth_l1']) - float(rB['depth_l1'])) <= mean_dd + 1e-12


def test_evaluation_hands_the_workspace_back_clean():
    """After evaluate_frame: the same view renders bit-identical planes; add_new_gaussians appends as many rows as on a fresh
    engine; a tracking and a mapping iteration give loss and gradients within the run-to-run spread of the float atomics (measured
    by running the un-evaluated engine twice; 2 x that spread, + one float32 ulp of the largest entry for a spread that happens to
    be zero); the evaluation's own sums are zero."""
    from splatam_amd import fused, slam
    from splatam_amd.fused import FusedEngine
    params, variables, frame, cam = _scene(seed=5)
    row = torch.zeros(8, dtype=torch.float64, device="cuda")

    def iteration(eng, tracking):
        eng.loss_backward(frame, 1, slam.REPLICA_TRACKING if tracking else slam.REPLICA_MAPPING, tracking=tracking)
        torch.cuda.synchronize()
        out = {'d_cam': eng.buf['d_cam'][:8].clone()}
        if not tracking:
            out.update({k: v.clone() for k, v in eng.grads.items()})
        return out

    plain, evald = FusedEngine(params, cam), FusedEngine(params, cam)
    for eng in (plain, evald):
        eng.relearn_lists(frame, 1)
    before = [t.clone() for t in evald.render(frame, 1)]
    evald.evaluate_frame(frame, 1, row, SIL_THRES, sil_mask=True)
    after = evald.render(frame, 1)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert float(fused.eval_workspace(evald.dev, evald.W, evald.H, True)[1][:-1].abs().max()) == 0.0
    for tracking in (True, False):
        r1, r2 = iteration(plain, tracking), iteration(plain, tracking)
        evald.evaluate_frame(frame, 1, row, SIL_THRES, sil_mask=False)
        r3 = iteration(evald, tracking)
        assert not plain.check_overflow(grow=False) and not evald.check_overflow(grow=False)
        for k in r1:
            spread = float((r1[k] - r2[k]).abs().max())
            ulp = float(np.spacing(np.float32(float(r1[k].abs().max()))))
            diff = min(float((r3[k] - r1[k]).abs().max()), float((r3[k] - r2[k]).abs().max()))      # (to the nearer of the two plain runs)
            print(f"EVALCLEAN tracking={int(tracking)} {k}: spread={spread:.3e} diff after evaluation={diff:.3e}")
            assert diff <= 2 * spread + ulp, (tracking, k, diff, spread)
    # map growth: an engine that owns its map, evaluated or not, appends the same rows
    counts = []
    W, H = evald.W, evald.H
    grow = dict(frame, intrinsics=torch.tensor([[0.5 * W, 0, W / 2 - 0.5], [0, 0.5 * W, H / 2 - 0.5], [0, 0, 1]], device="cuda"))
    for evaluate_first in (False, True):
        p = {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}
        v = {k: t.clone() for k, t in variables.items()}
        eng = FusedEngine(p, cam, gaussian_capacity=p['means3D'].shape[0] + 200000, variables=v)
        eng.relearn_lists(frame, 1)
        if evaluate_first:
            eng.evaluate_frame(frame, 1, row, SIL_THRES, sil_mask=True)
        counts.append((eng.add_new_gaussians(grow, 0.5, 1, "projective", "isotropic"), eng.P))
    assert counts[0] == counts[1] and counts[0][0] > 0, counts


def test_evaluate_reads_the_device_once():
    """Between learning the list statistics and the table read nothing may synchronise: the enqueue phase of ``evaluate`` runs under
    torch's sync debug mode "error" (it sees .item(), .tolist(), .cpu(), blocking copies -- how every host read of fused.py is made)."""
    from splatam_amd import evaluation
    from splatam_amd.fused import FusedEngine
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
            enforced = False
        except RuntimeError:
            enforced = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') is not enforced by this torch build")
    dataset, params = eval_ref.golden_case("cuda")                # 12 frames of 240 x 176, rendered once, resident on the device
    orig_relearn, orig_read = FusedEngine.relearn_lists, evaluation._read_table
    phases = []

    def relearn(self, *a, **k):
        out = orig_relearn(self, *a, **k)
        phases.append("learnt")
        torch.cuda.set_sync_debug_mode("error")
        return out

    def read(table):
        torch.cuda.set_sync_debug_mode("default")
        phases.append("read")
        return orig_read(table)
    FusedEngine.relearn_lists, evaluation._read_table = relearn, read
    try:
        got = evaluation.evaluate(dataset, params, len(dataset), SIL_THRES, 60, True, eval_every=1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        FusedEngine.relearn_lists, evaluation._read_table = orig_relearn, orig_read
    assert phases == ["learnt", "read"] and got['repeated'] == []
    assert got['frames'] == list(range(12)) and np.isfinite(got['psnr']).all() and np.isfinite(got['ms_ssim']).all()
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_reference.npz"))
    np.testing.assert_allclose(got['ate_rmse'], float(gold["valid/every1/ate"]), rtol=1e-5)      # poses only: independent of the renderer
    # the frames were rendered by the HIP rasterizer here and by the oracle in the recording: the same scene to ~1e-4 per pixel
    np.testing.assert_allclose(got['psnr'], gold["valid/every1/psnr"], atol=0.05)
    np.testing.assert_allclose(got['depth_l1'], gold["valid/every1/l1"], rtol=2e-2)


def test_rows_rendered_on_truncated_lists_are_evaluated_again():
    """A view whose lists outgrow the learnt buckets raises the row's flag (slot 5); ``evaluate`` re-learns the lists on that view and
    evaluates it again.  Forced here: after the statistics have been learnt the buckets are shrunk to 16 entries per tile."""
    from splatam_amd import evaluation
    from splatam_amd.fused import FusedEngine
    dataset, params = eval_ref.golden_case("cuda")
    want = evaluation.evaluate(dataset, params, len(dataset), SIL_THRES, 0, False, eval_every=5)
    assert want['repeated'] == [] and want['sil_mask']
    orig = FusedEngine.relearn_lists
    calls = []

    def relearn(self, *a, **k):
        orig(self, *a, **k)
        calls.append(self.tile_stride)
        if len(calls) == 1:
            self.tile_stride = 16
    FusedEngine.relearn_lists = relearn
    try:
        got = evaluation.evaluate(dataset, params, len(dataset), SIL_THRES, 0, False, eval_every=5)
    finally:
        FusedEngine.relearn_lists = orig
    assert got['frames'] == [0, 4, 9] and got['repeated'] == [0, 4, 9], (got['repeated'], calls)
    for k in ('psnr', 'depth_l1', 'ms_ssim'):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-10)
    np.testing.assert_allclose(got['ate_rmse'], want['ate_rmse'], rtol=1e-12)


@pytest.fixture(scope="module")
def slam_runs():
    from splatam_amd import pipeline
    W, H, f = 240, 176, 210.0
    out = {}
    for engine in ("fused", "dropin"):
        ds = pipeline.SyntheticRGBDSequence(14000, W, H, f, f, W / 2 - 0.5, H / 2 - 0.5, num_frames=4, seed=2, step_m=0.012, step_deg=0.4).preload()
        cfg = pipeline.replica_config(tracking_iters=12, mapping_iters=24, keyframe_every=2)
        torch.manual_seed(0)
        np.random.seed(0)
        params, variables, stats = pipeline.rgbd_slam(ds, cfg, engine=engine, evaluate=dict(eval_every=1))
        torch.cuda.synchronize()
        out[engine] = (ds, cfg, params, stats)
    return out


@pytest.mark.parametrize("engine", ["fused", "dropin"])
def test_rgbd_slam_evaluates_its_final_map(slam_runs, engine):
    from splatam_amd import evaluation, pipeline, slam
    ds, cfg, params, stats = slam_runs[engine]
    ev = stats['eval']
    assert ev['frames'] == [0, 1, 2, 3] and ev['lpips'] is None and not ev['sil_mask']
    by_hand = evaluation.evaluate(ds, params, len(ds), cfg['mapping']['sil_thres'], cfg['mapping']['num_iters'], cfg['mapping']['add_new_gaussians'])
    for k in ('psnr', 'depth_l1', 'depth_rmse', 'ms_ssim'):
        print(f"EVALSLAM {engine} {k}: {np.round(ev[k], 6).tolist()} max rel diff by hand {np.abs(ev[k] / by_hand[k] - 1).max():.2e}")
        np.testing.assert_allclose(ev[k], by_hand[k], rtol=1e-10)
    first = torch.linalg.inv(ds[0][3])
    est = [first] + [pipeline._est_w2c(params, t) for t in range(1, len(ds))]
    gt = [torch.linalg.inv(ds[t][3]) for t in range(len(ds))]
    np.testing.assert_allclose(ev['ate_rmse'], slam.evaluate_ate(gt, est), rtol=1e-6)
    assert ev['ate_rmse'] < 0.02 and ev['avg_psnr'] > 20 and 0.5 < ev['avg_ms_ssim'] <= 1.0


def test_fused_and_dropin_runs_score_alike_and_evaluation_is_opt_in(slam_runs):
    """The two loops' maps and poses agree within the loop tests' tolerances (poses 2e-3, row counts 2e-3: tests/test_gpu_pipeline.py),
    which moves a 25-35 dB PSNR by a fraction of a dB: 1 dB (12 % in RMS error) is a sanity bound on top of those tests."""
    from splatam_amd import pipeline
    ef, ed = slam_runs["fused"][3]['eval'], slam_runs["dropin"][3]['eval']
    print(f"EVALSLAM psnr fused {np.round(ef['psnr'], 3).tolist()} dropin {np.round(ed['psnr'], 3).tolist()}")
    assert np.abs(ef['psnr'] - ed['psnr']).max() < 1.0
    ds, cfg = slam_runs["fused"][0], slam_runs["fused"][1]
    torch.manual_seed(0)
    np.random.seed(0)
    _, _, stats = pipeline.rgbd_slam(ds, cfg, engine="fused", num_frames=2)
    assert 'eval' not in stats
    with pytest.raises(ValueError):
        pipeline.rgbd_slam(ds, cfg, engine="fused", num_frames=1, evaluate=dict(every=2))
