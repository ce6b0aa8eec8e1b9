"""Evaluation of a finished run, the parts that need no GPU: the kernels' arithmetic (csrc/eval_math.h compiled for the host)
against the float64 torch restatement (tests/eval_ref.py), the torch mirror (``slam.eval_frame_metrics`` / ``ms_ssim`` /
``evaluate_ate``, ``evaluation.evaluate(engine="mirror")``) against a recording of the reference's own ``eval``
(tests/golden/eval_reference.npz, made by tests/golden/make_golden_eval.py on the C oracle), and the C ABI of the evaluation."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import eval_ref
from tests.util import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "eval_reference.npz"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. eval_math.h on the host
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    L = host_shim("eval_math_shim", "eval_math.h")
    L.em_pyramid_floats.restype = C.c_size_t
    return L


def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def test_window_weights(shim):
    g = np.zeros(11, np.float32)
    shim.em_window(_p(g))
    c = torch.arange(11, dtype=torch.float64) - 5
    want = torch.exp(-c ** 2 / (2 * 1.5 ** 2))
    want = (want / want.sum()).numpy()
    np.testing.assert_allclose(g, want, rtol=6e-8, atol=0)          # the float64 weights, rounded once
    assert abs(float(g.astype(np.float64).sum()) - 1.0) < 2e-7


def test_ssim_and_cs_pixel(shim):
    g = torch.Generator().manual_seed(0)
    n = 4096
    x, y = torch.rand(n, 11, 11, generator=g, dtype=torch.float64), torch.rand(n, 11, 11, generator=g, dtype=torch.float64)
    y = 0.7 * x + 0.3 * y
    w = torch.rand(11, 11, generator=g, dtype=torch.float64)
    w = w / w.sum()
    E = lambda t: (t * w).sum((1, 2))                               # noqa: E731
    mu1, mu2, e11, e22, e12 = E(x), E(y), E(x * x), E(y * y), E(x * y)
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    cs = (2 * s12 + 0.03 ** 2) / (s1 + s2 + 0.03 ** 2)
    ss = (2 * mu1 * mu2 + 0.01 ** 2) / (mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * cs
    a = [t.numpy().astype(np.float32) for t in (mu1, mu2, e11, e22, e12)]
    got_ss, got_cs = np.zeros(n, np.float32), np.zeros(n, np.float32)
    shim.em_ssim_pixel(n, *[_p(t) for t in a], _p(got_ss), _p(got_cs))
    # float32 inputs of a cancelling sigma^2 (|e - mu^2| ~ 0.05 of operands ~ 0.3): a few 1e-6
    np.testing.assert_allclose(got_cs, cs.numpy(), atol=2e-5)
    np.testing.assert_allclose(got_ss, ss.numpy(), atol=2e-5)


@pytest.mark.parametrize("n", [680, 1200, 85, 43, 233, 177, 161, 11])
def test_pooling_index_rule_at_even_and_odd_sizes(shim, n):
    """avg_pool2d(2, padding = n % 2, count_include_pad): size and source indices against torch itself on an index ramp."""
    x = torch.arange(1, n + 1, dtype=torch.float64).view(1, 1, 1, n)            # (1-based: the zero pad is recognisable)
    want = torch.nn.functional.avg_pool2d(x.expand(1, 1, 2, n), 2, padding=[0, n % 2])[0, 0, 0]
    assert shim.em_pool_size(n) == want.numel() == eval_ref.level_sizes(n)[1]
    for p in range(want.numel()):
        first = shim.em_pool_first(p, n)
        assert -1 <= first and first + 1 <= n - 1
        taps = [(first + k + 1) if first + k >= 0 else 0 for k in (0, 1)]        # values of the ramp, 0 for the pad
        assert 2 * sum(taps) / 4 == float(want[p]), (n, p)
    for level in range(5):
        assert shim.em_level_size(n, level) == eval_ref.level_sizes(n)[level]


def test_finish_arithmetic(shim):
    """relu, level weights, product over levels, mean over channels, PSNR over all pixels, the depth quotient -- in double."""
    W, H = 233, 177
    rng = np.random.default_rng(3)
    tot = np.zeros(40)
    tot[0:3] = rng.uniform(50, 80, 3)
    tot[3], tot[4] = 321.5, 30000
    ws, hs = eval_ref.level_sizes(W), eval_ref.level_sizes(H)
    means = rng.uniform(0.9, 1.0, (5, 3, 2))
    means[1, 2, 0] = -0.01                                           # a negative cs mean: clamped to 0 -> the channel's product is 0
    for lv in range(5):
        for ch in range(3):
            tot[8 + 6 * lv + 2 * ch: 8 + 6 * lv + 2 * ch + 2] = means[lv, ch] * (ws[lv] - 10) * (hs[lv] - 10)
            assert shim.em_level_slot(lv, ch) == 8 + 6 * lv + 2 * ch
    row = np.full(8, -1.0)
    shim.em_finish(_p(tot, C.c_double), W, H, 1, _p(row, C.c_double))
    vals = torch.tensor(np.concatenate([means[:4, :, 0], means[4:, :, 1]]))
    w = torch.tensor(eval_ref.WEIGHTS, dtype=torch.float64).view(-1, 1)
    want_ms = float(torch.prod(torch.relu(vals) ** w, 0).mean())
    want_psnr = float((20 * torch.log10(1.0 / torch.sqrt(torch.tensor(tot[0:3]) / (W * H)))).mean())
    np.testing.assert_allclose(row[:5], [want_psnr, 321.5 / 30000, 321.5 / 30000, want_ms, 30000], rtol=1e-14)
    shim.em_finish(_p(tot, C.c_double), W, H, 0, _p(row, C.c_double))
    assert np.isnan(row[3]) and row[0] == pytest.approx(want_psnr, rel=1e-14)
    tot[4] = 0.0
    tot[3] = 0.0
    shim.em_finish(_p(tot, C.c_double), W, H, 1, _p(row, C.c_double))
    assert np.isnan(row[1]) and np.isnan(row[2])                     # 0 / 0, as torch


@pytest.mark.parametrize("W,H,sil_mask", [(233, 177, True), (320, 240, False)])
def test_host_model_of_a_frame_matches_the_restatement(shim, W, H, sil_mask):
    """The whole frame by plain loops over eval_math.h (window, weighting, ssim pixel, pooling rule, finish) against the float64
    restatement, within the bound the GPU test uses: 4 |f32 - f64| + 16 float32 ulps per level mean and for the result."""
    planes = eval_ref.seeded_planes(W, H, seed=21)
    r64 = eval_ref.frame_metrics(*planes, 0.5, sil_mask)
    r32 = eval_ref.frame_metrics(*planes, 0.5, sil_mask, dtype=torch.float32)
    a = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in planes]
    tot, row = np.zeros(40), np.zeros(8)
    shim.em_frame(W, H, *[_p(t) for t in a], C.c_float(0.5), int(sil_mask), _p(tot, C.c_double), _p(row, C.c_double))
    ws, hs = eval_ref.level_sizes(W), eval_ref.level_sizes(H)
    for lv in range(5):
        for ch in range(3):
            for k, name in ((0, 'cs'), (1, 'ss')):
                got = tot[8 + 6 * lv + 2 * ch + k] / ((ws[lv] - 10) * (hs[lv] - 10))
                want, f32 = float(r64[name][lv, ch]), float(r32[name][lv, ch])
                assert abs(got - want) <= 4 * abs(f32 - want) + eval_ref.f32_ulps(want), (lv, ch, name)
    want, f32 = float(r64['ms_ssim']), float(r32['ms_ssim'])
    assert abs(row[3] - want) <= 4 * abs(f32 - want) + eval_ref.f32_ulps(want)
    np.testing.assert_allclose(row[0], float(r64['psnr']), rtol=1e-6)
    np.testing.assert_allclose(row[2], float(r64['depth_l1']), rtol=1e-6)
    assert row[1] == row[2] and row[4] == r64['valid']
    assert shim.em_pyramid_floats(W, H) == 6 * sum(w * h for w, h in zip(ws[1:], hs[1:]))


def test_per_pixel_weighting_and_depth_term(shim):
    rgb, depth, sil, gt_im, gt_depth = eval_ref.seeded_planes(233, 177, seed=4)
    n = 233 * 177
    for sil_mask in (False, True):
        out = [np.zeros(n, np.float32) for _ in range(4)]
        shim.em_pixel(n, _p(rgb[1].numpy().ravel()), _p(gt_im[1].numpy().ravel()), _p(depth.numpy().ravel()), _p(gt_depth.numpy().ravel()),
                      _p(sil.numpy().ravel()), C.c_float(0.5), int(sil_mask), *[_p(o) for o in out])
        v = (gt_depth[0] > 0).float()
        p = (sil > 0.5).float() if sil_mask else torch.ones_like(sil)
        assert np.array_equal(out[0], (rgb[1] * p * v).numpy().ravel()) and np.array_equal(out[1], (gt_im[1] * p * v).numpy().ravel())
        assert np.array_equal(out[2], ((((depth[0] * v) - gt_depth[0]) * p).abs() * v).numpy().ravel())
        assert np.array_equal(out[3], v.numpy().ravel())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the torch mirror against the recording of the reference's eval
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_run():
    """``evaluation.evaluate(engine="mirror")`` with the C oracle behind ``slam.Renderer`` on the regenerated golden case."""
    from oracle import c_ref
    from splatam_amd import evaluation, slam
    saved = slam.Renderer
    slam.Renderer = c_ref.CRasterizer
    try:
        dataset, params = eval_ref.golden_case("cpu")
        out = {}
        for vname, (mapping_iters, add_new) in eval_ref.GOLDEN_VARIANTS.items():
            for every in eval_ref.GOLDEN_EVERY:
                out[f"{vname}/every{every}"] = evaluation.evaluate(dataset, params, len(dataset), eval_ref.GOLDEN_SIL_THRES, mapping_iters, add_new,
                                                                   eval_every=every, engine="mirror")
    finally:
        slam.Renderer = saved
    return dataset, params, out


@pytest.mark.parametrize("vname", list(eval_ref.GOLDEN_VARIANTS))
@pytest.mark.parametrize("every", eval_ref.GOLDEN_EVERY)
def test_evaluate_follows_the_reference_eval(golden_run, vname, every):
    """Frame selection, mask variant, PSNR / depth numbers and the trajectory error with its NaN-pose skipping: the same torch
    operations on the same inputs as the reference's, hence float32 rounding (rtol 1e-5)."""
    _, _, runs = golden_run
    key = f"{vname}/every{every}"
    got = runs[key]
    assert got['frames'] == GOLD[f"{key}/frames"].tolist()
    assert got['frames'] == ([0, 4, 9] if every == 5 else list(range(12)))
    assert got['sil_mask'] == (vname == "sil") and got['lpips'] is None and got['repeated'] == []
    np.testing.assert_allclose(got['psnr'], GOLD[f"{key}/psnr"], rtol=1e-5)
    np.testing.assert_allclose(got['depth_l1'], GOLD[f"{key}/l1"], rtol=1e-5)
    np.testing.assert_allclose(got['depth_rmse'], GOLD[f"{key}/rmse"], rtol=1e-5)
    np.testing.assert_allclose(got['ate_rmse'], float(GOLD[f"{key}/ate"]), rtol=1e-5)
    np.testing.assert_allclose(got['ms_ssim'], GOLD[f"{key}/ssim_restated_not_upstream"], rtol=1e-5)       # (two restatements: pins no upstream)
    np.testing.assert_allclose(got['avg_psnr'], GOLD[f"{key}/psnr"].mean(), rtol=1e-5)
    # the NaN ground-truth pose was skipped on both sides: 11 of 12 poses entered the alignment
    assert GOLD[f"{key}/ate_gt_w2c"].shape[0] == GOLD[f"{key}/ate_est_w2c"].shape[0] == 11


def test_the_two_mask_variants_differ_and_rmse_is_l1(golden_run):
    _, _, runs = golden_run
    a, b = runs["valid/every1"], runs["sil/every1"]
    assert np.abs(a['psnr'] - b['psnr']).max() > 0.1 and np.abs(a['depth_l1'] - b['depth_l1']).max() > 1e-4
    for r in (a, b):
        np.testing.assert_allclose(r['depth_rmse'], r['depth_l1'], rtol=1e-6)     # the reference's per-pixel root (kept, documented)


def test_evaluate_ate_and_align_against_the_reference():
    from splatam_amd import slam
    for key in ("valid/every1", "sil/every5"):
        gt, est = torch.tensor(GOLD[f"{key}/ate_gt_w2c"]), torch.tensor(GOLD[f"{key}/ate_est_w2c"])
        np.testing.assert_allclose(slam.evaluate_ate(list(gt), list(est)), float(GOLD[f"{key}/ate"]), rtol=1e-5)
    for i in range(3):
        rot, trans, err = slam.align_trajectories(GOLD[f"align/{i}/model"], GOLD[f"align/{i}/data"])
        np.testing.assert_allclose(rot, GOLD[f"align/{i}/rot"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(trans, GOLD[f"align/{i}/trans"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(err, GOLD[f"align/{i}/trans_error"], rtol=1e-7, atol=1e-12)


def test_evaluate_writes_the_reference_text_files(golden_run, tmp_path):
    from oracle import c_ref
    from splatam_amd import evaluation, slam
    dataset, params, _ = golden_run
    saved = slam.Renderer
    slam.Renderer = c_ref.CRasterizer
    try:
        got = evaluation.evaluate(dataset, params, len(dataset), 0.5, 60, True, eval_every=5, engine="mirror", eval_dir=str(tmp_path), ms_ssim=False)
    finally:
        slam.Renderer = saved
    assert sorted(os.listdir(tmp_path)) == ["l1.txt", "psnr.txt", "rmse.txt", "ssim.txt"]
    np.testing.assert_allclose(np.loadtxt(tmp_path / "psnr.txt"), got['psnr'])
    assert np.isnan(got['ms_ssim']).all() and np.isnan(got['avg_ms_ssim'])
    assert evaluation.eval_frame_indices(12, 5) == [0, 4, 9] and evaluation.eval_frame_indices(3, 1) == [0, 1, 2]
    assert evaluation.uses_silhouette_mask(0, False) and not evaluation.uses_silhouette_mask(0, True) and not evaluation.uses_silhouette_mask(1, False)
    with pytest.raises(ValueError):
        evaluation.evaluate(dataset, params, 12, 0.5, 60, True, engine="torch")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. slam.ms_ssim against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(320, 240), (233, 177)])
def test_mirror_ms_ssim_matches_the_restatement(W, H):
    from splatam_amd import slam
    rgb, depth, sil, gt_im, gt_depth = eval_ref.seeded_planes(W, H, seed=31)
    v = (gt_depth > 0).float()
    for X, Y in ((rgb, gt_im), (rgb * v, gt_im * v)):                # plain, and with a fully masked region (the invalid rectangle)
        want = float(eval_ref.ms_ssim_levels(X[None].double(), Y[None].double())[2])
        assert abs(float(slam.ms_ssim(X[None].double(), Y[None].double())) - want) < 1e-14
        f32 = float(eval_ref.ms_ssim_levels(X[None], Y[None])[2])
        assert abs(float(slam.ms_ssim(X[None], Y[None])) - want) <= 4 * abs(f32 - want) + eval_ref.f32_ulps(want)
    assert 0.9 < want < 1.0


def test_mirror_ms_ssim_refuses_small_frames():
    from splatam_amd import slam
    x = torch.rand(1, 3, 160, 300)
    with pytest.raises(ValueError, match="160"):
        slam.ms_ssim(x, x)
    slam.ms_ssim(torch.rand(1, 3, 161, 161), torch.rand(1, 3, 161, 161))


def test_mirror_frame_metrics_match_the_restatement():
    from splatam_amd import slam
    rgb, depth, sil, gt_im, gt_depth = eval_ref.seeded_planes(233, 177, seed=8)
    for sil_mask in (False, True):
        m = slam.eval_frame_metrics(rgb, torch.cat([depth, sil[None]]), {'im': gt_im, 'depth': gt_depth}, 0.5, sil_mask)
        r = eval_ref.frame_metrics(rgb, depth, sil, gt_im, gt_depth, 0.5, sil_mask)
        np.testing.assert_allclose(float(m['psnr']), float(r['psnr']), rtol=1e-5)
        np.testing.assert_allclose(float(m['depth_l1']), float(r['depth_l1']), rtol=1e-5)
        np.testing.assert_allclose(float(m['depth_rmse']), float(m['depth_l1']), rtol=1e-6)
        assert int(m['valid']) == r['valid'] and abs(float(m['ms_ssim']) - float(r['ms_ssim'])) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the C ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1200, 680), (233, 177)])
def test_eval_workspace_layout(W, H):
    from splatam_amd import _capi
    lay = _capi.eval_workspace_layout(W, H, True)
    assert lay.names == ["pyramid", "sums"]
    ws, hs = eval_ref.level_sizes(W), eval_ref.level_sizes(H)
    if (W, H) == (1200, 680):
        assert list(zip(ws, hs)) == [(1200, 680), (600, 340), (300, 170), (150, 85), (75, 43)]
    assert lay.bytes["pyramid"] == 4 * 6 * sum(w * h for w, h in zip(ws[1:], hs[1:]))
    assert lay.bytes["sums"] == 8 * (_capi.SPLAT_ITER_SUM_COPIES + 1) * _capi.SPLAT_EVAL_SUMS
    assert lay.zero_init == {"pyramid": False, "sums": True}
    assert lay.offset["pyramid"] == 0 and lay.offset["sums"] % _capi.SPLAT_SLAB_ALIGN == 0 and lay.offset["sums"] >= lay.bytes["pyramid"]
    assert lay.total % _capi.SPLAT_SLAB_ALIGN == 0 and lay.total >= lay.offset["sums"] + lay.bytes["sums"]
    no = _capi.eval_workspace_layout(W, H, False)
    assert no.names == ["sums"] and no.bytes["sums"] == lay.bytes["sums"]
    # bind: the pointers land at the offsets
    ews = _capi.SplatEvalWorkspace()
    slab = 1 << 20
    assert _capi.lib().splat_eval_workspace_bind(C.byref(ews), slab, lay.arrays, lay.n) == 0
    assert ews.pyramid == slab + lay.offset["pyramid"] and ews.sums == slab + lay.offset["sums"]
    assert _capi.lib().splat_eval_workspace_bind(C.byref(ews), slab + 8, lay.arrays, lay.n) == 1


def test_eval_structs_constants_and_refusals():
    import re
    from splatam_amd import _capi, fused
    from tests.test_capi_cpu import HEADER, _struct_fields
    L = _capi.lib()
    for name in ("SplatEvalConfig", "SplatEvalWorkspace"):
        assert [f[0] for f in getattr(_capi, name)._fields_] == _struct_fields(name)
        assert L.splat_sizeof(name.encode()) == C.sizeof(getattr(_capi, name)) > 0
        assert getattr(_capi, name) in _capi.MIRRORED_STRUCTS
    for k in ("SPLAT_EVAL_ROW", "SPLAT_EVAL_LEVELS", "SPLAT_EVAL_SUMS", "SPLAT_EVAL_LAYOUT_MS_SSIM", "SPLAT_EVAL_PSNR", "SPLAT_EVAL_DEPTH_RMSE",
              "SPLAT_EVAL_DEPTH_L1", "SPLAT_EVAL_MS_SSIM", "SPLAT_EVAL_VALID", "SPLAT_EVAL_FLAGGED"):
        assert getattr(_capi, k) == int(re.search(rf"#define {k} (\d+)", HEADER).group(1))
    assert L.splat_abi_version() >= 12
    # a frame MS-SSIM cannot take is refused before anything is launched: layout, the metrics call, the Python surface
    total = C.c_size_t(0)
    assert L.splat_eval_workspace_layout(160, 112, 1, None, 0, C.byref(total)) == -1
    assert L.splat_eval_workspace_layout(300, 160, 1, None, 0, C.byref(total)) == -1
    assert L.splat_eval_workspace_layout(160, 112, 0, None, 0, C.byref(total)) == 1
    assert L.splat_eval_workspace_layout(0, 112, 0, None, 0, C.byref(total)) == -1
    cfg, ews = _capi.SplatEvalConfig(), _capi.SplatEvalWorkspace()
    cfg.sil_thres, cfg.sil_mask, cfg.ms_ssim = 0.5, 1, 1
    ews.pyramid, ews.sums = 4096, 8192                              # (never dereferenced: the call is refused)
    args = (4096, 4096, 4096, 4096, 4096)
    assert L.splat_eval_metrics(160, 112, *args, C.byref(cfg), C.byref(ews), 4096, None) == 1
    assert L.splat_eval_metrics(300, 200, None, *args[1:], C.byref(cfg), C.byref(ews), 4096, None) == 1
    assert L.splat_eval_metrics(300, 200, *args, C.byref(cfg), C.byref(ews), None, None) == 1
    ews.pyramid = None
    assert L.splat_eval_metrics(300, 200, *args, C.byref(cfg), C.byref(ews), 4096, None) == 1
    assert L.splat_iter_eval(None, None, None, C.byref(cfg), None, C.byref(ews), 4096, None) == 1
    with pytest.raises(RuntimeError, match="160"):
        _capi.eval_workspace_layout(160, 112, True)
    # CPU tensors raise: the library has no CPU path
    planes = eval_ref.seeded_planes(233, 177, seed=1)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        fused.evaluate_metrics(planes[0], planes[1], planes[2], {'im': planes[3], 'depth': planes[4]}, torch.zeros(8, dtype=torch.float64), 0.5)
