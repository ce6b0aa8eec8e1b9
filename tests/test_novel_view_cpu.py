"""Scoring held-out views, the parts that need no GPU: the hole rule of csrc/eval_math.h compiled for the host, and
``evaluation.evaluate_novel_views(engine="mirror")`` on the C oracle against a recording of the reference's own ``eval_nvs``
(tests/golden/nvs_reference.npz, made by tests/golden/make_golden_nvs.py on the scene of tests/nvs_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import eval_ref, nvs_ref
from tests.util import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "nvs_reference.npz"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the hole rule on the host
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    L = host_shim("eval_holes_shim", "eval_math.h")
    L.eh_count.restype = C.c_longlong
    L.eh_valid.argtypes = [C.c_longlong, C.c_int, C.c_int]
    return L


def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def _count(shim, gt_depth, sil, thres):
    gt_depth, sil = np.ascontiguousarray(gt_depth, np.float32).ravel(), np.ascontiguousarray(sil, np.float32).ravel()
    flags = np.zeros(gt_depth.size, np.uint8)
    n = shim.eh_count(gt_depth.size, _p(gt_depth), _p(sil), C.c_float(thres), _p(flags, C.c_ubyte))
    return n, flags.astype(bool)


def test_hole_rule_is_the_torch_expression_on_seeded_planes(shim):
    """``(~(silhouette > sil_thres | ~(depth > 0))).sum()`` of eval_nvs, on planes with silhouettes EQUAL to the threshold (not
    present: a hole), NaN silhouettes (compare false: a hole), zero and negative depth (no valid depth: never a hole)."""
    from splatam_amd import _capi
    _, _, sil, _, gt_depth = eval_ref.seeded_planes(233, 177, seed=12)
    sil, gt_depth = sil.clone(), gt_depth[0].clone()
    sil[10:14, 20:40] = 0.5                           # equal to the threshold, over valid and invalid depth
    sil[30:33, 50:90] = float("nan")
    gt_depth[60:64, 100:140] = -1.0                   # negative depth with silhouettes on both sides of the threshold
    sil[60:62, 100:140] = 0.1
    gt_depth[12, 20:30] = 0.0
    want = ~((sil > 0.5) | ~(gt_depth > 0))
    n, flags = _count(shim, gt_depth.numpy(), sil.numpy(), 0.5)
    assert n == int(want.sum()) and np.array_equal(flags, want.numpy().ravel())
    assert flags.reshape(177, 233)[10:14, 20:40].sum() == int((gt_depth[10:14, 20:40] > 0).sum()) > 0         # equal: holes where depth is valid
    assert flags.reshape(177, 233)[30:33, 50:90].sum() == int((gt_depth[30:33, 50:90] > 0).sum()) > 0         # NaN: holes where depth is valid
    assert not flags.reshape(177, 233)[60:64, 100:140].any() and not flags.reshape(177, 233)[12, 20:30].any()
    # a threshold that float32 does not hold exactly is compared as float32, as torch compares a float32 plane with a Python number
    thres = 0.99
    sil2 = torch.full((4, 8), float(np.float32(thres)))
    sil2[1] = float(np.nextafter(np.float32(thres), np.float32(2)))
    sil2[2] = float(np.nextafter(np.float32(thres), np.float32(0)))
    depth2 = torch.ones(4, 8)
    n, flags = _count(shim, depth2.numpy(), sil2.numpy(), thres)
    assert np.array_equal(flags, (~((sil2 > thres) | ~(depth2 > 0))).numpy().ravel()) and n == 24
    assert shim.eh_sum_slot() == 5 and _capi.SPLAT_EVAL_HOLES == 6 and _capi.SPLAT_EVAL_SUMS == 40


def test_validity_rule_is_float32_as_torch_evaluates_it(shim):
    """``holes / (H W) * 100 > 0.1`` with an integer tensor: torch divides in float32.  Every count around the limit of three frame
    sizes, against torch itself and against ``evaluation.percent_holes``."""
    from splatam_amd import evaluation
    for W, H in ((240, 176), (876, 584), (1752, 1168), (1000, 1000), (16, 12)):
        limit = W * H // 1000
        for holes in list(range(max(limit - 40, 0), limit + 40)) + [0, W * H]:
            invalid = bool(torch.tensor(holes) / (H * W) * 100 > 0.1)
            assert bool(shim.eh_valid(holes, W, H)) == (not invalid), (W, H, holes)
            assert bool(evaluation.percent_holes([holes], H, W)[0] > np.float32(0.1)) == invalid
    assert evaluation.percent_holes([3], 12, 16).dtype == np.float32
    # exactly 0.1 % (1000 holes of 1000 x 1000) is NOT above the limit: the product rounds to float32(0.1) and is compared with it as float32
    assert not bool(torch.tensor(1000) / (1000 * 1000) * 100 > 0.1) and shim.eh_valid(1000, 1000, 1000) and not shim.eh_valid(1001, 1000, 1000)


def test_abi_17_config_carries_the_switch():
    import re
    from splatam_amd import _capi
    from tests.test_capi_cpu import HEADER, _struct_fields
    assert _capi.ABI_VERSION == 17 == _capi.lib().splat_abi_version()
    assert _struct_fields("SplatEvalConfig")[-1] == "holes" == _capi.SplatEvalConfig._fields_[-1][0]
    assert _capi.lib().splat_sizeof(b"SplatEvalConfig") == C.sizeof(_capi.SplatEvalConfig) == 16
    assert _capi.SPLAT_EVAL_HOLES == int(re.search(r"#define SPLAT_EVAL_HOLES (\d+)", HEADER).group(1))
    # holes without a silhouette is refused before anything is launched
    cfg, ews = _capi.SplatEvalConfig(), _capi.SplatEvalWorkspace()
    cfg.sil_thres, cfg.sil_mask, cfg.ms_ssim, cfg.holes = 0.5, 0, 0, 1
    ews.pyramid, ews.sums = None, 8192                               # (never dereferenced: the call is refused)
    L = _capi.lib()
    assert L.splat_eval_metrics(300, 200, 4096, 4096, None, 4096, 4096, C.byref(cfg), C.byref(ews), 4096, None) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the torch mirror against the recording of the reference's eval_nvs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_runs():
    """``evaluation.evaluate_novel_views(engine="mirror")`` with the C oracle behind ``slam.Renderer`` on the regenerated cases."""
    from oracle import c_ref
    from splatam_amd import evaluation, slam
    saved = slam.Renderer
    slam.Renderer = c_ref.CRasterizer
    try:
        out = {}
        for name in nvs_ref.CASES:
            dataset, params, (mapping_iters, add_new), every = nvs_ref.case(name, "cpu")
            out[name] = evaluation.evaluate_novel_views(dataset, params, len(dataset), nvs_ref.SIL_THRES, mapping_iters, add_new, eval_every=every,
                                                        engine="mirror")
    finally:
        slam.Renderer = saved
    return out


@pytest.mark.parametrize("name", list(nvs_ref.CASES))
def test_mirror_follows_the_reference_eval_nvs(golden_runs, name):
    """Scored indices, hole counts and verdicts equal; PSNR / depth numbers within float32 rounding of the same torch operations on
    the same inputs (rtol 1e-5, the bound of tests/test_eval_cpu.py); the averages over the VALID frames only."""
    got = golden_runs[name]
    kind, variant, every, general = nvs_ref.CASES[name]
    assert got['frames'] == GOLD[f"{name}/frames"].tolist() == ([0, 2, 5, 8, 11] if every == 3 else list(range(12)))
    assert got['holes'].tolist() == GOLD[f"{name}/holes"].tolist() and got['holes'].dtype == np.int64
    assert got['valid_nvs_frames'].tolist() == GOLD[f"{name}/valid"].tolist() and got['valid_nvs_frames'].dtype == bool
    assert got['sil_mask'] == (variant == eval_ref.GOLDEN_VARIANTS["sil"]) and got['lpips'] is None and got['repeated'] == [] and 'ate_rmse' not in got
    np.testing.assert_allclose(got['psnr'], GOLD[f"{name}/psnr"], rtol=1e-5)
    np.testing.assert_allclose(got['depth_l1'], GOLD[f"{name}/l1"], rtol=1e-5)
    np.testing.assert_allclose(got['depth_rmse'], GOLD[f"{name}/rmse"], rtol=1e-5)
    np.testing.assert_allclose(got['ms_ssim'], GOLD[f"{name}/ssim_restated_not_upstream"], rtol=1e-5)       # (two restatements: pins no upstream)
    valid = GOLD[f"{name}/valid"]
    assert 2 <= valid.sum() <= len(valid) - 2
    for k, g in (('psnr', 'psnr'), ('depth_l1', 'l1'), ('depth_rmse', 'rmse'), ('ms_ssim', 'ssim_restated_not_upstream')):
        np.testing.assert_allclose(got['avg_' + k], GOLD[f"{name}/{g}"][valid].mean(), rtol=1e-5)
        assert abs(got['avg_' + k] - GOLD[f"{name}/{g}"].mean()) > 1e-4 * abs(got['avg_' + k])       # not the mean over all frames
    np.testing.assert_array_equal(got['percent_holes'], (torch.tensor(GOLD[f"{name}/holes"]) / (176 * 240) * 100).numpy())
    np.testing.assert_allclose(got['depth_rmse'], got['depth_l1'], rtol=1e-6)                          # the reference's per-pixel root, kept


def test_general_first_pose_gives_the_frames_of_the_identity_case(golden_runs):
    """``first_frame_w2c @ inv(pose_t)``: with a general first matrix either factor alone is another view (PSNR far off); the product
    is the same view up to float32 rounding of the matrices."""
    a, b = golden_runs["general/valid/every3"], golden_runs["iso/valid/every1"]
    rows = [b['frames'].index(k) for k in a['frames']]
    np.testing.assert_allclose(a['psnr'], b['psnr'][rows], atol=0.02)
    assert a['holes'].tolist() == b['holes'][rows].tolist()


def test_files_and_picture_names(tmp_path, monkeypatch):
    from oracle import c_ref
    from splatam_amd import evaluation, slam
    saved_pictures, directories = [], evaluation._FrameSaver.NAMES

    class Saver:
        def __init__(self, eval_dir, dev, H, W, rendered_prefix="gs"):
            self.names = [(d, rendered_prefix if d.startswith("rendered_") else p) for d, p in directories]
            assert (H, W) == (176, 240)

        def save(self, t, out6, im, depth):
            assert out6.shape[0] >= 5 and tuple(out6.shape[1:]) == (176, 240) and tuple(im.shape) == (3, 176, 240) and tuple(depth.shape) == (1, 176, 240)
            saved_pictures.extend(os.path.join(d, f"{p}_{t:04d}.png") for d, p in self.names)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False
    monkeypatch.setattr(evaluation, "_FrameSaver", Saver)
    monkeypatch.setattr(slam, "Renderer", c_ref.CRasterizer)
    name = "iso/sil/every3"
    dataset, params, (mapping_iters, add_new), every = nvs_ref.case(name, "cpu")
    got = evaluation.evaluate_novel_views(dataset, params, len(dataset), nvs_ref.SIL_THRES, mapping_iters, add_new, eval_every=every, engine="mirror",
                                          eval_dir=str(tmp_path), ms_ssim=False, save_frames=True)
    assert sorted(os.listdir(tmp_path)) == ["l1.txt", "psnr.txt", "rmse.txt", "ssim.txt", "valid_nvs_frames.npy"]
    np.testing.assert_allclose(np.loadtxt(tmp_path / "psnr.txt"), got['psnr'])
    np.testing.assert_allclose(np.loadtxt(tmp_path / "l1.txt"), got['depth_l1'])
    np.testing.assert_allclose(np.loadtxt(tmp_path / "rmse.txt"), got['depth_rmse'])
    flags = np.load(tmp_path / "valid_nvs_frames.npy")
    assert flags.dtype == bool and flags.tolist() == GOLD[f"{name}/valid"].tolist()
    assert np.isnan(got['ms_ssim']).all() and np.isnan(got['avg_ms_ssim']) and np.isnan(np.loadtxt(tmp_path / "ssim.txt")).all()
    assert sorted(saved_pictures) == sorted(os.path.join(d, f"{p}_{k:04d}.png") for k in (0, 2, 5, 8, 11)
                                            for d, p in (("rendered_rgb", "splatam"), ("rendered_depth", "splatam"), ("rgb", "gt"), ("depth", "gt")))
    assert evaluation.novel_view_indices(13, 3) == [0, 2, 5, 8, 11] and evaluation.novel_view_indices(2, 5) == [0] and evaluation.novel_view_indices(1, 1) == []


def test_no_valid_frame_gives_nan_averages_and_refusals(monkeypatch):
    from oracle import c_ref
    from splatam_amd import evaluation, slam
    monkeypatch.setattr(slam, "Renderer", c_ref.CRasterizer)
    dataset, params, _, _ = nvs_ref.case("iso/valid/every1", "cpu")
    # items 0, 3, 4: the first training frame and two "open" views
    sub = nvs_ref.HeldOutSplit.__new__(nvs_ref.HeldOutSplit)
    sub.items = [dataset[0], dataset[3], dataset[4]]
    got = evaluation.evaluate_novel_views(sub, params, 3, nvs_ref.SIL_THRES, 60, True, engine="mirror", ms_ssim=False)
    assert got['frames'] == [0, 1] and not got['valid_nvs_frames'].any() and np.isfinite(got['psnr']).all()
    assert all(np.isnan(got['avg_' + k]) for k in ('psnr', 'depth_rmse', 'depth_l1', 'ms_ssim'))
    with pytest.raises(ValueError, match="mirror"):
        evaluation.evaluate_novel_views(sub, params, 3, 0.5, 60, True, engine="torch")
    with pytest.raises(ValueError, match="eval_dir"):
        evaluation.evaluate_novel_views(sub, params, 3, 0.5, 60, True, engine="mirror", save_frames=True)
    with pytest.raises(ValueError, match="HIP device"):
        evaluation.evaluate_novel_views(sub, params, 3, 0.5, 60, True, engine="mirror", save_frames=True, eval_dir="unused", ms_ssim=False)


def test_matrix_to_quaternion_picks_the_well_conditioned_branch():
    """Every branch (largest of |w|, |x|, |y|, |z|), against scipy; and the composition eval_nvs applies to an anisotropic map:
    R(quat_mult(q(R_cam), q)) = R_cam R(q)."""
    from scipy.spatial.transform import Rotation
    from splatam_amd import slam
    rng = np.random.default_rng(5)
    rotvecs = [rng.normal(size=3) * 0.05, np.array([np.pi - 0.01, 0, 0]), np.array([0, np.pi - 0.02, 0.01]), np.array([0.01, 0, np.pi - 0.01])]
    rotvecs += [rng.normal(size=3) for _ in range(20)]
    branches = set()
    for rv in rotvecs:
        R = Rotation.from_rotvec(rv).as_matrix()
        q = slam.matrix_to_quaternion(torch.tensor(R, dtype=torch.float32)).double().numpy()
        x, y, z, w = Rotation.from_matrix(R).as_quat()
        want = np.array([w, x, y, z])
        branches.add(int(np.argmax(np.abs(want))))
        assert min(np.abs(q - want).max(), np.abs(q + want).max()) < 2e-6, (rv, q, want)
        g = torch.Generator().manual_seed(1)
        qs = torch.nn.functional.normalize(torch.randn(16, 4, generator=g))
        qc = torch.nn.functional.normalize(torch.tensor(q, dtype=torch.float32)[None])
        np.testing.assert_allclose(slam.build_rotation(slam.quat_mult(qc, qs)).numpy(), (torch.tensor(R, dtype=torch.float32) @ slam.build_rotation(qs)).numpy(), atol=3e-6)
    assert branches == {0, 1, 2, 3}
