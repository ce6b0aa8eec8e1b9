"""Scoring held-out views on the device: the hole count of the first-level metric kernel (csrc/evalmetrics.hip, SplatEvalConfig.holes),
``FusedEngine.evaluate_view`` at a pose, ``evaluation.evaluate_novel_views`` against the recording of the reference's ``eval_nvs``
(tests/golden/nvs_reference.npz) and against the torch mirror, its host synchronisation, and a ScanNet++ tree from disk through the
frame loop and ``python -m splatam_amd.eval_novel_view``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import eval_ref, nvs_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "nvs_reference.npz"))
SIL_THRES = nvs_ref.SIL_THRES


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,ms_ssim", [(37, 29, False), (66, 50, False), (240, 176, True)])
def test_hole_count_of_the_metric_kernel(W, H, ms_ssim):
    """37 x 29 and 66 x 50: odd, no multiples of 4 or of the 32 x 24 tile, one and several workgroups; 240 x 176 with the pyramid.  The
    count equals torch's integer count on the same float32 planes (NaN and threshold-equal silhouettes among them), whatever
    sil_mask; the other slots are bit-equal to the call without the count, which leaves slot 6 at 0; a second call gives the same
    row: the sums were handed back zeroed."""
    from splatam_amd import _capi, fused
    rgb, depth, sil, gt_im, gt_depth = eval_ref.seeded_planes(W, H, seed=300 + W)
    sil = sil.clone()
    sil[H // 3, : W // 2] = float("nan")
    sil[H // 3 + 1, : W // 2] = SIL_THRES
    want = int((~((sil > SIL_THRES) | ~(gt_depth[0] > 0))).sum())
    assert want > int((~((torch.nan_to_num(sil, nan=1.0) > SIL_THRES) | ~(gt_depth[0] > 0))).sum()) > 0      # the NaN row adds holes
    planes = [t.cuda() for t in (rgb, depth, sil)]
    frame = {'im': gt_im.cuda(), 'depth': gt_depth.cuda()}

    def call(sil_mask, holes):
        row = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
        sums = fused.evaluate_metrics(*planes, frame, row, SIL_THRES, sil_mask=sil_mask, ms_ssim=ms_ssim, holes=holes)
        torch.cuda.synchronize()
        assert float(sums[:-1].abs().max()) == 0.0
        return row.cpu().numpy(), sums[-1].cpu().numpy()
    for sil_mask in (False, True):
        with_count, tot = call(sil_mask, True)
        without, tot0 = call(sil_mask, False)
        again, _ = call(sil_mask, True)
        print(f"NVSHOLES {W}x{H} sil_mask={int(sil_mask)}: kernel {with_count[_capi.SPLAT_EVAL_HOLES]:.0f} torch {want}")
        assert with_count[_capi.SPLAT_EVAL_HOLES] == want and tot[5] == want
        assert without[_capi.SPLAT_EVAL_HOLES] == 0 and tot0[5] == 0 and without[7] == with_count[7] == 0
        others = [k for k in range(8) if k != _capi.SPLAT_EVAL_HOLES]
        assert with_count[others].tobytes() == without[others].tobytes()
        assert np.delete(tot, 5).tobytes() == np.delete(tot0, 5).tobytes()
        assert again.tobytes() == with_count.tobytes()
    with pytest.raises(RuntimeError):
        fused.evaluate_metrics(planes[0], planes[1], None, frame, torch.zeros(8, dtype=torch.float64, device="cuda"), SIL_THRES, ms_ssim=False, holes=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# a view at a pose
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine_and_frame(name, k):
    """(engine around the case's map with a camera at the first frame, its frame-0 data, data of held-out frame k, its effective w2c)."""
    from splatam_amd import evaluation, slam
    from splatam_amd.fused import FusedEngine
    dataset, params, variant, every = nvs_ref.case(name, "cuda")
    color0, depth0, intrinsics, pose0 = evaluation._frame(dataset, 0)
    first = torch.linalg.inv(pose0).contiguous()
    cam = slam.setup_camera(color0.shape[2], color0.shape[1], intrinsics.cpu().numpy(), first.cpu().numpy())
    eng = FusedEngine({n: v.detach().float().contiguous() for n, v in params.items()}, cam)
    color, depth, _, pose = evaluation._frame(dataset, k + 1)
    w2c = (first @ torch.linalg.inv(pose)).contiguous()
    data0 = {'cam': cam, 'im': color0, 'depth': depth0, 'id': 0, 'intrinsics': intrinsics.cpu(), 'w2c': first}
    data = {'cam': cam, 'im': color, 'depth': depth, 'id': k + 1, 'intrinsics': intrinsics.cpu(), 'w2c': first}
    return eng, data0, data, w2c, params


def test_evaluate_view_is_render_view_and_evaluate_metrics_and_touches_nothing_else():
    from splatam_amd import _capi, fused
    from splatam_amd.fused import PARAM_ORDER
    eng, data0, data, w2c, _ = _engine_and_frame("aniso/sil/every1", 2)
    eng.relearn_lists(data0, 0)
    eng.render(data0, 0)
    main = eng._camera

    def snapshot():
        s = {f"param {n}": eng.params[n].detach().clone() for n in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        s.update({f"exp_avg {n}": eng.exp_avg[n].clone() for n in PARAM_ORDER})
        s.update({f"exp_avg_sq {n}": eng.exp_avg_sq[n].clone() for n in PARAM_ORDER})
        s.update({f"rendered {i}": t.clone() for i, t in enumerate(eng.rendered())})
        return s
    before = snapshot()
    view = eng.view_camera(240, 176)
    eng.relearn_lists(data, 0, view=view, w2c=w2c)
    row = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    img = eng.evaluate_view(view, w2c, data, row, SIL_THRES, sil_mask=True)
    planes = img.out6.clone()
    row_b = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    eng.evaluate_view(view, w2c, data, row_b, SIL_THRES, sil_mask=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    assert eng._camera is main
    after = snapshot()
    for name in before:
        assert torch.equal(before[name], after[name]), name
    # the same kernels by hand
    by_hand = eng.render_view(view, w2c=w2c, intrinsics=data['intrinsics'], rgb8=False)
    assert by_hand.rgb8 is None and torch.equal(by_hand.out6, planes)
    row2 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    fused.evaluate_metrics(by_hand.out6[0:3], by_hand.out6[3], by_hand.out6[4], data, row2, SIL_THRES, sil_mask=True, holes=True)
    torch.cuda.synchronize()
    a, b, c = row.cpu().numpy(), row2.cpu().numpy(), row_b.cpu().numpy()
    np.testing.assert_allclose(a[:4], b[:4], rtol=1e-10)
    np.testing.assert_allclose(c[:4], b[:4], rtol=1e-10)
    assert a[4] == b[4] == float((data['depth'] > 0).sum()) and a[_capi.SPLAT_EVAL_FLAGGED] == 0 and int(by_hand.truncated) == 0
    want = int((~((planes[4] > SIL_THRES) | ~(data['depth'][0] > 0))).sum())
    assert a[_capi.SPLAT_EVAL_HOLES] == b[_capi.SPLAT_EVAL_HOLES] == c[_capi.SPLAT_EVAL_HOLES] == want > 500       # an "open" view
    # holes=False: slot 6 stays 0, the rest is the same row
    row3 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    eng.evaluate_view(view, w2c, data, row3, SIL_THRES, sil_mask=True, holes=False)
    d = row3.cpu().numpy()
    assert d[_capi.SPLAT_EVAL_HOLES] == 0
    np.testing.assert_allclose(d[:5], a[:5], rtol=1e-10)
    with pytest.raises(RuntimeError, match="176"):
        eng.evaluate_view(view, w2c, dict(data, im=data['im'][:, :100]), row3, SIL_THRES)


# ---------------------------------------------------------------------------------------------------------------------------------
# the driver against the recording and against the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_runs():
    from splatam_amd import evaluation
    out = {}
    for name in nvs_ref.CASES:
        dataset, params, (mapping_iters, add_new), every = nvs_ref.case(name, "cuda")
        out[name] = evaluation.evaluate_novel_views(dataset, params, len(dataset), SIL_THRES, mapping_iters, add_new, eval_every=every)
    return out


@pytest.mark.parametrize("name", list(nvs_ref.CASES))
def test_device_path_follows_the_reference_eval_nvs(device_runs, name):
    """Frames rendered by the HIP rasterizer here and by the oracle in the recording: psnr atol 0.05 and depth L1 rtol 2e-2, the bounds
    tests/test_gpu_eval.py uses for this scene; hole counts within each frame's recorded ``undecided`` pixels; equal verdicts."""
    got = device_runs[name]
    assert got['frames'] == GOLD[f"{name}/frames"].tolist() and got['repeated'] == [] and got['lpips'] is None
    for i, k in enumerate(got['frames']):
        print(f"NVSGOLD {name} k={k}: psnr {got['psnr'][i]:.4f} / {GOLD[f'{name}/psnr'][i]:.4f}  l1 {got['depth_l1'][i]:.6f} / {GOLD[f'{name}/l1'][i]:.6f}  "
              f"holes {got['holes'][i]} / {GOLD[f'{name}/holes'][i]} (undecided {GOLD[f'{name}/undecided'][i]})  valid {got['valid_nvs_frames'][i]}")
    np.testing.assert_allclose(got['psnr'], GOLD[f"{name}/psnr"], atol=0.05)
    np.testing.assert_allclose(got['depth_l1'], GOLD[f"{name}/l1"], rtol=2e-2)
    np.testing.assert_allclose(got['depth_rmse'], got['depth_l1'], rtol=1e-12)
    assert (np.abs(got['holes'] - GOLD[f"{name}/holes"]) <= GOLD[f"{name}/undecided"]).all()
    assert got['valid_nvs_frames'].tolist() == GOLD[f"{name}/valid"].tolist()
    valid = GOLD[f"{name}/valid"]
    for key in ('psnr', 'depth_l1', 'depth_rmse', 'ms_ssim'):
        np.testing.assert_allclose(got['avg_' + key], got[key][valid].mean(), rtol=1e-12)
    assert np.isfinite(got['ms_ssim']).all()


@pytest.mark.parametrize("name,k", [("iso/valid/every1", 0), ("aniso/sil/every1", 2), ("general/valid/every3", 5)])
def test_device_row_against_the_mirror_on_the_dropin_rasterizer(name, k):
    """The bounds of test_evaluate_frame_equals_metrics_of_its_planes_and_the_mirror (tests/test_gpu_eval.py): through the float64
    restatement r on both sets of planes, |kernel(A) - mirror(B)| <= |kernel(A) - r(A)| + |r(A) - r(B)| + |r(B) - mirror(B)| with the
    outer terms bounded as everywhere (1e-6 / 1e-5 relative; MS-SSIM 4 |f32 - f64| + 16 ulps) and the middle one measured."""
    from splatam_amd import evaluation
    eng, _, data, w2c, params = _engine_and_frame(name, k)
    sil_mask = evaluation.uses_silhouette_mask(*nvs_ref.CASES[name][1])
    view = eng.view_camera(240, 176)
    eng.relearn_lists(data, 0, view=view, w2c=w2c)
    row = torch.zeros(8, dtype=torch.float64, device="cuda")
    A = eng.evaluate_view(view, w2c, data, row, SIL_THRES, sil_mask=sil_mask).out6.clone()
    dataset = nvs_ref.case(name, "cuda")[0]
    mrow, B = evaluation._mirror_nvs_row(params, data, torch.linalg.inv(dataset[k + 1][3]), SIL_THRES, sil_mask, True)
    a, m = row.cpu().numpy(), mrow.numpy()

    def ref(p, dtype=torch.float64):
        return eval_ref.frame_metrics(p[0:3].cpu(), p[3].cpu(), p[4].cpu(), data['im'].cpu(), data['depth'].cpu(), SIL_THRES, sil_mask, dtype=dtype)
    rA, rB, rA32 = ref(A), ref(B), ref(A, torch.float32)
    for key, slot in (("psnr", 0), ("depth_l1", 2)):
        planes_term = abs(float(rA[key]) - float(rB[key]))
        bound = 1e-6 * abs(float(rA[key])) + planes_term + 1e-5 * abs(float(rB[key]))
        print(f"NVSMIRROR {name} k={k} {key}: kernel={a[slot]:.9f} mirror={m[slot]:.9f} |diff|={abs(a[slot] - m[slot]):.3e} planes term={planes_term:.3e} bound={bound:.3e}")
        assert abs(a[slot] - m[slot]) <= bound, key
    kernel_term = 4 * abs(float(rA32['ms_ssim']) - float(rA['ms_ssim'])) + eval_ref.f32_ulps(float(rA['ms_ssim']))
    planes_term = abs(float(rA['ms_ssim']) - float(rB['ms_ssim']))
    assert abs(a[3] - m[3]) <= kernel_term + planes_term + 1e-5 * float(rB['ms_ssim'])
    # the two hole counts differ by no more pixels than the two silhouettes decide differently
    flips = int((((A[4] > SIL_THRES) != (B[4] > SIL_THRES)) & (data['depth'][0] > 0)).sum())
    print(f"NVSMIRROR {name} k={k} holes: kernel={a[6]:.0f} mirror={m[6]:.0f} pixels decided differently={flips}")
    assert abs(a[6] - m[6]) <= flips and a[4] == m[4]


# ---------------------------------------------------------------------------------------------------------------------------------
# host synchronisation
# ---------------------------------------------------------------------------------------------------------------------------------
def test_novel_views_read_the_device_once():
    """The method of tests/test_gpu_eval.py::test_evaluate_reads_the_device_once: from the end of ``relearn_lists`` to the table read
    torch's sync debug mode is "error"."""
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
    dataset, params, (mapping_iters, add_new), every = nvs_ref.case("iso/valid/every1", "cuda")
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
        got = evaluation.evaluate_novel_views(dataset, params, len(dataset), SIL_THRES, mapping_iters, add_new, eval_every=every)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        FusedEngine.relearn_lists, evaluation._read_table = orig_relearn, orig_read
    assert phases == ["learnt", "read"] and got['repeated'] == []
    assert got['frames'] == list(range(12)) and got['valid_nvs_frames'].tolist() == GOLD["iso/valid/every1/valid"].tolist()


def test_views_rendered_on_truncated_lists_are_evaluated_again():
    """After the view's statistics have been learnt its buckets are shrunk to 16 entries per tile: every row comes back flagged, is
    evaluated again on lists re-learnt for its own pose, and appears in ``repeated``."""
    from splatam_amd import evaluation
    from splatam_amd.fused import FusedEngine
    dataset, params, (mapping_iters, add_new), every = nvs_ref.case("iso/sil/every3", "cuda")
    want = evaluation.evaluate_novel_views(dataset, params, len(dataset), SIL_THRES, mapping_iters, add_new, eval_every=every)
    assert want['repeated'] == [] and want['sil_mask']
    orig = FusedEngine.relearn_lists
    calls = []

    def relearn(self, *a, view=None, **k):
        orig(self, *a, view=view, **k)
        calls.append(view.camera.tile_stride)
        if len(calls) == 1:
            view.camera.tile_stride = 16
    FusedEngine.relearn_lists = relearn
    try:
        got = evaluation.evaluate_novel_views(dataset, params, len(dataset), SIL_THRES, mapping_iters, add_new, eval_every=every)
    finally:
        FusedEngine.relearn_lists = orig
    assert got['frames'] == [0, 2, 5, 8, 11] and got['repeated'] == [0, 2, 5, 8, 11], (got['repeated'], calls)
    for key in ('psnr', 'depth_l1', 'ms_ssim'):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-10)
    assert got['holes'].tolist() == want['holes'].tolist() and got['valid_nvs_frames'].tolist() == want['valid_nvs_frames'].tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# from disk: run on the train split, score the held-out one from the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_scannetpp_tree_through_the_loop_and_the_command_line(tmp_path):
    import novel_view_files as nv
    from splatam_amd import pipeline, run
    W, H, F = 240, 176, 200.0
    n_train, n_test = 8, 5
    ds = pipeline.SyntheticRGBDSequence(14000, W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, num_frames=n_train + n_test, seed=5, step_m=0.012, step_deg=0.4)
    items = []
    for t in range(n_train + n_test):
        color, depth, _, pose = ds[t]
        rgb = np.rint(color.cpu().numpy()).clip(0, 255).astype(np.uint8)
        raw = np.rint(depth.cpu().numpy()[..., 0].astype(np.float64) * 1000.0)
        assert raw.max() <= 65535
        items.append((f"DSC{t:05d}.JPG", rgb, raw.astype(np.uint16), pose.cpu().numpy().astype(np.float64), False))
    # train: the even frames of the first stretch in time order; held out: frames between and beyond them
    train = [items[t] for t in (0, 2, 3, 5, 6, 8, 9, 11)]
    test = [items[t] for t in (1, 4, 7, 10, 12)]
    root = str(tmp_path / "data")
    nv.write_scannetpp(root, "8b5caf3398", train, test, dict(w=W, h=H, fl_x=F, fl_y=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5))
    cfg = pipeline.replica_config(tracking_iters=10, mapping_iters=15, keyframe_every=2)
    cfg.update(workdir=str(tmp_path / "experiments"), run_name="8b5caf3398_0", seed=0, primary_device="cuda:0", eval_every=1,
               report_global_progress_every=500, report_iter_progress=False, load_checkpoint=False, save_checkpoints=False, use_wandb=False,
               data=dict(dataset_name="scannetpp", basedir=root, sequence="8b5caf3398", ignore_bad=False, use_train_split=True,
                         desired_image_height=H, desired_image_width=W, start=0, end=-1, stride=1, num_frames=-1))
    torch.manual_seed(0)
    np.random.seed(0)
    _, _, stats, params_path = run.run(dict(cfg, data=dict(cfg['data'])), engine="fused", evaluate=False)
    torch.cuda.synchronize()
    assert stats['frames'] == n_train and os.path.isfile(params_path)
    nvs_cfg = dict(cfg, scene_path=params_path, data=dict(cfg['data'], use_train_split=False))
    path = str(tmp_path / "eval_novel_view.py")
    with open(path, "w") as f:
        f.write("# written by tests/test_gpu_novel_view.py\nconfig = " + repr(nvs_cfg) + "\n")
    done = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "-m", "splatam_amd.eval_novel_view", path], cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    print(done.stdout)
    assert done.returncode == 0
    for line in ("Average PSNR:", "Average Depth RMSE:", "Average Depth L1:", "Average MS-SSIM:", "Average LPIPS: not computed"):
        assert line in done.stdout
    eval_dir = os.path.join(cfg['workdir'], "8b5caf3398_0", "eval_nvs")
    for name in ("psnr.txt", "rmse.txt", "l1.txt", "ssim.txt"):
        rows = np.loadtxt(os.path.join(eval_dir, name))
        assert rows.shape == (n_test,) and np.isfinite(rows).all(), name
    flags = np.load(os.path.join(eval_dir, "valid_nvs_frames.npy"))
    assert flags.shape == (n_test,) and flags.dtype == bool
    psnr = np.loadtxt(os.path.join(eval_dir, "psnr.txt"))
    assert psnr.min() > 15                                           # a map of this scene seen from between its training poses, not noise
    from PIL import Image
    for folder, prefix in (("rendered_rgb", "splatam"), ("rendered_depth", "splatam"), ("rgb", "gt"), ("depth", "gt")):
        assert sorted(os.listdir(os.path.join(eval_dir, folder))) == [f"{prefix}_{k:04d}.png" for k in range(n_test)]
        with Image.open(os.path.join(eval_dir, folder, f"{prefix}_0003.png")) as im:
            assert im.size == (W, H) and im.mode == "RGB"
    # the ground-truth picture of held-out frame 1 is the file the loader read (8-bit colour survives the round trip)
    with Image.open(os.path.join(eval_dir, "rgb", "gt_0001.png")) as im:
        assert np.abs(np.asarray(im).astype(np.int32) - test[1][1].astype(np.int32)).max() <= 1
    # wandb is refused with run.py's message
    with open(path, "w") as f:
        f.write("config = " + repr(dict(nvs_cfg, use_wandb=True)) + "\n")
    from splatam_amd import eval_novel_view
    with pytest.raises(SystemExit, match="use_wandb"):
        eval_novel_view.main([path])
