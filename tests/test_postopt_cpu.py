"""The refinement of a finished map (splatam_amd/post_opt.py, slam.get_loss_gs, the learning-rate schedule) held to a recording of
the REFERENCE'S OWN scripts/post_splatam_opt.py (tests/golden/make_golden_postopt.py, run where /root/reference exists, on the C
oracle).  CPU only: the rasterizer behind ``slam.Renderer`` is the oracle here, exactly as it was when the fixture was generated.
The HIP half is tests/test_gpu_postopt.py."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import dataset_files as files
import loop_trace as LT
from tests.util import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "postopt_reference.npz"))
PARAM_KEYS = ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales', 'cam_unnorm_rots', 'cam_trans')
GAUSSIAN_KEYS = PARAM_KEYS[:5]


def seed_everything(seed):
    """/root/reference/utils/common_utils.py:8-22"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


@pytest.fixture
def oracle(monkeypatch):
    from oracle import c_ref
    from splatam_amd import slam
    monkeypatch.setattr(slam, "Renderer", c_ref.CRasterizer)
    return slam


def loss_case(name, device="cpu"):
    """(params, curr_data at the frame's own pose, (n, W, H, f, cx, cy, t), the negative-depth pixel) of a recorded loss case."""
    from splatam_amd import slam
    n, W, H, f, cx, cy, t, ny, nx = GOLD[f"loss/{name}/meta"]
    n, W, H, t = int(n), int(W), int(H), int(t)
    params = {k: torch.tensor(GOLD[f"loss/{name}/param/{k}"], device=device) for k in PARAM_KEYS}
    w2c = torch.tensor(GOLD[f"loss/{name}/w2c"], device=device)
    k = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    cam = slam.setup_camera(W, H, k, GOLD[f"loss/{name}/w2c"], device=device)
    curr = {'cam': cam, 'im': torch.tensor(GOLD[f"loss/{name}/im"], device=device), 'depth': torch.tensor(GOLD[f"loss/{name}/depth"], device=device),
            'id': t, 'w2c': w2c}
    return params, curr, (n, W, H, f, cx, cy, t), (int(ny), int(nx))


# ---------------------------------------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_get_loss_gs_matches_reference_code(oracle, name):
    """Loss, both weighted terms and every parameter gradient of the reference's get_loss_gs, at the tolerances of the golden test of
    get_loss (tests/test_slam_mirror.py); the frame has a block of zero depth and one pixel of negative depth."""
    slam = oracle
    params, curr, (n, W, H, f, cx, cy, t), neg = loss_case(name)
    depth = curr['depth']
    assert 0.15 <= float((depth[:, : H // 2, : (2 * W) // 5] == 0).sum()) / (H * W) <= 0.25        # the block: about a fifth of the image
    assert float(depth[0, neg[0], neg[1]]) < 0 and int((depth < 0).sum()) == 1
    P = {k: torch.nn.Parameter(v.clone()) for k, v in params.items()}
    variables = {'max_2D_radius': torch.zeros(n), 'means2D_gradient_accum': torch.zeros(n), 'denom': torch.zeros(n)}
    loss, variables, wl = slam.get_loss_gs(P, curr, variables, dict(im=0.5, depth=1.0))
    loss.backward()
    want = GOLD[f"loss/{name}/loss"]
    np.testing.assert_allclose(np.array([loss.item(), wl['im'].item(), wl['depth'].item()]), want, rtol=2e-5)
    for k in PARAM_KEYS:
        ref = GOLD[f"loss/{name}/grad/{k}"]
        g = torch.zeros_like(P[k]) if P[k].grad is None else P[k].grad
        scale = np.abs(ref).max() + 1e-20
        assert np.abs(g.numpy() - ref).max() <= 2e-4 * scale + 1e-12, (k, np.abs(g.numpy() - ref).max(), scale)
    assert P['cam_unnorm_rots'].grad is None and P['cam_trans'].grad is None                     # no pose gradient
    np.testing.assert_array_equal(variables['max_2D_radius'].numpy(), GOLD[f"loss/{name}/max_2D_radius"])
    ref = GOLD[f"loss/{name}/means2D_grad"]
    assert np.abs(variables['means2D'].grad.numpy() - ref).max() <= 2e-4 * (np.abs(ref).max() + 1e-20)
    assert np.array_equal(variables['seen'].numpy(), GOLD[f"loss/{name}/max_2D_radius"] > 0)


@pytest.mark.parametrize("name", ["a", "b"])
def test_get_loss_gs_is_not_get_loss(oracle, name):
    """get_loss(mapping=True) on the same input -- the same map seen from the same pose through the transform to frame t -- has the
    same image term and ANOTHER depth term: its masked sum runs over gt > 0 and is divided by the mask count."""
    slam = oracle
    params, curr, (n, W, H, f, cx, cy, t), _ = loss_case(name)
    cam0 = slam.setup_camera(W, H, [[f, 0, cx], [0, f, cy], [0, 0, 1]], np.eye(4, dtype=np.float32), device="cpu")
    frame = dict(curr, cam=cam0, w2c=torch.eye(4))
    variables = {'max_2D_radius': torch.zeros(n)}
    cfg = slam.REPLICA_MAPPING
    params = {k: torch.nn.Parameter(v) for k, v in params.items()}
    _, _, wl = slam.get_loss(params, frame, dict(variables), t, dict(im=0.5, depth=1.0), cfg['use_sil_for_loss'], cfg['sil_thres'], True, False,
                             mapping=True)
    _, _, wl_gs = slam.get_loss_gs(params, curr, dict(variables), dict(im=0.5, depth=1.0))
    want = GOLD[f"loss/{name}/loss"]
    assert abs(float(wl_gs['depth'].detach()) - want[2]) <= 2e-5 * want[2]
    assert abs(float(wl['im'].detach()) - want[1]) <= 1e-3 * want[1]                   # the image term is shared (camera moved vs Gaussians moved)
    assert abs(float(wl['depth'].detach()) - want[2]) > 0.05 * want[2], (float(wl['depth'].detach()), want[2])
    # ... and it is the normaliser and the mask, nothing else: sum over (gt > 0) = sum over (gt != 0) - the negative pixel's share
    count_pos, HW = float((curr['depth'] > 0).sum()), float(H * W)
    assert float(wl['depth'].detach()) * count_pos < want[2] * HW


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-pixel arithmetic of the kernels, on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def shim():
    L = host_shim("postopt_math_shim", "fused_math.h")
    L.pm_depth_divisor.restype = C.c_float
    L.pm_depth_divisor.argtypes = [C.c_int, C.c_float, C.c_float]
    L.pm_depth_grad.restype = C.c_float
    L.pm_depth_grad.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]
    return L


def _pixels():
    #                  valid      exact match   missing   negative   missing + NaN render   NaN depth sensor
    depth = np.array([2.0, 1.5,   3.0,          2.5,      2.0,       np.nan,                1.0], dtype=np.float32)
    gt = np.array([2.5, 1.0,      3.0,          0.0,      -2.0,      0.0,                   np.nan], dtype=np.float32)
    return depth, gt


def test_gs_depth_pixel(shim):
    depth, gt = _pixels()
    n = depth.size
    mask, err, sign = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    shim.pm_depth_pixel_gs(n, _p(depth), _p(gt), _p(mask, C.c_int), _p(err), _p(sign))
    assert mask.tolist() == [1, 1, 1, 0, 1, 0, 1]                     # gt != 0: the negative depth and the NaN are inside
    np.testing.assert_array_equal(err[:6], np.array([0.5, 0.5, 0.0, 0.0, 4.0, 0.0], dtype=np.float32))
    assert np.isnan(err[6])                                           # as upstream: |depth - nan|
    np.testing.assert_array_equal(sign[:6], np.array([-1.0, 1.0, 0.0, 0.0, 1.0, 0.0], dtype=np.float32))
    # torch's statement of the same pixels (finite render): |depth * valid - gt| and autograd's sign
    d = torch.tensor(depth[:5], requires_grad=True)
    g = torch.tensor(gt[:5])
    torch.abs(d * (g != 0) - g).sum().backward()
    np.testing.assert_array_equal(err[:5], torch.abs(d * (g != 0) - g).detach().numpy())
    np.testing.assert_array_equal(sign[:5], d.grad.numpy())
    # get_loss' mask on the same pixels leaves the negative depth out
    mask2, err2, sign2 = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    dsq = (depth * depth).astype(np.float32)
    shim.pm_depth_pixel_map(n, _p(depth), _p(dsq), _p(gt), _p(mask2, C.c_int), _p(err2), _p(sign2))
    assert mask2.tolist() == [1, 1, 1, 0, 0, 0, 0]


def test_gs_divisor_gradient_and_frame_model(shim):
    assert shim.pm_depth_divisor(1, 123.0, 4928.0) == 4928.0 and shim.pm_depth_divisor(0, 123.0, 4928.0) == 123.0
    assert shim.pm_depth_grad(1, 1.0, -1.0, 4928.0) == np.float32(-1.0) / np.float32(4928.0)
    assert shim.pm_depth_grad(1, 0.5, 1.0, 3.0) == np.float32(0.5) / np.float32(3.0) and shim.pm_depth_grad(0, 0.5, 1.0, 3.0) == 0.0
    # a frame against torch: the recorded frame of loss case "a" with a render made up from its depth
    gt = GOLD["loss/a/depth"][0].ravel().astype(np.float32)
    rng = np.random.default_rng(0)
    depth = (np.abs(gt) + 0.1 * rng.standard_normal(gt.size)).astype(np.float32) + 1.0
    dsq = depth * depth
    HW = gt.size
    for gs in (1, 0):
        sums, term, grad = np.zeros(2), C.c_float(0), np.zeros(HW, np.float32)
        shim.pm_frame(gs, HW, _p(depth), _p(dsq), _p(gt), C.c_float(1.0), _p(sums, C.c_double), C.byref(term), _p(grad))
        d = torch.tensor(depth, requires_grad=True)
        g = torch.tensor(gt)
        if gs:
            want = torch.abs(d * (g != 0) - g).mean()
        else:
            m = g > 0
            want = torch.where(m, torch.abs(g - d), torch.zeros(())).sum() / m.sum()
        want.backward()
        assert abs(term.value - float(want)) <= 2e-6 * float(want), (gs, term.value, float(want))
        np.testing.assert_allclose(grad, d.grad.numpy(), rtol=1e-6, atol=0)
        assert sums[1] == float(((g != 0) if gs else (g > 0)).sum())


def test_gs_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    """The same header as a stand-alone host program (its own main) built with -fsanitize=address,undefined: it models a frame in
    both modes and checks it against an independent loop; any sanitizer report or mismatch is a non-zero exit.  The sanitizer runtimes
    are linked statically, so the program starts in whatever environment the test runs in (nothing of it is changed)."""
    exe = str(tmp_path / "postopt_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DPOSTOPT_SHIM_MAIN", "-o", exe, os.path.join(HERE, "postopt_math_shim.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout


# ---------------------------------------------------------------------------------------------------------------------------------
# the learning-rate schedule
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", [0.01, 1.0])
def test_expon_lr_schedule(mult):
    from splatam_amd import slam
    lr_init, lr_final, max_steps = GOLD["lr/args"]
    steps = GOLD["lr/steps"]
    assert steps.tolist() == [1, 2, int(max_steps) // 2, int(max_steps)]
    as_script = slam.get_expon_lr_func(lr_init=lr_init, lr_final=lr_final, lr_delay_mult=mult, max_steps=int(max_steps))
    delayed = slam.get_expon_lr_func(lr_init=lr_init, lr_final=lr_final, lr_delay_steps=100, lr_delay_mult=mult, max_steps=int(max_steps))
    np.testing.assert_allclose([as_script(int(s)) for s in steps], GOLD[f"lr/mult{mult}/script"], rtol=1e-14)
    np.testing.assert_allclose([delayed(int(s)) for s in steps], GOLD[f"lr/mult{mult}/delay100"], rtol=1e-14)
    assert as_script(int(max_steps)) == pytest.approx(lr_final, rel=1e-12) and as_script(0) == pytest.approx(lr_init, rel=1e-12)
    assert [slam.get_expon_lr_func(0.0, 0.0)(5), as_script(-1)] == GOLD["lr/disabled"].tolist() == [0.0, 0.0]
    opt = torch.optim.Adam([{'params': [torch.nn.Parameter(torch.zeros(1))], 'name': 'means3D', 'lr': 1.0},
                            {'params': [torch.nn.Parameter(torch.zeros(1))], 'name': 'rgb_colors', 'lr': 2.0}])
    assert slam.update_learning_rate(opt, as_script, 2) == as_script(2)
    assert [g['lr'] for g in opt.param_groups] == [as_script(2), 2.0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------
def loop_config(run_name, tmp_path):
    """The recorded configuration with the finished run's params.npz written where it names it."""
    cfg = json.loads(str(GOLD[f"loop/{run_name}/config"]))
    ckpt = str(tmp_path / "finished.npz")
    np.savez(ckpt, **{k[len("loop/ckpt/"):]: GOLD[k] for k in GOLD.files if k.startswith("loop/ckpt/")})
    cfg['workdir'], cfg['data']['param_ckpt_path'] = str(tmp_path), ckpt
    return cfg


def run_mirror(run_name, tmp_path, **kw):
    from splatam_amd import post_opt
    cfg = loop_config(run_name, tmp_path)
    ds = LT.RecordedRGBDSequence(GOLD, "loop")
    seed_everything(cfg['seed'])
    return (cfg,) + post_opt.post_splatam_opt(cfg, engine="mirror", dataset=ds, **kw)


@pytest.fixture(scope="module")
def mirror_dens(tmp_path_factory):
    from oracle import c_ref
    from splatam_amd import slam
    saved = slam.Renderer
    slam.Renderer = c_ref.CRasterizer
    try:
        return run_mirror("dens", tmp_path_factory.mktemp("postopt_dens"), evaluate=False)
    finally:
        slam.Renderer = saved


def test_recorded_case_is_the_one_the_issue_names():
    cfg = json.loads(str(GOLD["loop/dens/config"]))
    dd = cfg['train']['densify_dict']
    assert (dd['start_after'], dd['densify_every'], dd['remove_big_after'], dd['reset_opacities_every'], dd['stop_after']) == (5, 10, 20, 20, 40)
    assert cfg['train']['num_iters_mapping'] == 40 and GOLD["loop/frames/color"].shape == (3, 48, 64, 3)
    assert GOLD["loop/ckpt/means3D"].shape[0] == 600
    q = GOLD["loop/ckpt/cam_unnorm_rots"][0].T
    assert len({tuple(np.round(r, 6)) for r in q}) == 3                   # three distinct poses
    assert GOLD["loop/dens/rows"][:, 0].tolist() == [10, 20, 30] and GOLD["loop/dens/rows"][0, 2] != GOLD["loop/dens/rows"][0, 1]


def test_mirror_loop_takes_the_reference_loops_decisions(mirror_dens):
    cfg, params, variables, stats, path = mirror_dens
    assert stats['views'] == GOLD["loop/dens/views"].tolist()                       # the same frame in every iteration
    assert [list(r) for r in stats['rows']] == GOLD["loop/dens/rows"].tolist()      # the same rows after every densification
    assert params['means3D'].shape[0] == GOLD["loop/dens/final/means3D"].shape[0]


def test_mirror_loop_losses_and_final_state(mirror_dens):
    """The tolerances of the whole-loop golden test (tests/test_loop_golden.py): losses to rounding at first, then drifting apart by
    what Adam (eps 1e-15) makes of rounding; final values per tensor in units of its learning rate."""
    cfg, params, variables, stats, path = mirror_dens
    gold = GOLD["loop/dens/losses"]
    rel = np.abs(np.array(stats['losses']) - gold) / np.abs(gold)
    print(f"{len(gold)} losses, relative difference: first three {rel[:3].max():.1e}, median {np.median(rel):.1e}, max {rel.max():.1e}")
    assert rel[:3].max() < 1e-6 and np.median(rel) < 2e-5 and rel.max() < 2e-3
    steps = cfg['train']['num_iters_mapping']
    for k in GAUSSIAN_KEYS:
        want, got = GOLD[f"loop/dens/final/{k}"], params[k].detach().numpy()
        assert want.shape == got.shape, k
        d, lr = np.abs(want - got), cfg['train']['lrs_mapping'][k]
        q50, q99 = np.quantile(d, [0.5, 0.99])
        print(f"{k}: |difference| / lr: median {q50 / lr:.1e}, 99 % {q99 / lr:.2f}, max {d.max() / lr:.2f} ({steps} steps)")
        assert q50 <= 0.01 * lr and q99 <= 2 * lr and d.max() <= steps * lr, k
    for k in ('cam_unnorm_rots', 'cam_trans'):                                       # the poses do not move
        assert np.array_equal(GOLD[f"loop/dens/final/{k}"], params[k].detach().numpy()) and np.array_equal(GOLD[f"loop/ckpt/{k}"], GOLD[f"loop/dens/final/{k}"])
    assert np.array_equal(GOLD["loop/dens/final/timestep"], variables['timestep'].numpy())


def test_written_params_are_the_reference_scripts(mirror_dens):
    """params.npz: exactly the reference's entries, dtypes and shapes; gt_w2c_all_frames holds the ESTIMATED poses."""
    from splatam_amd import post_opt
    cfg, params, variables, stats, path = mirror_dens
    got = dict(np.load(path, allow_pickle=True))
    want = {k[len("loop/dens/final/"):]: GOLD[k] for k in GOLD.files if k.startswith("loop/dens/final/")}
    assert sorted(got) == sorted(want) and 'keyframe_time_indices' not in got
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (k, got[k].dtype, w.dtype, got[k].shape, w.shape)
    loaded = {k: torch.tensor(GOLD[f"loop/ckpt/{k}"]) for k in ('cam_unnorm_rots', 'cam_trans')}
    poses = np.stack([post_opt.estimated_w2c(loaded, t).numpy() for t in range(3)])
    assert np.array_equal(got['gt_w2c_all_frames'], poses)
    np.testing.assert_allclose(got['gt_w2c_all_frames'], want['gt_w2c_all_frames'], rtol=0, atol=1e-6)
    assert not np.allclose(got['gt_w2c_all_frames'][1], np.eye(4), atol=1e-3)
    for k in ('intrinsics', 'w2c', 'org_width', 'org_height'):
        assert np.array_equal(got[k], want[k]), k


def test_mirror_loop_without_densification_and_with_evaluation(oracle, tmp_path):
    cfg, params, variables, stats, path = run_mirror("plain", tmp_path, num_iters=12)
    assert stats['views'] == GOLD["loop/plain/views"][:12].tolist() and stats['rows'] == []
    rel = np.abs(np.array(stats['losses']) - GOLD["loop/plain/losses"][:12]) / GOLD["loop/plain/losses"][:12]
    assert rel[:3].max() < 1e-6 and rel.max() < 2e-3
    ev = stats['eval']
    assert stats['eval_7k'] is None and ev is not None and np.isfinite(ev['avg_psnr']) and len(ev['psnr']) == 3
    assert os.path.exists(os.path.join(cfg['workdir'], cfg['run_name'], "eval", "psnr.txt"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
CONFIG_PY = """
config = dict(
    workdir={workdir!r}, run_name="refined", seed=0, primary_device="cpu", report_iter_progress=False, use_wandb={wandb},
    data=dict(basedir={basedir!r}, gradslam_data_cfg={yaml!r}, sequence="room", desired_image_height=24, desired_image_width=32, start=0,
              end=-1, stride=1, num_frames=3, eval_stride=1, eval_num_frames=3, param_ckpt_path={ckpt!r}),
    train=dict(num_iters_mapping=40, sil_thres=0.5, loss_weights=dict(im=0.5, depth=1.0),
               lrs_mapping=dict(means3D=0.00032, rgb_colors=0.0025, unnorm_rotations=0.001, logit_opacities=0.05, log_scales=0.005,
                                cam_unnorm_rots=0.0, cam_trans=0.0),
               lrs_mapping_means3D_final=0.0000032, lr_delay_mult=0.01, use_gaussian_splatting_densification=True,
               densify_dict=dict(start_after=1, remove_big_after=3, stop_after=40, densify_every=2, grad_thresh=0.0002, num_to_split_into=2,
                                 removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005, reset_opacities=True,
                                 reset_opacities_every=4)))
"""


def write_experiment(tmp_path, wandb=False):
    from oracle import raster_ref as R
    W, H, f = 32, 24, 28.0
    root = str(tmp_path / "data")
    files.write_replica(root, "room", files.seeded_frames(3, W, H, seed=4), files.seeded_poses(3, seed=4))
    yaml = tmp_path / "replica.yaml"
    yaml.write_text(f"dataset_name: 'replica'\ncamera_params:\n  image_height: {H}\n  image_width: {W}\n  fx: {f}\n  fy: {f}\n  cx: {W / 2 - 0.5}\n"
                    f"  cy: {H / 2 - 0.5}\n  png_depth_scale: 6553.5\n  crop_edge: 0\n")
    n = 150
    p = R.synthetic_cloud(n, W, H, f, f, W / 2 - 0.5, H / 2 - 0.5, seed=3, anisotropic=False)
    rots = np.zeros((1, 4, 3), dtype=np.float32)
    rots[0, 0] = 1.0
    rots[0, 1] = [0.0, 0.01, -0.01]
    ckpt = {k: v.numpy() for k, v in p.items()}
    ckpt.update(cam_unnorm_rots=rots, cam_trans=np.array([[[0.0, 0.01, 0.02]] * 3], dtype=np.float32).reshape(1, 3, 3),
                timestep=np.zeros(n, dtype=np.float32), intrinsics=np.eye(3, dtype=np.float32), w2c=np.eye(4, dtype=np.float32), org_width=W,
                org_height=H, gt_w2c_all_frames=np.stack([np.eye(4, dtype=np.float32)] * 3), keyframe_time_indices=np.array([0]))
    path = str(tmp_path / "finished.npz")
    np.savez(path, **ckpt)
    exp = tmp_path / "post_splatam_opt.py"
    exp.write_text(CONFIG_PY.format(workdir=str(tmp_path / "out"), basedir=root, yaml=str(yaml), ckpt=path, wandb=wandb))
    return str(exp), n


def test_command_line_runs_a_tiny_refinement(oracle, tmp_path, capsys):
    from splatam_amd import post_opt
    exp, n = write_experiment(tmp_path)
    assert post_opt.main([exp, "--engine", "mirror", "--no-eval", "--num-iters", "5"]) == 0
    out = str(tmp_path / "out" / "refined")
    saved = dict(np.load(os.path.join(out, "params.npz"), allow_pickle=True))
    assert os.path.exists(os.path.join(out, "config.py")) and not os.path.exists(os.path.join(out, "eval"))
    assert saved['gt_w2c_all_frames'].shape == (3, 4, 4) and saved['means3D'].shape[1] == 3 and saved['timestep'].shape[0] == saved['means3D'].shape[0]
    assert saved['intrinsics'].shape == (4, 4) and int(saved['org_width']) == 32
    assert "5 iterations" in capsys.readouterr().out


@pytest.mark.parametrize("key", ["use_wandb", "report_iter_progress"])
def test_command_line_refuses_what_it_cannot_honour(tmp_path, key):
    from splatam_amd import post_opt
    exp, _ = write_experiment(tmp_path, wandb=(key == "use_wandb"))
    if key == "report_iter_progress":
        text = open(exp).read().replace("report_iter_progress=False", "report_iter_progress=True")
        open(exp, "w").write(text)
    with pytest.raises(SystemExit, match=key):
        post_opt.main([exp, "--engine", "mirror", "--no-eval", "--num-iters", "5"])
    assert not os.path.exists(str(tmp_path / "out"))            # ... before anything is written
