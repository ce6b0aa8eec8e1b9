"""The refinement of a finished map on the device: the ``gs`` mode of the fused mapping loss (csrc/fused.hip, get_loss_gs of
/root/reference/scripts/post_splatam_opt.py:111-147) against the float32 / float64 C oracle, its normaliser, the driver
(splatam_amd/post_opt.py, engine="fused") against the recording of the reference's own script (tests/golden/postopt_reference.npz)
and the additive C ABI.  The CPU half is tests/test_postopt_cpu.py.

The loss comparison reuses the staged acceptance of tests/test_gpu_configs.py (imported, not edited): (A) rendered planes 1e-4 with
every excess explained by the float64 oracle, (B) loss 1e-4, (C) gradient planes equal except at kinks, (D) parameter gradients
1e-3 of the maximum with every row beyond it explained by the float64 oracle (assert_grad_outliers_explained) at the 88 x 56 /
2 000-Gaussian shape, and there AND calibrated against the float32 oracle's own noise (assert_grad_calibrated, as it is) at 264 x 168 /
20 000 Gaussians -- three times the frame at the same density: its count statement allows 1e-4 of a tensor's elements, which is
less than one element of a 2 000-row tensor and two or more of a 20 000-row one.  Its oracle is swapped for get_loss_gs: world-frame Gaussians through a
camera AT the frame's pose, which is what the reference renders -- the engine transforms the Gaussians to frame t under an identity
camera instead, and stage (A) is where the two are held together."""
import ctypes as C

import numpy as np
import pytest
import torch

import loop_trace as LT
import test_gpu_configs as TC
from test_postopt_cpu import GOLD, loop_config, seed_everything
from tests.util import assert_grad_calibrated, assert_grad_outliers_explained, flip_pixels, oracle_flip_bounds

pytestmark = pytest.mark.gpu

W, H, N = 88, 56, 2000          # 5.5 x 3.5 tiles of 16: wider than the 11-tap window, a partial tile on both edges
CAM = dict(fx=80.0, fy=78.0, cx=43.2, cy=27.6)
# the same camera at three times the frame, ten times the Gaussians (16.5 x 10.5 tiles): where assert_grad_calibrated's rate resolves
LARGE = dict(W=264, H=168, N=20000, cam=dict(fx=240.0, fy=234.0, cx=129.6, cy=82.8))
SMALL = dict(W=W, H=H, N=N, cam=CAM)
GS = dict(loss='gs', loss_weights=dict(im=0.5, depth=1.0))


def _case(aniso, time_idx, seed=0, negative=True, size=SMALL):
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    c, W, H, N = size['cam'], size['W'], size['H'], size['N']
    params, variables = slam.synthetic_params(N, W, H, c['fx'], c['fy'], c['cx'], c['cy'], num_frames=3, seed=seed, device="cuda", anisotropic=aniso)
    k = [[c['fx'], 0, c['cx']], [0, c['fy'], c['cy']], [0, 0, 1]]
    w2c = torch.eye(4, device="cuda")
    cam = slam.setup_camera(W, H, k, np.eye(4, dtype=np.float32), device="cuda")
    im, depth = slam.synthetic_frame(params, cam, w2c, time_idx, rot_deg=0.4, trans_m=0.01)
    g = torch.Generator().manual_seed(seed + 1)
    im = (im + 0.03 * torch.randn(im.shape, generator=g).cuda()).clamp(0, 1).contiguous()
    depth = (depth * (1 + 0.01 * torch.randn(depth.shape, generator=g).cuda())).contiguous()
    depth[:, : H // 2, : (2 * W) // 5] = 0.0                    # the block of missing depth: a fifth of the image
    if negative:
        ys, xs = torch.nonzero(depth[0] > 0, as_tuple=True)
        i = len(ys) // 2
        depth[0, ys[i], xs[i]] = -depth[0, ys[i], xs[i]]        # one pixel of negative depth: inside the gs mask
    with torch.no_grad():                                       # two distinct, non-identity poses
        params['cam_unnorm_rots'][0, :, 1] = torch.tensor([0.98, 0.01, -0.02, 0.015], device="cuda") * 1.1
        params['cam_trans'][0, :, 1] = torch.tensor([0.01, -0.02, 0.015], device="cuda")
        params['cam_unnorm_rots'][0, :, 2] = torch.tensor([0.97, -0.02, 0.015, 0.01], device="cuda") * 0.9
        params['cam_trans'][0, :, 2] = torch.tensor([-0.015, 0.01, 0.02], device="cuda")
    frame = {'cam': cam, 'im': im, 'depth': depth, 'id': time_idx, 'w2c': w2c}
    return FusedEngine(params, cam), params, variables, frame, (W, H, k)


def _oracle_get_loss_gs(params, frame, variables, cam_args, cfg, tracking, monkeypatch, time_idx=1, first_w2c=None, frame_w2c=None):
    """What test_gpu_configs._oracle_get_loss returns, for get_loss_gs: the reference-shaped statements on CPU tensors with the C oracle as
    Renderer, the camera built at the estimated pose of ``time_idx`` as the refinement script builds it."""
    from splatam_amd import post_opt, slam
    assert not tracking and first_w2c is None and frame_w2c is None
    monkeypatch.setattr(slam, "Renderer", TC._Spy)
    TC._Spy.renders = []
    Wc, Hc, k = cam_args
    pc = {k_: torch.nn.Parameter(v.detach().cpu().clone()) for k_, v in params.items()}
    w2c_t = post_opt.estimated_w2c(pc, time_idx)
    curr = {'cam': slam.setup_camera(Wc, Hc, k, w2c_t.numpy(), device="cpu"), 'im': frame['im'].cpu(), 'depth': frame['depth'].cpu(), 'id': time_idx,
            'w2c': w2c_t}
    vc = {k_: v.cpu().clone() for k_, v in variables.items()}
    loss, _, wl = slam.get_loss_gs(pc, curr, vc, cfg['loss_weights'])
    loss.backward()
    im, ds = TC._Spy.renders
    _oracle_get_loss_gs.terms = (float(wl['depth'].detach()), float(wl['im'].detach()))
    _oracle_get_loss_gs.renders = (im.detach().numpy(), ds.detach().numpy())
    return float(loss.detach()), [im.detach(), ds.detach()], [im.grad, ds.grad if ds.grad is not None else torch.zeros_like(ds)]


def _flipped_pixels(eng, params, frame, cam_args, time_idx):
    """Pixels where a float32 decision flip HAPPENED between the engine's renders and the oracle's (tests/util.py: flip_pixels on the
    float64 oracle's account of both renders), with the float64 centres and radii of the Gaussians."""
    from splatam_amd import slam
    pc64, frame64 = TC._cpu_case(params, frame, cam_args, torch.float64, time_idx)
    with torch.no_grad():
        tg64 = slam.transform_to_frame(pc64, time_idx, gaussians_grad=False, camera_grad=False)
        b_im, _, xy, radii, _ = oracle_flip_bounds(slam.transformed_params2rendervar(pc64, tg64), frame64['cam'])
        b_ds, _, _, _, _ = oracle_flip_bounds(slam.transformed_params2depthplussilhouette(pc64, frame64['w2c'], tg64), frame64['cam'])
    imf, depthf, silf, dsqf = eng.rendered()
    ref_im, ref_ds = _oracle_get_loss_gs.renders
    flagged = flip_pixels(b_im, (imf.cpu().numpy(),), (ref_im,)) | flip_pixels(b_ds, (torch.cat([depthf, silf[None], dsqf]).cpu().numpy(),), (ref_ds,))
    return flagged, xy, radii


GS_CASES = [(False, 1), (True, 2), (True, 1), (False, 2)]


@pytest.mark.parametrize("aniso,time_idx", GS_CASES)
def test_fused_gs_loss_vs_oracle(aniso, time_idx, monkeypatch):
    _run_gs_case(aniso, time_idx, monkeypatch, SMALL)


@pytest.mark.parametrize("aniso,time_idx", [(False, 2), (True, 1)])
def test_fused_gs_loss_vs_oracle_calibrated(aniso, time_idx, monkeypatch):
    """The same stages where the per-tensor statements of assert_grad_calibrated resolve (20 000 rows: 20 000 .. 80 000 elements)."""
    _run_gs_case(aniso, time_idx, monkeypatch, LARGE)


def _run_gs_case(aniso, time_idx, monkeypatch, size):
    from splatam_amd import _capi, slam
    eng, params, variables, frame, cam_args = _case(aniso, time_idx, size=size)
    # the existing mapping mode on this engine, before: twice (the second on the lists the first one's statistics sized)
    for _ in range(2):
        eng.loss_backward(frame, time_idx, slam.REPLICA_MAPPING, tracking=False)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
    before = dict(report=eng.buf['d_cam'].clone(), planes=eng.buf['dL_dout6'].clone(), out6=eng.buf['out6'].clone(),
                  grads={k: v.clone() for k, v in eng.grads.items()})
    eng.loss_backward(frame, time_idx, GS, tracking=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    what = f"fused gs {size['W']} x {size['H']} {'aniso' if aniso else 'iso'} t={time_idx}"
    monkeypatch.setattr(TC, "_oracle_get_loss", _oracle_get_loss_gs)
    g32, g64 = TC._fused_stages(eng, params, variables, frame, cam_args, size['cam'], GS, False, what, monkeypatch, time_idx=time_idx)
    rep = eng.buf['d_cam'].cpu().numpy().astype(np.float64)
    d_term, im_term = _oracle_get_loss_gs.terms
    print(f"{what}: loss {rep[_capi.SPLAT_REPORT_LOSS]:.7f}, depth term {rep[_capi.SPLAT_REPORT_DEPTH_TERM]:.7f} (oracle {d_term:.7f}), "
          f"image term {rep[_capi.SPLAT_REPORT_IM_TERM]:.7f} (oracle {im_term:.7f})")
    assert abs(rep[_capi.SPLAT_REPORT_DEPTH_TERM] - d_term) <= 1e-4 * abs(d_term)
    assert abs(rep[_capi.SPLAT_REPORT_IM_TERM] - im_term) <= 1e-4 * abs(im_term)
    assert rep[_capi.SPLAT_REPORT_LOSS] == np.float32(np.float32(rep[_capi.SPLAT_REPORT_DEPTH_TERM]) + np.float32(rep[_capi.SPLAT_REPORT_IM_TERM]))
    assert rep[_capi.SPLAT_REPORT_SUMS + 2] == float((frame['depth'] != 0).sum())          # the gs mask's count
    assert float(np.abs(rep[_capi.SPLAT_REPORT_DROT:_capi.SPLAT_REPORT_DROT + 7]).max()) == 0.0      # no pose gradient
    keys = ["means3D", "rgb_colors", "logit_opacities", "log_scales"] + (["unnorm_rotations"] if aniso else [])
    tail = 2.0 if eng.depth_tie_pixels == 0 else 3.0                 # (as test_gpu_configs.test_fused_mapping_vs_oracle)
    flagged, xy, radii = _flipped_pixels(eng, params, frame, cam_args, time_idx)
    for k in keys:
        got = eng.grads[k].cpu().numpy()
        assert np.isfinite(got).all(), k
        # 1e-3 of the tensor's maximum; a row beyond it lies over a pixel where the float64 oracle finds a float32 decision that flipped
        assert_grad_outliers_explained(got, g32[k], flagged, xy, radii, what=f"{what} grad {k}")
        if size is LARGE:
            assert_grad_calibrated(got, g32[k], g64[k], what=f"{what} grad {k}", tail_factor=tail)
    if not aniso:
        assert float(eng.grads["unnorm_rotations"].abs().max()) == 0.0
    # ... and the mode leaves nothing behind: the mapping mode again gives what it gave before (planes bit for bit; the parameter
    # gradients are sums of float atomics, equal to the order of their rounding)
    eng.loss_backward(frame, time_idx, slam.REPLICA_MAPPING, tracking=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    assert torch.equal(eng.buf['out6'], before['out6']) and torch.equal(eng.buf['dL_dout6'], before['planes'])
    r0, r1 = before['report'].cpu().numpy(), eng.buf['d_cam'].cpu().numpy()
    for slot in (_capi.SPLAT_REPORT_LOSS, _capi.SPLAT_REPORT_DEPTH_TERM, _capi.SPLAT_REPORT_IM_TERM):
        assert abs(float(r0[slot]) - float(r1[slot])) <= 2 * 2.0 ** -24 * abs(float(r0[slot])), (slot, r0[slot], r1[slot])
    assert r0[_capi.SPLAT_REPORT_SUMS + 2] == r1[_capi.SPLAT_REPORT_SUMS + 2] == float((frame['depth'] > 0).sum())
    for k, v in before['grads'].items():
        assert float((eng.grads[k] - v).abs().max()) <= 1e-5 * float(v.abs().max()) + 1e-30, k


def test_gs_and_mapping_terms_differ_by_the_normaliser_only():
    """Valid count well below H W, every valid depth positive (the two masks agree): REPORT_DEPTH_TERM(gs) * H W ==
    REPORT_DEPTH_TERM(mapping) * count.  Each term is one float32 division of the same sum (w_depth = 1), rounded to 2^-24 relative;
    the sum itself (double atomics, cast to float) may differ by one more rounding: 4 x 2^-24 in all."""
    from splatam_amd import _capi
    eng, params, variables, frame, _ = _case(False, 1, seed=3, negative=False)
    depth = frame['depth']
    count = float((depth > 0).sum())
    assert float((depth < 0).sum()) == 0 and count < 0.8 * H * W
    cfg_map = dict(use_sil_for_loss=False, sil_thres=0.5, use_l1=True, ignore_outlier_depth_loss=False, loss_weights=dict(im=0.5, depth=1.0))
    terms = {}
    for name, cfg in (("mapping", cfg_map), ("gs", GS)):
        eng.loss_backward(frame, 1, cfg, tracking=False)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        rep = eng.buf['d_cam'].cpu().numpy().astype(np.float64)
        assert rep[_capi.SPLAT_REPORT_SUMS + 2] == count
        terms[name] = (rep[_capi.SPLAT_REPORT_DEPTH_TERM], rep[_capi.SPLAT_REPORT_IM_TERM], rep[_capi.SPLAT_REPORT_SUMS])
    a, b = terms["gs"][0] * (H * W), terms["mapping"][0] * count
    print(f"depth term gs {terms['gs'][0]:.9g} x {H * W} = {a:.9g}; mapping {terms['mapping'][0]:.9g} x {count:.0f} = {b:.9g}; relative {abs(a - b) / b:.2e}")
    assert abs(a - b) <= 4 * 2.0 ** -24 * b
    assert abs(terms["gs"][1] - terms["mapping"][1]) <= 2 * 2.0 ** -24 * terms["mapping"][1]      # the image term is the same statement
    assert terms["gs"][0] < 0.9 * terms["mapping"][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------------------
def run_fused(run_name, tmp_path, edit=None, **kw):
    from splatam_amd import post_opt
    cfg = loop_config(run_name, tmp_path)
    cfg['primary_device'] = "cuda:0"
    if edit is not None:
        edit(cfg)
    ds = LT.RecordedRGBDSequence(GOLD, "loop", device="cuda")
    seed_everything(cfg['seed'])
    out = post_opt.post_splatam_opt(cfg, engine="fused", dataset=ds, **kw)
    torch.cuda.synchronize()
    return (cfg,) + out


def test_fused_driver_follows_the_reference_loop_without_densification(tmp_path):
    """40 iterations, densification off: the frame of every iteration, and the losses within the margin the GPU whole-loop test
    allows against its recording (tests/test_gpu_loop_golden.py: first 1e-4, median 2e-3, maximum 3e-2)."""
    cfg, params, variables, stats, path = run_fused("plain", tmp_path, evaluate=False, record_losses=True)
    assert stats['views'] == GOLD["loop/plain/views"].tolist() and stats['rows'] == [] and stats['redone_iterations'] == 0
    gold = GOLD["loop/plain/losses"]
    rel = np.abs(np.array(stats['losses']) - gold) / np.abs(gold)
    print(f"fused post-opt: {len(gold)} losses, relative difference to the reference loop: first {rel[0]:.1e}, median {np.median(rel):.1e}, max {rel.max():.1e}")
    assert rel[0] < 1e-4 and np.median(rel) < 2e-3 and rel.max() < 3e-2
    assert params['means3D'].shape[0] == 600 and all(bool(torch.isfinite(params[k]).all()) for k in params)
    assert not stats['engine'].check_overflow(grow=False)
    saved = dict(np.load(path, allow_pickle=True))
    assert sorted(saved) == sorted(k[len("loop/plain/final/"):] for k in GOLD.files if k.startswith("loop/plain/final/"))
    assert np.array_equal(saved['cam_trans'], GOLD["loop/ckpt/cam_trans"])


def test_fused_driver_densifies_on_schedule(tmp_path):
    """40 iterations with densification: the rows after the FIRST densification are the recording's (the later ones follow split
    samples drawn by another generator: rows change on schedule), nothing is NaN, the lists end clean, the evaluation is finite."""
    cfg, params, variables, stats, path = run_fused("dens", tmp_path, evaluate=True, record_losses=True)
    gold_rows = GOLD["loop/dens/rows"]
    assert stats['views'] == GOLD["loop/dens/views"].tolist()
    assert [r[0] for r in stats['rows']] == gold_rows[:, 0].tolist() == [10, 20, 30]
    print(f"rows at the densifications: {stats['rows']}; recorded {gold_rows.tolist()}")
    assert list(stats['rows'][0]) == gold_rows[0].tolist()
    assert stats['rows'][1][2] != stats['rows'][1][1] and stats['rows'][1][1] == stats['rows'][0][2]
    n = params['means3D'].shape[0]
    assert n == stats['rows'][-1][2] and variables['timestep'].shape[0] == n
    assert all(bool(torch.isfinite(params[k]).all()) for k in params) and np.isfinite(stats['losses']).all()
    assert not stats['engine'].check_overflow(grow=False)
    ev = stats['eval']
    assert stats['eval_7k'] is None and np.isfinite(ev['psnr']).all() and np.isfinite(ev['avg_psnr']) and len(ev['psnr']) == 3
    saved = dict(np.load(path, allow_pickle=True))
    assert saved['means3D'].shape == (n, 3) and saved['timestep'].shape == (n,) and saved['gt_w2c_all_frames'].shape == (3, 4, 4)


def test_fused_driver_takes_no_opacity_step_on_a_reset_iteration(tmp_path):
    """An opacity reset OFF the densification schedule (iteration 3 of 4; nothing is densified): the reference re-creates
    logit_opacities alone, so that iteration's optimizer.step() leaves it at inverse_sigmoid(0.01) and moves the other groups."""
    import math

    def edit(cfg):
        cfg['train']['densify_dict'].update(start_after=1000, reset_opacities_every=3)
    for name in ("four", "three"):
        (tmp_path / name).mkdir()
    _, p4, _, s4, _ = run_fused("dens", tmp_path / "four", edit=edit, evaluate=False, num_iters=4)
    p4 = {k: v.detach().clone() for k, v in p4.items()}
    _, p3, _, s3, _ = run_fused("dens", tmp_path / "three", edit=edit, evaluate=False, num_iters=3)
    assert s4['rows'] == [] and s4['views'][:3] == s3['views'] and s4['redone_iterations'] == 0
    reset = torch.full_like(p4['logit_opacities'], math.log(0.01 / (1 - 0.01)))
    assert torch.equal(p4['logit_opacities'], reset) and not torch.equal(p3['logit_opacities'].detach(), reset)
    for k in ('means3D', 'rgb_colors', 'log_scales'):
        assert not torch.equal(p4[k], p3[k].detach()), k


def test_fused_driver_runs_flagged_iterations_again(tmp_path, monkeypatch):
    """The engine starts the loop on per-tile buckets far too small (stride 64, longest list 40: a flag, not a fault), the flag is
    read every 2 iterations: the iterations the device skipped are run again as plain ones, each recorded with the frame it drew, and
    the mapping optimizer's step count ends at the number of iterations -- the skipped steps were taken back."""
    from splatam_amd import fused

    class SmallBuckets(fused.FusedEngine):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.tile_stride, self.max_list_hint = 64, 40
    monkeypatch.setattr(fused, "FusedEngine", SmallBuckets)
    cfg, params, variables, stats, path = run_fused("dens", tmp_path, evaluate=False, num_iters=6, check_every=2)
    print(f"redone iterations {stats['redone_iterations']}, views {stats['redone_views']}, map_step {stats['engine'].map_step}")
    assert stats['redone_iterations'] > 0
    assert len(stats['redone_views']) == stats['redone_iterations']
    assert stats['engine'].map_step == 6
    assert not stats['engine'].check_overflow(grow=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI: additions inside version 17
# ---------------------------------------------------------------------------------------------------------------------------------
def test_gs_entry_points_are_additive_within_abi_17():
    from splatam_amd import _capi, slam
    L = _capi.lib()
    assert L.splat_abi_version() == 17 == _capi.ABI_VERSION
    for name in ("splat_iter_loss_backward_ex", "splat_iter_mapping_step_ex", "splat_iter_loss_backward", "splat_iter_mapping_step"):
        assert hasattr(L, name), name
    assert L.splat_sizeof(b"SplatLossConfig") == 44 == C.sizeof(_capi.SplatLossConfig)              # the old struct is what it was
    assert L.splat_sizeof(b"SplatLossConfigEx") == 60 == C.sizeof(_capi.SplatLossConfigEx)
    assert _capi.SplatLossConfigEx.base.offset == 0 and _capi.SplatLossConfigEx.loss_mode.offset == 44
    # SPLAT_LOSS_SPLATAM through the new entry point is the old entry point; what the gs mode cannot express is refused
    eng, params, variables, frame, _ = _case(False, 1)
    cfg = slam.REPLICA_MAPPING
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    want = eng.buf['d_cam'].clone()
    ex = _capi.SplatLossConfigEx()
    C.memmove(C.byref(ex), C.byref(eng.loss_config(cfg, False)), C.sizeof(_capi.SplatLossConfig))
    ws, m, fr = eng._workspace(True, with_ssim=True), eng._map_struct(), eng._frame(frame, 1)

    def call(e):
        return L.splat_iter_loss_backward_ex(C.byref(eng._camera.struct), C.byref(m), C.byref(fr), C.byref(e), C.byref(ws), eng._stream())
    assert call(ex) == 0
    torch.cuda.synchronize()
    got = eng.buf['d_cam']
    assert abs(float(got[_capi.SPLAT_REPORT_LOSS]) - float(want[_capi.SPLAT_REPORT_LOSS])) <= 2 * 2.0 ** -24 * float(want[_capi.SPLAT_REPORT_LOSS])
    ex.loss_mode = 2
    assert call(ex) != 0
    ex.loss_mode = _capi.SPLAT_LOSS_GS
    for field in ("tracking", "camera_grad", "ignore_outlier_depth_loss", "defer_finish"):
        setattr(ex.base, field, 1)
        assert call(ex) != 0, field
        setattr(ex.base, field, 0)
    ex.reserved[1] = 1
    assert call(ex) != 0
    ex.reserved[1] = 0
    assert call(ex) == 0
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)


def test_plain_c_binding_still_builds_and_passes_unchanged():
    import subprocess
    from test_gpu_capi_c import build_capi_smoke
    exe = build_capi_smoke()
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "capi_smoke ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
