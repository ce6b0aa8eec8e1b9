"""LPIPS on the device (csrc/lpips.hip, splatam_amd/lpips.py) against the float64 numpy restatement (tests/lpips_ref.py): the MFMA lane
maps with exact integer data, each layer alone within 1e-6 S, the whole chain at 83 x 61 and 203 x 131, the exact cases, and the figure
through ``evaluate`` / ``evaluate_novel_views``.  All weights are ``random_weights(seed)``; every figure is printed before it is asserted
(profiles/lpips.md records them)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval_ref, lpips_ref, nvs_ref

pytestmark = pytest.mark.gpu

SIL_THRES = 0.5
SIZES = ((83, 61), (203, 131))          # taps 20x14, 9x6, 4x2 (16 output rows: under one MFMA tile) and 50x32, 24x15, 11x7


def layer_input_extents(W, H):
    """(w, h) of what each layer's convolution reads for a W x H image."""
    from splatam_amd import _capi, lpips
    L = _capi.lib()
    out = []
    for l in range(5):
        if l == 0:
            out.append((W, H))
        else:
            w, h = L.splat_lpips_tap_size(W, l - 1), L.splat_lpips_tap_size(H, l - 1)
            out.append(((w - 3) // 2 + 1, (h - 3) // 2 + 1) if lpips.CONV_GEOMETRY[l][2] else (w, h))
    return out


@pytest.fixture(scope="module")
def weights():
    from splatam_amd import lpips
    return lpips.random_weights(11)


@pytest.fixture(scope="module")
def net(weights):
    from splatam_amd import lpips
    return lpips.Lpips(weights, "cuda")


# ---------------------------------------------------------------------------------------------------------------- lane maps, exact
def _tap(k):
    return {11: (7, 2), 5: (3, 1), 3: (2, 0)}[k]            # (dy, dx): asymmetric, off the centre


@pytest.fixture(scope="module")
def delta_net():
    """Zero biases; output channel n of every layer holds ONE 1.0, at tap ``_tap(k)`` of input channel (7 n + 3) % Cin."""
    from splatam_amd import lpips
    cw = []
    for cout, cin, k, _ in lpips.CONV_SHAPES:
        w = torch.zeros(cout, cin, k, k)
        dy, dx = _tap(k)
        w[torch.arange(cout), (7 * torch.arange(cout) + 3) % cin, dy, dx] = 1.0
        cw.append(w)
    w = lpips.LpipsWeights(cw, [torch.zeros(s[0]) for s in lpips.CONV_SHAPES], [torch.ones(s[0]) for s in lpips.CONV_SHAPES])
    return lpips.Lpips(w, "cuda")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("layer", range(5))
def test_lane_maps_with_exact_integer_data(delta_net, layer, size):
    """The output must be the shifted, permuted input bit for bit: a row / column swap in an operand or in the result, or a wrong
    k -> (c, dy, dx) map, cannot pass."""
    from splatam_amd import lpips
    cout, cin, k, _ = lpips.CONV_SHAPES[layer]
    stride, pad, _ = lpips.CONV_GEOMETRY[layer]
    w, h = layer_input_extents(*size)[layer]
    rng = np.random.default_rng(100 * layer + w)
    x = rng.integers(0, 200, size=(2, cin, h, w)).astype(np.float32)
    y = delta_net.conv_layer(layer, torch.from_numpy(x).cuda()).cpu().numpy()
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    assert y.shape == (2, cout, ho, wo)
    dy, dx = _tap(k)
    xp = np.zeros((2, cin, h + 2 * pad, w + 2 * pad), dtype=np.float32)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    want = xp[:, (7 * np.arange(cout) + 3) % cin][:, :, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride]
    assert want.shape == y.shape and np.abs(want).max() > 0
    assert np.array_equal(y, want), (layer, int((y != want).sum()), y.size)


# ---------------------------------------------------------------------------------------------------------------- each layer alone
@pytest.fixture(scope="module")
def chains(weights):
    """The float64 restatement, once per size and seed: (image pair, value, taps, S, layer inputs)."""
    out = {}
    for W, H in SIZES:
        for seed in range(3):
            a, b = lpips_ref.image_pair(W, H, 1000 * seed + W)
            out[(W, H, seed)] = (a, b) + lpips_ref.lpips(a, b, weights)
    return out


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("layer", range(5))
def test_each_layer_alone_within_1e6_of_its_scale(net, weights, chains, layer, size):
    """True channel counts on the chain's own extents; the device and the restatement get the SAME float32 inputs.  Every element:
    |device - ref64| <= 1e-6 S, S = sum_k |a_k b_k| + |bias| (a k-ordered float32 chain measures 3.5e-7 S at K = 4096; worst case K 2^-24)."""
    from splatam_amd import lpips
    cw, cb, _ = lpips_ref.weights64(weights)
    stride, pad, _ = lpips.CONV_GEOMETRY[layer]
    x32 = chains[size + (0,)][5][layer].astype(np.float32)
    want, S = lpips_ref.conv_relu(x32.astype(np.float64), cw[layer], cb[layer], stride, pad)
    got = net.conv_layer(layer, torch.from_numpy(x32).cuda()).cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    ratio = np.abs(got - want) / S
    print(f"LPIPSLAYER layer={layer} input={x32.shape[3]}x{x32.shape[2]} K={cw[layer][0].size} max |device - ref64| / S = {ratio.max():.3e}")
    assert ratio.max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- the whole chain
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("size", SIZES)
def test_whole_chain_against_the_restatement(net, weights, chains, size, seed):
    """Every tap: max |tap - ref64| / max |ref64| at most 4 x the same statistic of ``slam.lpips`` in float32 on the CPU (both are
    float32 in different summation orders; the margin is the project's calibration against the float32 form's own noise).  The scalar:
    1e-4 relative (the project's colour tolerance, below the three decimals the figure is quoted to)."""
    from splatam_amd import slam
    W, H = size
    a, b, want, taps, _, _ = chains[size + (seed,)]
    got = net(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    dev_taps = [t.cpu().numpy().astype(np.float64) for t in net.taps(W, H)]
    got = float(got.cpu())
    v32, taps32 = slam.lpips(torch.from_numpy(a), torch.from_numpy(b), weights, return_taps=True)
    for l in range(5):
        assert dev_taps[l].shape == taps[l].shape
        scale = np.abs(taps[l]).max()
        e_dev, e_32 = np.abs(dev_taps[l] - taps[l]).max() / scale, np.abs(taps32[l].numpy().astype(np.float64) - taps[l]).max() / scale
        print(f"LPIPSCHAIN {W}x{H} seed={seed} tap{l}: device {e_dev:.3e}  float32 torch {e_32:.3e}  ratio {e_dev / e_32:.2f}")
        assert e_dev <= 4 * e_32, (l, e_dev, e_32)
    print(f"LPIPSCHAIN {W}x{H} seed={seed} value: ref64 {want:.9f} device rel {abs(got / want - 1):.3e} float32 torch rel {abs(float(v32) / want - 1):.3e}")
    assert want > 1e-3 and abs(got - want) <= 1e-4 * want


# ---------------------------------------------------------------------------------------------------------------- exact cases
def test_exact_cases(net):
    from splatam_amd import _capi
    a, b = (torch.from_numpy(t).cuda() for t in lpips_ref.image_pair(83, 61, 7))
    assert float(net(a, a).cpu()) == 0.0
    first, second = net(a, b).clone(), net(a, b).clone()
    assert float(first.cpu()) > 0 and torch.equal(first, second) and first.dtype == torch.float64 and first.dim() == 0
    # a frame whose every pixel is masked (no depth anywhere; and, with the silhouette variant, no presence anywhere)
    sil, depth = torch.rand(61, 83, device="cuda"), torch.rand(1, 61, 83, device="cuda") + 0.5
    assert float(net.planes(a, sil, b, torch.zeros_like(depth), SIL_THRES, sil_mask=False).cpu()) == 0.0
    assert float(net.planes(a, torch.zeros_like(sil), b, depth, SIL_THRES, sil_mask=True).cpu()) == 0.0
    # ... and an unmasked one is the plain figure of the two images
    full = net.planes(a, torch.ones_like(sil), b, depth, SIL_THRES, sil_mask=True)
    assert torch.equal(full, first)
    # 30 x 40 is refused before any launch
    with pytest.raises(ValueError, match="31"):
        net(torch.zeros(3, 30, 40, device="cuda"), torch.zeros(3, 30, 40, device="cuda"))
    arrays = (_capi.SplatArrayInfo * 16)()
    assert _capi.lib().splat_lpips_workspace_layout(40, 30, arrays, 16, None) < 0
    ws, _ = net.workspace(83, 61)
    out = torch.full((), -1.0, dtype=torch.float64, device="cuda")
    assert _capi.lib().splat_lpips_images(40, 30, a.data_ptr(), a.data_ptr(), net.net.data_ptr(), ctypes.byref(ws), out.data_ptr(), None) != 0
    # ... and so is a workspace laid out for another size (203 x 131 images would overrun the 83 x 61 slab)
    big = torch.zeros(3, 131, 203, device="cuda")
    assert _capi.lib().splat_lpips_images(203, 131, big.data_ptr(), big.data_ptr(), net.net.data_ptr(), ctypes.byref(ws), out.data_ptr(), None) != 0
    assert float(out.cpu()) == -1.0
    # shapes are checked, not element counts: a [H, W, 3] image, or a second image of another shape, is no [3, H, W] image
    with pytest.raises((RuntimeError, ValueError)):
        net(a.permute(1, 2, 0).contiguous(), b.permute(1, 2, 0).contiguous())
    with pytest.raises(RuntimeError, match=r"im1 must be .*\[3, 61, 83\]"):
        net(a, b.reshape(3, 83, 61))
    with pytest.raises(RuntimeError, match="sil must be"):
        net.planes(a, sil.t().contiguous(), b, depth, SIL_THRES, sil_mask=True)


# ---------------------------------------------------------------------------------------------------------------- through the evaluation
def test_evaluate_fills_slot_7_without_another_host_read(weights, net):
    """With weights ``evaluate`` still enqueues everything between learning the lists and THE table read (torch's sync debug mode
    "error" where the build enforces it; the phases are recorded either way); slots 0..6 are bit for bit the rows without weights; the
    figure agrees with the torch mirror's within the chain tolerance, 1e-4 relative."""
    from splatam_amd import _capi, evaluation, slam
    from splatam_amd.fused import FusedEngine
    dataset, params = eval_ref.golden_case("cuda")
    args = (dataset, params, len(dataset), SIL_THRES, 0, False)
    plain = evaluation.evaluate(*args, eval_every=5)
    assert plain['lpips'] is None and 'avg_lpips' not in plain
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
            enforced = False
        except RuntimeError:
            enforced = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    orig_relearn, orig_read, orig_frame = FusedEngine.relearn_lists, evaluation._read_table, FusedEngine.evaluate_frame
    phases, tables = [], []

    def relearn(self, *a, **k):
        out = orig_relearn(self, *a, **k)
        phases.append("learnt")
        if enforced:
            torch.cuda.set_sync_debug_mode("error")
        return out

    def read(table):
        torch.cuda.set_sync_debug_mode("default")
        phases.append("read")
        tables.append(orig_read(table))
        return tables[-1]

    lp = {}

    def frame(self, curr_data, t, row, *a, **k):
        lp.setdefault('net', k.get('lpips'))
        return orig_frame(self, curr_data, t, row, *a, **k)
    FusedEngine.relearn_lists, evaluation._read_table, FusedEngine.evaluate_frame = relearn, read, frame
    try:
        got = evaluation.evaluate(*args, eval_every=5, lpips_weights=weights)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        FusedEngine.relearn_lists, evaluation._read_table, FusedEngine.evaluate_frame = orig_relearn, orig_read, orig_frame
    assert phases == ["learnt", "read"] and got['repeated'] == [] and got['frames'] == [0, 4, 9]
    assert lp['net'] is not None
    table = tables[0]
    assert table.shape == (3, _capi.SPLAT_EVAL_ROW) and np.array_equal(table[:, _capi.SPLAT_EVAL_LPIPS], got['lpips'])
    assert (got['lpips'] > 0).all() and np.isfinite(got['lpips']).all() and got['avg_lpips'] == float(got['lpips'].mean())
    for k in ('psnr', 'depth_rmse', 'depth_l1', 'ms_ssim', 'valid_pixels'):
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    # against the mirror's expressions (``slam.eval_frame_metrics`` with weights: what ``engine="mirror"`` puts into slot 7) on the drop-in
    # rasterizer's two renders, evaluated in float32 on the CPU: within the chain tolerance, 1e-4 relative.  (The two renderers' planes
    # differ by ~1e-6 per pixel, which moves the figure by ~1e-8 relative: profiles/lpips.md; the bound has four decades over that.)
    cam = slam.setup_camera(240, 176, dataset[0][2][:3, :3].cpu().numpy(), torch.linalg.inv(dataset[0][3]).cpu().numpy(), device="cuda")
    w2c = torch.linalg.inv(dataset[0][3]).cuda().float().contiguous()
    for i, t in enumerate(got['frames']):
        color, depth, _, _ = evaluation._frame(dataset, t)
        with torch.no_grad():
            p = {k: v.detach() for k, v in params.items()}
            tg = slam.transform_to_frame(p, t, gaussians_grad=False, camera_grad=False)
            ds, _, _ = slam.Renderer(raster_settings=cam)(**slam.transformed_params2depthplussilhouette(p, w2c, tg))
            im, _, _ = slam.Renderer(raster_settings=cam)(**slam.transformed_params2rendervar(p, tg))
            m = slam.eval_frame_metrics(im.cpu(), ds.cpu(), {'im': color.cpu(), 'depth': depth.cpu()}, SIL_THRES, True, with_ms_ssim=False,
                                        lpips_weights=weights)
        ka, tb = got['lpips'][i], float(m['lpips'])
        print(f"LPIPSEVAL frame {t}: fused {ka:.9f} mirror {tb:.9f} relative difference {abs(ka - tb) / tb:.3e}")
        assert abs(ka - tb) <= 1e-4 * tb


@pytest.mark.parametrize("sil_mask", [False, True])
def test_evaluate_frame_and_view_score_the_planes_they_rendered(net, sil_mask):
    """Slot 7 of ``evaluate_frame`` / ``evaluate_view`` is, bit for bit, ``Lpips.planes`` of the colour and SILHOUETTE planes the render
    left, with the call's own ``sil_thres`` / ``sil_mask`` -- and differs from what the depth plane in the silhouette's place, the other
    mask variant, or the frame before would give.  Slots 0..6 are the row without ``lpips``."""
    from splatam_amd import _capi
    from splatam_amd.fused import FusedEngine
    from tests.test_gpu_eval import _scene
    params, _, frame, cam = _scene()
    frame = dict(frame)
    depth = frame['depth'].clone()
    depth[:, :60, :80] = 0.0                                   # pixels without depth: the valid mask matters
    frame['depth'] = depth
    eng = FusedEngine(params, cam)
    eng.relearn_lists(frame, 1)
    eng.render(frame, 1)
    thres = float(torch.quantile(eng.rendered()[2].flatten()[::7], 0.3).cpu())     # a threshold the silhouette straddles: presence matters
    row, plain = (torch.full((8,), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
    eng.evaluate_frame(frame, 0, plain, thres, sil_mask=sil_mask, lpips=net)       # another pose first: stale planes would show
    eng.evaluate_frame(frame, 1, plain, thres, sil_mask=sil_mask)
    eng.evaluate_frame(frame, 1, row, thres, sil_mask=sil_mask, lpips=net)
    im, d, sil, _ = (t.clone() for t in eng.rendered())
    assert 0.02 < float((sil > thres).float().mean()) < 0.98
    want = net.planes(im, sil, frame['im'], frame['depth'], thres, sil_mask=sil_mask).clone()
    assert torch.equal(row[_capi.SPLAT_EVAL_LPIPS], want) and float(want.cpu()) > 0
    assert torch.equal(row[:7], plain[:7]) and float(plain[7].cpu()) == 0.0
    others = {'depth as silhouette': net.planes(im, d[0].contiguous(), frame['im'], frame['depth'], thres, sil_mask=True).clone(),
              'other mask variant': net.planes(im, sil, frame['im'], frame['depth'], thres, sil_mask=not sil_mask).clone(),
              'no depth mask': net.planes(im, sil, frame['im'], torch.ones_like(depth), thres, sil_mask=sil_mask).clone()}
    eng.render(frame, 0)
    im0, _, sil0, _ = eng.rendered()
    others['planes of pose 0'] = net.planes(im0.contiguous(), sil0.contiguous(), frame['im'], frame['depth'], thres, sil_mask=sil_mask).clone()
    for name, v in others.items():
        print(f"LPIPSPLANES sil_mask={int(sil_mask)} {name}: {float(v.cpu()):.9f} (the frame's: {float(want.cpu()):.9f})")
        if name == 'depth as silhouette' and not sil_mask:
            continue                                           # (without sil_mask the silhouette is not read at all)
        assert not torch.equal(v, want), name
    # evaluate_view at the same pose
    view = eng.view_camera(eng.W, eng.H)
    k = torch.tensor([[0.5 * eng.W, 0, eng.W / 2 - 0.5], [0, 0.5 * eng.W, eng.H / 2 - 0.5], [0, 0, 1]])
    data = dict(frame, intrinsics=frame.get('intrinsics', k))
    w2c = frame['w2c'].float().contiguous()
    vrow = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    img = eng.evaluate_view(view, w2c, data, vrow, thres, sil_mask=sil_mask, lpips=net)
    o = img.out6
    want_v = net.planes(o[0:3].clone(), o[4].clone(), frame['im'], frame['depth'], thres, sil_mask=sil_mask).clone()
    assert torch.equal(vrow[_capi.SPLAT_EVAL_LPIPS], want_v) and float(want_v.cpu()) > 0


def test_evaluate_frame_without_weights_leaves_slot_7_zero_and_a_flagged_row_is_recomputed(weights):
    from splatam_amd import _capi, evaluation
    from splatam_amd.fused import FusedEngine
    dataset, params = eval_ref.golden_case("cuda")
    args = (dataset, params, len(dataset), SIL_THRES, 0, False)
    want = evaluation.evaluate(*args, eval_every=5, lpips_weights=weights)
    orig = FusedEngine.relearn_lists
    calls = []

    def relearn(self, *a, **k):
        orig(self, *a, **k)
        calls.append(self.tile_stride)
        if len(calls) == 1:
            self.tile_stride = 16
    FusedEngine.relearn_lists = relearn
    try:
        got = evaluation.evaluate(*args, eval_every=5, lpips_weights=weights)
    finally:
        FusedEngine.relearn_lists = orig
    assert got['repeated'] == [0, 4, 9]
    np.testing.assert_allclose(got['lpips'], want['lpips'], rtol=1e-10)
    # evaluate_frame alone: slot 7 is 0 without ``lpips``
    from tests.test_gpu_eval import _scene
    scene_params, _, frame, cam = _scene()
    eng = FusedEngine(scene_params, cam)
    eng.relearn_lists(frame, 1)
    row = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    eng.evaluate_frame(frame, 1, row, SIL_THRES)
    assert float(row[_capi.SPLAT_EVAL_LPIPS].cpu()) == 0.0


def test_novel_views_average_over_the_valid_frames(weights):
    from splatam_amd import evaluation
    chosen = None
    for cand in nvs_ref.CASES:              # a case with both valid and invalid frames, if the recordings have one
        dataset, params, (mapping_iters, add_new), every = nvs_ref.case(cand, "cuda")
        plain = evaluation.evaluate_novel_views(dataset, params, len(dataset), SIL_THRES, mapping_iters, add_new, eval_every=every)
        if plain['valid_nvs_frames'].any() and not plain['valid_nvs_frames'].all():
            chosen = (cand, dataset, params, mapping_iters, add_new, every, plain)
            break
    assert chosen is not None, "no recorded case mixes valid and invalid novel views"
    name, dataset, params, mapping_iters, add_new, every, plain = chosen
    got = evaluation.evaluate_novel_views(dataset, params, len(dataset), SIL_THRES, mapping_iters, add_new, eval_every=every, lpips_weights=weights)
    valid = got['valid_nvs_frames']
    assert plain['lpips'] is None and got['lpips'].shape == valid.shape and (got['lpips'] > 0).all()
    assert got['avg_lpips'] == float(got['lpips'][valid].mean()) and got['avg_lpips'] != float(got['lpips'].mean())
    for k in ('psnr', 'depth_l1', 'ms_ssim', 'holes'):
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    print(f"LPIPSNVS {name}: lpips {np.round(got['lpips'], 6).tolist()} valid {valid.tolist()} avg {got['avg_lpips']:.6f}")


# ---------------------------------------------------------------------------------------------------------------- the command lines
def test_run_prints_an_lpips_average_with_weights(weights, tmp_path, capsys):
    """``python -m splatam_amd.run CONFIG.py --lpips-weights W`` (in this process: ``run.main``) on a three-frame ReplicaV2-layout
    sequence written here: the evaluation reports ``Average LPIPS: 0.xxx``; without the flag no such line is printed."""
    import dataset_files as files
    from splatam_amd import lpips, pipeline, run
    W, H, F, SCALE, FRAMES = 160, 112, 140.0, 6553.5, 3
    root = str(tmp_path / "sequence")
    ds = pipeline.SyntheticRGBDSequence(6000, W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, num_frames=FRAMES, seed=2, step_m=0.012, step_deg=0.4)
    frames, poses = [], []
    for t in range(FRAMES):
        color, depth, _, pose = ds[t]
        frames.append((np.rint(color.cpu().numpy()).clip(0, 255).astype(np.uint8),
                       np.rint(depth.cpu().numpy()[..., 0].astype(np.float64) * SCALE).astype(np.uint16)))
        poses.append(pose.cpu().numpy())
    files.write_replica_v2(root, "room0", frames, np.stack(poses))
    yaml_path = str(tmp_path / "synthetic.yaml")
    with open(yaml_path, "w") as f:
        f.write(f"dataset_name: 'replicav2'\ncamera_params:\n  image_height: {H}\n  image_width: {W}\n  fx: {F}\n  fy: {F}\n"
                f"  cx: {W / 2 - 0.5}\n  cy: {H / 2 - 0.5}\n  png_depth_scale: {SCALE}\n")
    cfg = pipeline.replica_config(tracking_iters=6, mapping_iters=10, keyframe_every=2)
    cfg.update(workdir=str(tmp_path / "experiments"), run_name="room0_0", seed=0, primary_device="cuda:0", eval_every=1,
               report_global_progress_every=500, report_iter_progress=False, load_checkpoint=False, save_checkpoints=False, use_wandb=False,
               data=dict(basedir=root, gradslam_data_cfg=yaml_path, sequence="room0", desired_image_height=H, desired_image_width=W,
                         start=0, end=-1, stride=1, num_frames=FRAMES))
    path = str(tmp_path / "experiment.py")
    with open(path, "w") as f:
        f.write("config = " + repr(cfg) + "\n")
    npz = str(tmp_path / "weights.npz")
    lpips.save_weights_npz(weights, npz)
    run.main([path, "--lpips-weights", npz])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("Average LPIPS: ")]
    assert len(line) == 1 and "Average PSNR" in out
    value = line[0][len("Average LPIPS: "):]
    assert len(value.split(".")[1]) == 3 and 0.0 <= float(value) < 2.0          # three decimals, as the reference prints
    run.main([path])
    assert "LPIPS" not in capsys.readouterr().out


def test_two_pictures_from_the_command_line(weights, tmp_path, capsys):
    from PIL import Image
    from splatam_amd import lpips
    a, b = lpips_ref.image_pair(97, 45, 3)
    paths = []
    for name, im in (("a.png", a), ("b.png", b)):
        paths.append(str(tmp_path / name))
        Image.fromarray(np.rint(im.transpose(1, 2, 0) * 255).astype(np.uint8)).save(paths[-1])
    npz = str(tmp_path / "weights.npz")
    lpips.save_weights_npz(weights, npz)
    on_device = lpips.main(paths + ["--weights", npz])
    on_cpu = lpips.main(paths + ["--weights", npz, "--device", "cpu"])
    out = capsys.readouterr().out
    assert out.count("LPIPS: ") == 2 and on_device > 0.01
    assert abs(on_device - on_cpu) <= 2e-4 * on_cpu                             # two float32 forms of the chain, 1e-4 each against float64
