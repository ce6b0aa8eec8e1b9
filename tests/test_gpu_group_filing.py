"""Group binning files the right records, whatever the frame and the map size (splat_device.h GROUP BINNING: F1 of the fused
iteration, K1 of the drop-in path).  The per-Gaussian kernel writes one 16-byte record (Gaussian id, depth bits, tile rectangle) per
2 x 2-tile group the rectangle touches; the slots come from the groups' live counters, which sixteen consecutive groups share 64
bytes of, and which a workgroup of 512 Gaussians reserves from once per non-empty group.

The records are checked against THEMSELVES: a record's own rectangle says which groups must hold a copy of it.  Then: the image is
bit-identical to the per-tile-bucket engine's (the composite sorts by (depth, id), so the order in a bucket reaches no result), loss
and gradients agree within the bounds of test_gpu_fused.py::test_group_binning_changes_nothing_but_speed (1e-6 relative, 2e-5 of
the maximum), and a bucket that is too small raises the overflow flag and holds the Adam step back."""
import pytest
import torch

from tests.test_gpu_fused import _scene

pytestmark = pytest.mark.gpu

GROUP_PER_LANE = 4          # kGroupPerLane, splat_device.h: a Gaussian's groups beyond these take their own atomics


def _scene_in_and_around(P, W, H, aniso, seed):
    """_scene of test_gpu_fused.py with a map of P Gaussians of which at most ~100 per tile project into the frame, the rest around it:
    group binning needs per-tile lists short enough for the composite's own sort (splat_device.h lists_sorted_by_composite: 819
    entries), which 8 000 or 30 001 Gaussians INSIDE a frame of six tiles cannot have.  The per-Gaussian kernel sees all P either way."""
    from splatam_amd import slam
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    if P <= 100 * tiles:
        return _scene(P, W, H, aniso=aniso, seed=seed)
    k = 0.5 * ((P / (100.0 * tiles)) ** 0.5 - 1.0)          # the window grows by k frames on every side
    f = 0.5 * W
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    params, variables = slam.synthetic_params(P, W, H, f, f, cx, cy, num_frames=3, seed=seed, device="cuda", anisotropic=aniso,
                                              region=(-k, -k, 1.0 + k, 1.0 + k))
    w2c = torch.eye(4, device="cuda")
    cam = slam.setup_camera(W, H, [[f, 0, cx], [0, f, cy], [0, 0, 1]], w2c.cpu().numpy(), device="cuda")
    im, depth = slam.synthetic_frame(params, cam, w2c, 1, rot_deg=0.4, trans_m=0.01)
    frame = {'cam': cam, 'im': im.contiguous(), 'depth': depth.contiguous(), 'id': 1, 'w2c': w2c}
    return params, variables, frame, cam


def _groups(W, H):
    ggx, ggy = ((W + 15) // 16 + 1) // 2, ((H + 15) // 16 + 1) // 2
    return ggx, ggx * ggy


def _check_records(recs, counts, W, H, P, depth=None, radii=None):
    """recs [G, stride, 4] int32 and counts [G] (CPU tensors): every Gaussian that has a record is in every group its rectangle
    touches exactly once and in no other group.  Returns (records, Gaussians filed, most groups one Gaussian touches)."""
    ggx, G = _groups(W, H)
    assert recs.shape[0] == G and counts.shape[0] == G
    stride = recs.shape[1]
    assert int(counts.min()) >= 0 and int(counts.max()) <= stride
    g_idx, s_idx = (torch.arange(stride)[None, :] < counts[:, None]).nonzero(as_tuple=True)
    r = recs[g_idx, s_idx].long() & 0xFFFFFFFF
    if r.shape[0] == 0:
        return 0, 0, 0
    ids = r[:, 0]
    x0, y0, x1, y1 = r[:, 2] & 0xFFFF, r[:, 2] >> 16, r[:, 3] & 0xFFFF, r[:, 3] >> 16
    assert int(ids.max()) < P
    assert bool((x1 > x0).all()) and bool((y1 > y0).all())                      # a non-empty rectangle ...
    assert int(x1.max()) <= (W + 15) // 16 and int(y1.max()) <= (H + 15) // 16  # ... of tiles of the frame
    gx0, gy0, gx1, gy1 = x0 >> 1, y0 >> 1, (x1 - 1) >> 1, (y1 - 1) >> 1
    gx, gy = g_idx % ggx, g_idx // ggx
    assert bool(((gx >= gx0) & (gx <= gx1) & (gy >= gy0) & (gy <= gy1)).all()), "a record in a group its rectangle does not touch"
    pair = ids * G + g_idx
    assert torch.unique(pair).numel() == pair.numel(), "a Gaussian twice in one group"
    # all copies of a Gaussian's record are the same words
    first = torch.zeros(P, 3, dtype=torch.long)
    first[ids] = r[:, 1:]
    assert bool((first[ids] == r[:, 1:]).all()), "copies of one Gaussian's record differ"
    touched = (gx1 - gx0 + 1) * (gy1 - gy0 + 1)
    copies = torch.bincount(ids, minlength=P)
    assert bool((copies[ids] == touched).all()), "a Gaussian is missing from a group its rectangle touches"
    if depth is not None:
        assert bool((r[:, 1] == (depth.view(torch.int32).long() & 0xFFFFFFFF)[ids]).all())
    if radii is not None:
        assert bool((radii[ids] > 0).all())
    return int(r.shape[0]), int((copies > 0).sum()), int(touched.max())


def _engine_records(eng, W, H):
    """(records, kept counts) after an iteration; the counter lines are as the iteration leaves them: word 1 the group's count, the
    rest zero."""
    from splatam_amd import _capi
    ws = eng._workspace(False, with_ssim=False)
    gs = int(ws.st.group_stride)
    assert gs > 0
    _, G = _groups(W, H)
    assert G == eng.num_groups
    gc = eng.buf['group_count'].view(-1, _capi.SPLAT_COUNTER_STRIDE).cpu()
    assert gc.shape[0] == G
    assert int(gc[:, 0].abs().max()) == 0 and int(gc[:, 2:].abs().max()) == 0
    recs = eng.buf['group_recs'][:G * gs * 4].view(G, gs, 4).cpu()
    return recs, gc[:, 1].long()


def _run_pair(params, frame, cam, W, H, tracking=False):
    """One learnt iteration with per-tile buckets and one with group binning; returns the group engine and both results."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    cfg = slam.REPLICA_TRACKING if tracking else slam.REPLICA_MAPPING
    outs, engines = [], []
    for groups in (False, True):
        eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
        eng.group_bins = groups
        for attempt in range(4):
            eng.loss_backward(frame, 1, cfg, tracking=tracking)
            if not eng.check_overflow():
                break
        assert eng.tile_stride > 0
        eng.loss_backward(frame, 1, cfg, tracking=tracking)
        torch.cuda.synchronize()
        assert not eng.check_overflow(grow=False)
        ws = eng._workspace(False, with_ssim=False)
        assert (ws.st.group_stride > 0) == groups
        outs.append((eng.buf['out6'].clone(), eng.grads['means3D'].clone(), eng.loss()))
        engines.append(eng)
    return engines[1], outs


def _assert_same_results(outs):
    assert torch.equal(outs[0][0], outs[1][0])
    assert abs(outs[0][2] - outs[1][2]) <= 1e-6 * abs(outs[0][2])
    assert float((outs[0][1] - outs[1][1]).abs().max()) <= 2e-5 * float(outs[0][1].abs().max())


@pytest.mark.parametrize("aniso", [False, True])
@pytest.mark.parametrize("P", [1, 511, 513, 8000, 30001])
@pytest.mark.parametrize("W,H", [(1200, 680), (1232, 720), (208, 160), (48, 32)])
def test_fused_iteration_files_every_record_once(W, H, P, aniso):
    """836 groups, 897 groups (not a multiple of 16 or 64: the last half line of live counters is partly used), 35 and 2 groups; maps
    of less than one workgroup, one Gaussian more than one, and several (the large maps on the small frames: _scene_in_and_around)."""
    params, variables, frame, cam = _scene_in_and_around(P, W, H, aniso, seed=41)
    eng, outs = _run_pair(params, frame, cam, W, H)
    recs, counts = _engine_records(eng, W, H)
    n_recs, n_filed, _ = _check_records(recs, counts, W, H, P, depth=eng.buf['depth'][:P].cpu(), radii=eng.buf['radii'][:P].cpu())
    print(f"{W}x{H} P={P} aniso={aniso}: {n_recs} records of {n_filed} Gaussians in {counts.numel()} groups, fullest {int(counts.max())}")
    assert n_filed > 0 and n_recs >= n_filed
    _assert_same_results(outs)


def test_a_map_of_the_flagship_size_files_every_record_once():
    """300 007 Gaussians on 1200 x 680 (workload B's shape): 586 workgroups contend for every group's counter, the last one is mostly
    past the end of the map."""
    W, H, P = 1200, 680, 300007
    params, variables, frame, cam = _scene(P, W, H, seed=43)
    eng, outs = _run_pair(params, frame, cam, W, H)
    recs, counts = _engine_records(eng, W, H)
    n_recs, n_filed, _ = _check_records(recs, counts, W, H, P, depth=eng.buf['depth'][:P].cpu(), radii=eng.buf['radii'][:P].cpu())
    print(f"{W}x{H} P={P}: {n_recs} records of {n_filed} Gaussians in {counts.numel()} groups, fullest {int(counts.max())}")
    assert n_filed > P // 2
    _assert_same_results(outs)


def test_wide_splats_file_their_further_groups_through_their_own_atomics():
    """Splats wide enough to touch more than kGroupPerLane groups: the records beyond the histogram's reserve on the same live counter."""
    W, H = 320, 240
    params, variables, frame, cam = _scene(6000, W, H, seed=37)
    with torch.no_grad():
        params['log_scales'] += 1.5
    eng, outs = _run_pair(params, frame, cam, W, H)
    recs, counts = _engine_records(eng, W, H)
    n_recs, n_filed, most = _check_records(recs, counts, W, H, 6000, depth=eng.buf['depth'][:6000].cpu(), radii=eng.buf['radii'][:6000].cpu())
    print(f"wide splats: {n_recs} records of {n_filed} Gaussians, up to {most} groups per Gaussian")
    assert most > GROUP_PER_LANE
    _assert_same_results(outs)


def test_a_full_group_bucket_raises_the_overflow_flag_and_gates_adam():
    """Group buckets forced far too small (group_stride = 4 x tile_stride): the records that do not fit raise
    status[SPLAT_STATUS_OVERFLOW], the iteration takes no Adam step and is counted, and the loop recovers on exact lists."""
    from splatam_amd import _capi, slam
    from splatam_amd.fused import FusedEngine
    W, H = 208, 160
    params, variables, frame, cam = _scene(8000, W, H, seed=11)
    p = {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}
    eng = FusedEngine(p, cam)
    cfg = slam.REPLICA_MAPPING
    for _ in range(2):
        eng.mapping_iteration(frame, 1, cfg)
        assert not eng.check_overflow()
    assert eng.tile_stride > 0
    recs, counts = _engine_records(eng, W, H)
    assert int(counts.max()) > 4 * 16                           # the groups hold more than the small buckets below
    snap = {k: v.detach().clone() for k, v in p.items()}
    eng.tile_stride, eng.max_list_hint = 16, 10
    eng.mapping_iteration(frame, 1, cfg)
    torch.cuda.synchronize()
    ws = eng._workspace(False, with_ssim=False)
    assert int(ws.st.group_stride) == 4 * 16
    rep = eng.buf['d_cam'].cpu()
    assert float(rep[_capi.SPLAT_REPORT_FLAG]) == 1.0 and int(rep.view(torch.int32)[_capi.SPLAT_REPORT_SKIPPED]) == 1
    assert int(rep.view(torch.int32)[_capi.SPLAT_REPORT_STATUS + _capi.SPLAT_STATUS_OVERFLOW]) == 1      # the status snapshot: overflow
    for k in snap:
        assert torch.equal(p[k].detach(), snap[k]), k
    steps_before = eng.map_step - 1                                 # (the gated iteration advanced the host-side count)
    assert eng.settle("map") == 1 and eng.skipped_iterations == 1 and eng.tile_stride == 0
    assert eng.map_step == steps_before == 2
    eng.mapping_iteration(frame, 1, cfg)
    assert eng.settle("map") == 0 and eng.map_step == steps_before + 1
    assert not torch.equal(p['means3D'].detach(), snap['means3D'])


def _live_counter_word(g, line_words):
    """Word of SplatState.group_count that holds group g's live counter (include/splat_hip.h: sixteen consecutive groups in the upper
    64 bytes of line g / 16).  The drop-in path reads its records right after the forward pass, before anything folds the counters."""
    return (g // 16) * line_words + (line_words - 16) + g % 16


@pytest.mark.parametrize("W,H,n", [(1200, 680, 30001), (1232, 720, 8000), (208, 160, 513), (48, 32, 511)])
def test_dropin_rasterizer_files_every_record_once(W, H, n):
    """K1 with group binning behind the reference API ("auto" sync mode: a scene's second call): the same invariants on the records
    the forward pass left, and the same image as the first call's exact lists."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings as Camera
    from oracle import raster_ref as R
    from splatam_amd import _capi
    from splatam_amd import rasterizer as rz
    f = 0.5 * W
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    cam = R.make_camera(W, H, f, f, cx, cy)
    rv = R.cloud_to_rendervar(R.synthetic_cloud(n, W, H, f, f, cx, cy, seed=3))
    cs = Camera(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=cam.bg.cuda(), scale_modifier=1.0,
                viewmatrix=cam.viewmatrix.cuda(), projmatrix=cam.projmatrix.cuda(), sh_degree=0, campos=cam.campos.cuda(), prefiltered=False)
    inp = {k: v.cuda().contiguous() for k, v in rv.items()}
    none = torch.empty(0, device="cuda")
    args = (cs, inp['means3D'], inp['colors_precomp'], inp['opacities'], inp['scales'], inp['rotations'], none, none, inp['means3D'])
    assert rz._SYNC_MODE == "auto"
    color0, radii0, depth0, _ = rz._rasterize_forward_once(*args, will_backward=False)
    n_fast = rz.fast_path_stats["fast"]
    color1, radii1, depth1, pk = rz._rasterize_forward_once(*args, will_backward=False)
    torch.cuda.synchronize()
    assert rz.fast_path_stats["fast"] == n_fast + 1 and not rz.fast_call_flagged(pk)
    assert torch.equal(color0, color1) and torch.equal(depth0, depth1) and torch.equal(radii0, radii1)
    ggx, G = _groups(W, H)
    gs, CS = int(pk.st.group_stride), _capi.SPLAT_COUNTER_STRIDE
    slab = pk.tensors['geom']
    words = slab.view(torch.int32)
    c0 = (int(pk.st.group_count) - slab.data_ptr()) // 4
    r0 = (int(pk.st.group_recs) - slab.data_ptr()) // 4
    gc = words[c0:c0 + G * CS].cpu()
    live = torch.tensor([_live_counter_word(g, CS) for g in range(G)])
    counts = gc[live].long()
    rest = gc.clone()
    rest[live] = 0
    assert int(rest.abs().max()) == 0                           # nothing but the live counters is written
    recs = words[r0:r0 + G * gs * 4].view(G, gs, 4).cpu()
    n_recs, n_filed, _ = _check_records(recs, counts, W, H, n, radii=radii1.cpu())
    print(f"drop-in {W}x{H} P={n}: {n_recs} records of {n_filed} Gaussians, fullest group {int(counts.max())}")
    assert n_filed > 0


def test_timing_helper_replays_the_kept_counts_and_leaves_the_counters_clean():
    """splat_iter_time_kernel fn 2 / 3 (the sorting forward composite outside an iteration) sets the live counters from the kept
    counts for its launches and zeroes them again: the image is the iteration's, the counter lines are as the iteration left them,
    and the next iteration files into empty counters."""
    import ctypes as C
    from splatam_amd import _capi, slam
    from splatam_amd.fused import FusedEngine
    W, H, P = 328, 232, 30000
    params, variables, frame, cam = _scene(P, W, H, seed=37)
    eng = FusedEngine({k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}, cam)
    cfg = slam.REPLICA_MAPPING
    for _ in range(3):
        eng.loss_backward(frame, 1, cfg, tracking=False)
        assert not eng.check_overflow()
    torch.cuda.synchronize()
    ws = eng._workspace(False, with_ssim=False)
    assert ws.st.group_stride > 0
    out6 = eng.buf['out6'].clone()
    recs, counts = _engine_records(eng, W, H)
    for fn in (2, 3):
        ms = C.c_float(0)
        eng.buf['out6'].zero_()
        _capi.check(eng.L.splat_iter_time_kernel(fn, 3, C.byref(eng._cam), eng.P, C.byref(ws), eng._stream(), C.byref(ms)), "time")
        torch.cuda.synchronize()
        assert ms.value > 0.0
        assert torch.equal(eng.buf['out6'], out6)
        _, counts_after = _engine_records(eng, W, H)              # (asserts that every word but word 1 is zero)
        assert torch.equal(counts_after, counts)
    eng.loss_backward(frame, 1, cfg, tracking=False)
    torch.cuda.synchronize()
    assert not eng.check_overflow(grow=False)
    assert torch.equal(eng.buf['out6'], out6)
    _, counts_next = _engine_records(eng, W, H)
    assert torch.equal(counts_next, counts)
