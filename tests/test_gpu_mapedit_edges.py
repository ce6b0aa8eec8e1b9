"""The map-edit kernels (splatam_amd/csrc/mapedit.hip through FusedEngine.add_new_gaussians / add_valid_depth_points /
remove_points / prune_gaussians / densify) at the block and scan edges: the cases of tests/mapedit_cases.py, against

 * the torch formulations of splatam_amd/slam.py for everything discrete (which rows exist, in what order, how many) -- pinned to the
   reference's own code by tests/test_mapedit_mirror.py and to float64 statements on these very cases by
   tests/test_mapedit_cases_cpu.py;
 * the float64 statements of tests/mapedit_cases.py for the values the kernels compute (back-projected means3D, log_scales of new
   rows, the split's means3D and log_scales): rtol = atol = 2e-6, and 2e-6 max(1, |ref|max) for the split, as in
   tests/test_gpu_mapedit.py.  Copied values -- pruned and cloned rows, colours, rotations, timestep, Adam moments, zeroed fields --
   are bit for bit.

What each group of cases would catch (read off mapedit.hip, not tried on the device):
 * dropping ``carry`` between the chunks of scan_blocks_kernel / densify_scan_kernel: every case at 262145 rows and more (513x512
   pixels) with rows selected on BOTH sides of workgroup 256 -- "all", "random50", "all_but_one_per_group", "last_of_64", ... (the rows
   of workgroup 256 land on row 0); "first_256_groups" through the totals.  In "after_256_groups" the carry itself is 0: what it
   notices is a scan that never reaches its second chunk (workgroup 256 keeps its raw count as its offset).  The model of
   tests/test_mapedit_cases_cpu.py::test_the_targeted_cases_tell_a_defect_from_sound_code states which case notices which defect;
 * an off-by-one in the ballot rank (``m & ((1 << lane) - 1)``) or in the wave offsets: "last_of_64" / "last_of_256" (the one selected
   lane of a wave is its last: any rank other than 0 moves the row), "all_but_one_per_group", "random50";
 * a round's ``base += tot`` or the workgroup's offset: "last_of_1024", "first_of_1024", "one_full_group";
 * the upper instead of the lower median: "two_lower" / "half_zero" at even HW; a rank lost between the radix passes: "bits_low" /
   "bits_mid" / "bits_high" (all the variation inside one pass);
 * the NaN counter (or any scratch word) left uncleared: the back-to-back medians, NaN plane first;
 * skipping the variable reset when nothing is appended: "invalid_selected" (counts[3] > 0, no row);
 * an append, clone or split that handles ``rows == capacity`` as a miss, or loses rows over a re-allocation: the capacity cases.
"""
import numpy as np
import pytest
import torch

from tests import mapedit_cases as mc
from tests.mapedit_cases import GAUSSIAN_KEYS, VAR_KEYS
from tests.test_mapedit_cases_cpu import (_id, assert_rows, draw_normals, frame_data, mirror_add, mirror_densify, mirror_result,
                                          make_mirror, mirror_valid_depth, prune_dict)

pytestmark = pytest.mark.gpu


def _dummy_cam(W, H, f=50.0):
    from splatam_amd import slam
    k = [[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]]
    return slam.setup_camera(W, H, k, np.eye(4, dtype=np.float32), device="cuda")


def make_engine(st, capacity, W=64, H=48):
    """A FusedEngine that owns the case's map: parameters, both moments and the four variables as the case gives them."""
    from splatam_amd.fused import FusedEngine
    params = {k: torch.nn.Parameter(st['params'][k].clone().cuda().contiguous()) for k in GAUSSIAN_KEYS}
    if 'cam_unnorm_rots' in st['params']:
        for k in ('cam_unnorm_rots', 'cam_trans'):
            params[k] = torch.nn.Parameter(st['params'][k].clone().cuda().contiguous())
    else:
        rots = torch.zeros(1, 4, mc.NUM_FRAMES, device="cuda")
        rots[:, 0, :] = 1.0
        params['cam_unnorm_rots'] = torch.nn.Parameter(rots)
        params['cam_trans'] = torch.nn.Parameter(torch.zeros(1, 3, mc.NUM_FRAMES, device="cuda"))
    variables = {k: st['variables'][k].clone().cuda() for k in VAR_KEYS}
    eng = FusedEngine(params, _dummy_cam(W, H), gaussian_capacity=capacity, variables=variables)
    for k in GAUSSIAN_KEYS:
        eng.exp_avg[k].copy_(st['exp_avg'][k].cuda())
        eng.exp_avg_sq[k].copy_(st['exp_avg_sq'][k].cuda())
    return eng, params, variables


def engine_result(eng, params, variables):
    torch.cuda.synchronize()
    return {'params': {k: params[k].detach().cpu().numpy() for k in GAUSSIAN_KEYS},
            'variables': {k: variables[k].cpu().numpy() for k in VAR_KEYS},
            'exp_avg': {k: eng.exp_avg[k].cpu().numpy() for k in GAUSSIAN_KEYS},
            'exp_avg_sq': {k: eng.exp_avg_sq[k].cpu().numpy() for k in GAUSSIAN_KEYS}}


def assert_identical(a, b):
    for g in ('params', 'variables', 'exp_avg', 'exp_avg_sq'):
        for k in a[g]:
            np.testing.assert_array_equal(a[g][k], b[g][k], err_msg=f"{g}/{k}")


def assert_discrete_as_mirror(got, ref):
    """Against the torch formulation: the same rows in the same order (copied fields equal bit for bit), the variables equal."""
    for k in GAUSSIAN_KEYS:
        assert got['params'][k].shape == ref['params'][k].shape, k
    for k in ('rgb_colors', 'unnorm_rotations', 'logit_opacities'):
        np.testing.assert_array_equal(got['params'][k], ref['params'][k], err_msg=k)
    for k in VAR_KEYS:
        np.testing.assert_array_equal(got['variables'][k], ref['variables'][k], err_msg=k)
    for m in ('exp_avg', 'exp_avg_sq'):
        if m in ref:
            for k in GAUSSIAN_KEYS:
                np.testing.assert_array_equal(got[m][k], ref[m][k], err_msg=f"{m}/{k}")


def median_word(eng):
    return np.frombuffer(np.int32(eng.buf['counts'][4].item()).tobytes(), dtype=np.float32)[0]


def same_float(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the median
# ---------------------------------------------------------------------------------------------------------------------
def _median_engine(W, H):
    frame, _ = mc.add_frame(W, H, "none", 1)
    eng, params, variables = make_engine(frame, mc.N0 + W * H, W, H)
    return eng, frame


def _median_of_plane(eng, frame, W, H, gt, rd):
    curr = frame_data(frame, "cuda")
    curr['depth'] = gt.reshape(1, H, W).cuda()
    depth_sil = torch.stack([rd.reshape(H, W), torch.ones(H, W)]).cuda()
    eng.add_new_gaussians(curr, mc.SIL_THRES, mc.TIME_IDX, "projective", "isotropic", depth_sil=depth_sil)
    torch.cuda.synchronize()
    return median_word(eng)


@pytest.mark.parametrize("case", mc.MEDIAN_CASES, ids=_id)
def test_median_is_torch_median_bit_for_bit(case):
    """counts[4] after add_new_gaussians == numpy.sort(err)[(HW - 1) // 2], NaN if any error is NaN (== torch.median on every plane:
    tests/test_mapedit_cases_cpu.py).  The upper median fails "two_lower" / "half_zero"; a histogram that drops the grid-stride tail
    fails 513x512 (1026 blocks of 256 against the cap of 1024)."""
    W, H, dist = case
    gt, rd, props = mc.median_plane(W, H, dist)
    eng, frame = _median_engine(W, H)
    got = _median_of_plane(eng, frame, W, H, gt, rd)
    assert same_float(got, props['expected']), (got, props['expected'])


@pytest.mark.parametrize("size", [(41, 25), (513, 512)], ids=_id)
@pytest.mark.parametrize("pair", [("nan_one", "two_lower"), ("zero_times_inf", "mostly_zero"), ("inf_majority", "bits_low")], ids=_id)
def test_medians_back_to_back_do_not_leak_scratch(size, pair):
    """Two planes one after the other on ONE engine, the NaN (or inf) plane first: the NaN counter, the prefix / rank words and the
    histogram are cleared between edits.  A NaN counter left standing makes the second median NaN."""
    W, H = size
    eng, frame = _median_engine(W, H)
    for dist in pair:
        gt, rd, props = mc.median_plane(W, H, dist)
        got = _median_of_plane(eng, frame, W, H, gt, rd)
        assert same_float(got, props['expected']), (dist, got, props['expected'])


# ---------------------------------------------------------------------------------------------------------------------
# append
# ---------------------------------------------------------------------------------------------------------------------
def _run_add(frame, capacity):
    eng, params, variables = make_engine(frame, capacity, frame['W'], frame['H'])
    dist = "isotropic" if frame['cols'] == 1 else "anisotropic"
    added = eng.add_new_gaussians(frame_data(frame, "cuda"), frame['sil_thres'], frame['time_idx'], "projective", dist,
                                  depth_sil=frame['depth_sil'].cuda())
    torch.cuda.synchronize()
    return eng, params, variables, added


@pytest.mark.parametrize("case", mc.ADD_CASES, ids=_id)
def test_add_new_gaussians_at_the_edges(case):
    """Every add frame against slam._add_from_render (rows, order, timestep, variable resets: exact) and the float64 back-projection
    (means3D, log_scales: 2e-6).  "invalid_selected": counts[3] > 0 with no row appended still zeroes the three variables of ALL rows;
    "none": map and variables untouched; the rule frames: selection by the depth rule alone, the silhouette alone, under a NaN
    median (silhouette only) and under a median of 0 (any rd > gt)."""
    frame, _ = mc.add_frame(*case)
    exp = mc.expected_add(frame)
    ref = mirror_add(frame)
    eng, params, variables, added = _run_add(frame, mc.N0 + exp['added'] + 5)
    counts = eng.buf['counts'].tolist()
    assert added == exp['added'] == ref['params']['means3D'].shape[0] - mc.N0 and eng.P == mc.N0 + added
    assert counts[3] == exp['non_presence'] and counts[2] == 0
    assert same_float(median_word(eng), exp['median'])
    got = engine_result(eng, params, variables)
    assert_discrete_as_mirror(got, ref)
    worst = assert_rows(got, exp)                               # (moments: the old rows' kept, the new rows' zero)
    print(f"add {_id(case)}: worst computed-value error {worst:.3g} (bound 2e-6 (1 + |ref|))")


@pytest.mark.parametrize("size", mc.PLANE_SIZES, ids=_id)
@pytest.mark.parametrize("n0", [0, mc.N0])
def test_add_valid_depth_points_at_the_edges(size, n0):
    """One Gaussian per pixel of depth > 0 under a world-to-camera transform that is not the identity, on an empty map and on one
    of N0 rows, against get_pointcloud(mask = depth > 0) + initialize_params and the float64 back-projection."""
    W, H = size
    cols = 1 if (W + n0) % 2 else 3
    frame = mc.valid_depth_frame(W, H, cols, n0)
    exp = mc.expected_valid_depth(frame)
    ref = mirror_valid_depth(frame)
    eng, params, variables = make_engine(frame, n0 + W * H, W, H)
    n = eng.add_valid_depth_points(frame['im'].cuda(), frame['depth'].cuda(), frame['intrinsics'], frame['w2c'].cuda())
    assert n == exp['added'] and eng.P == n0 + n
    got = engine_result(eng, params, variables)
    for k in ('rgb_colors', 'unnorm_rotations', 'logit_opacities'):
        np.testing.assert_array_equal(got['params'][k], ref['params'][k], err_msg=k)
    for k in VAR_KEYS:
        np.testing.assert_array_equal(got['variables'][k], ref['variables'][k], err_msg=k)
    worst = assert_rows(got, exp)
    print(f"valid-depth {W}x{H} on {n0} rows: worst computed-value error {worst:.3g} (bound 2e-6 (1 + |ref|))")


# ---------------------------------------------------------------------------------------------------------------------
# removal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.COMPACTION_CASES, ids=_id)
def test_remove_points_at_the_edges(case):
    """remove_points(~keep): parameters, both moments and all four variables == x[keep] bit for bit, for every kept (size, pattern).
    The patterns put the kept rows on the last lane of a wave, the last / first row of a round and of a workgroup, and (262145,
    263169 rows) on either side, or both sides, of the scan's first chunk of 256 workgroups."""
    n, pattern = case
    keep = mc.select_mask(n, pattern)
    st = mc.map_state(n, 1 + 2 * (n % 2), seed="remove")
    eng, params, variables = make_engine(st, n + 3)
    removed = eng.remove_points(torch.from_numpy(~keep).cuda())
    assert removed == int((~keep).sum()) and eng.P == int(keep.sum())
    assert_rows(engine_result(eng, params, variables), mc.compacted(st, keep))


@pytest.mark.parametrize("cols", [1, 3])
def test_a_map_pruned_to_zero_rows_grows_again(cols):
    """"All removed" leaves P == 0; add_valid_depth_points on that engine then gives the same map as on a fresh empty engine (stale
    rows, moments and variables beyond P do not come back)."""
    W, H = 41, 25
    frame = mc.valid_depth_frame(W, H, cols, mc.N0)
    eng, params, variables = make_engine(frame, mc.N0 + W * H, W, H)
    assert eng.remove_points(torch.ones(mc.N0, dtype=torch.bool, device="cuda")) == mc.N0 and eng.P == 0
    assert params['means3D'].shape[0] == 0 and variables['timestep'].shape[0] == 0
    assert eng.remove_points(torch.zeros(0, dtype=torch.bool, device="cuda")) == 0
    args = (frame['im'].cuda(), frame['depth'].cuda(), frame['intrinsics'], frame['w2c'].cuda())
    n = eng.add_valid_depth_points(*args)
    emptied = engine_result(eng, params, variables)
    fresh_frame = mc.valid_depth_frame(W, H, cols, 0)
    fresh, fparams, fvariables = make_engine(fresh_frame, W * H, W, H)
    assert fresh.add_valid_depth_points(*args) == n == int((frame['depth'] > 0).sum())
    assert_identical(emptied, engine_result(fresh, fparams, fvariables))


@pytest.mark.parametrize("case", mc.PRUNE_CASES, ids=_id)
def test_prune_gaussians_by_its_own_rules(case):
    """prune_gaussians forming the flags on the device -- opacity alone, opacity with the size rule, anisotropic (the largest of three
    columns decides) -- against slam.prune_gaussians on a real Adam and the float64 rules, at 1025 and 262145 rows."""
    from splatam_amd import slam
    n, rule = case
    st = mc.prune_state(n, rule)
    remove_big = rule != "opacity"
    rem = mc.expected_prune(st, remove_big)
    mparams, mvars, opt = make_mirror(st, "cuda")
    mvars['scene_radius'] = torch.tensor(mc.PRUNE_RADIUS, device="cuda")
    mparams, mvars = slam.prune_gaussians(mparams, mvars, opt, 0, prune_dict(remove_big))
    ref = mirror_result(mparams, mvars, opt)
    eng, params, variables = make_engine(st, n)
    removed = eng.prune_gaussians(0, prune_dict(remove_big), mc.PRUNE_RADIUS)
    assert removed == int(rem.sum()) and eng.P == n - removed == ref['params']['means3D'].shape[0]
    got = engine_result(eng, params, variables)
    assert_identical(got, ref)
    assert_rows(got, mc.compacted(st, ~rem))


# ---------------------------------------------------------------------------------------------------------------------
# densify
# ---------------------------------------------------------------------------------------------------------------------
SEED = 1234


def _run_densify(st, capacity):
    eng, params, variables = make_engine(st, capacity)
    torch.manual_seed(SEED)
    changed = eng.densify(1, st['dict'], st['radius'], accumulate=False)
    return eng, params, variables, changed


@pytest.mark.parametrize("case", mc.DENSIFY_CASES, ids=_id)
def test_densify_at_the_edges(case):
    """densify(iter, dd, R, accumulate=False) against slam.densify, both on the GPU under the same torch.manual_seed, and against
    the float64 statement with the same standard-normal draws.  First the number of selected rows (so that the draws line up), then
    parameters within tolerance, moments and variables exact, and timestep of every new row == its SOURCE row's (stated on the
    sources: the reference's densify does not extend timestep).  "clone:<pattern>" / "split:<pattern>" put the selection of one
    step on the ballot, workgroup and scan-chunk boundaries of duplicate_rows_kernel / densify_scan_kernel; "thresh_0" selects the
    0 / 0 and zero-gradient rows and lets the fresh clones (beyond rows_with_grad, padded gradient 0) pass the gradient test."""
    n, kind = case
    st = mc.densify_state(n, kind)
    to_clone, to_split, _, _ = mc.densify_selection(st)
    n_split = st['dict']['num_to_split_into']
    exp = mc.expected_densify(st, draw_normals(n_split * int(to_split.sum()), SEED, "cuda"))
    ref = mirror_densify(st, SEED, "cuda")
    eng, params, variables, changed = _run_densify(st, exp['peak'] + 5)
    rows = exp['params']['means3D'].shape[0]
    assert changed and eng.P == rows == ref['params']['means3D'].shape[0], (eng.P, rows)
    got = engine_result(eng, params, variables)
    assert_discrete_as_mirror(got, ref)
    for k in ('means3D', 'log_scales'):
        r = ref['params'][k]
        assert rows == 0 or float(np.abs(got['params'][k] - r).max()) <= 2e-6 * max(1.0, float(np.abs(r).max())), k
    worst = assert_rows(got, exp, relative_to_max=True)
    print(f"densify {_id(case)}: worst computed-value error {worst:.3g} (bound 2e-6 max(1, |ref|max))")
    np.testing.assert_array_equal(got['variables']['timestep'], st['variables']['timestep'].numpy()[exp['source']])


# ---------------------------------------------------------------------------------------------------------------------
# capacity: an exact fit, a miss by one row, ample room
# ---------------------------------------------------------------------------------------------------------------------
def _remove_half_and_check(eng, params, variables):
    """One further edit after a growth: the re-allocated flags, staging and scratch buffers are the right size."""
    before = engine_result(eng, params, variables)
    keep = mc.select_mask(eng.P, "random50", seed="after growth")
    assert eng.remove_points(torch.from_numpy(~keep).cuda()) == int((~keep).sum())
    after = engine_result(eng, params, variables)
    for g in before:
        for k in before[g]:
            np.testing.assert_array_equal(after[g][k], before[g][k][keep], err_msg=f"{g}/{k}")


def test_append_at_exact_capacity_one_row_short_and_ample():
    """rows0 + added == capacity is a fit (Pcap unchanged, no retry); one row less grows the map once; all three leave bit-identical
    maps, moments and variables."""
    frame, _ = mc.add_frame(41, 25, "random50", 3)
    rows = mc.N0 + mc.expected_add(frame)['added']
    results = {}
    for room, cap in (("exact", rows), ("short", rows - 1), ("ample", rows + 1000)):
        eng, params, variables, added = _run_add(frame, cap)
        assert eng.P == rows
        assert eng.Pcap == cap if room != "short" else eng.Pcap > cap
        results[room] = engine_result(eng, params, variables)
        if room == "short":
            _remove_half_and_check(eng, params, variables)
    assert_identical(results["exact"], results["ample"])
    assert_identical(results["short"], results["ample"])


@pytest.mark.parametrize("kind", ["clone_only", "split_only"])
def test_clone_and_split_at_exact_capacity_one_row_short_and_ample(kind):
    st = mc.densify_state(1025, kind)
    to_clone, to_split, _, _ = mc.densify_selection(st)
    peak = 1025 + int(to_clone.sum()) + st['dict']['num_to_split_into'] * int(to_split.sum())
    results = {}
    for room, cap in (("exact", peak), ("short", peak - 1), ("ample", 4 * peak)):
        eng, params, variables, _ = _run_densify(st, cap)
        assert eng.Pcap == cap if room != "short" else eng.Pcap > cap
        results[room] = engine_result(eng, params, variables)
        if room == "short":
            _remove_half_and_check(eng, params, variables)
    assert_identical(results["exact"], results["ample"])
    assert_identical(results["short"], results["ample"])


def test_clone_grows_and_then_split_grows_again_in_one_densify():
    """Capacity one row short for the clones: the engine grows to 1.5 x; the split's rows do not fit into that either (checked on the
    state by tests/test_mapedit_cases_cpu.py) and it grows a second time, with the selection flags re-made in between."""
    st = mc.densify_state(2049, "double_growth")
    to_clone, to_split, _, _ = mc.densify_selection(st)
    C, S, n_split = int(to_clone.sum()), int(to_split.sum()), st['dict']['num_to_split_into']
    first = int((2049 + C) * 1.5) + 1024
    assert C > 0 and 2049 + C + n_split * S > first
    eng, params, variables, _ = _run_densify(st, 2049 + C - 1)
    assert eng.Pcap > first                                     # grown twice
    grown = engine_result(eng, params, variables)
    _remove_half_and_check(eng, params, variables)
    ample = _run_densify(st, 4 * (2049 + C + n_split * S))
    assert_identical(grown, engine_result(*ample[:3]))
    exp = mc.expected_densify(st, draw_normals(n_split * S, SEED, "cuda"))
    assert_rows(grown, exp, relative_to_max=True)


# ---------------------------------------------------------------------------------------------------------------------
# an edited map still runs
# ---------------------------------------------------------------------------------------------------------------------
def test_an_edited_map_still_renders_and_steps():
    """1025 rows after add + densify + prune: relearn_lists and one mapping_iteration on a 48x32 camera -- no overflow flag, a
    finite loss.  The only render in this file."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    W, H, n = 48, 32, 1025
    f, cx, cy = 40.0, W / 2 - 0.5, H / 2 - 0.5
    params, variables = slam.synthetic_params(n, W, H, f, f, cx, cy, num_frames=3, seed=11, device="cuda")
    k = torch.tensor([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    cam = slam.setup_camera(W, H, k.numpy(), np.eye(4, dtype=np.float32), device="cuda")
    g = torch.Generator().manual_seed(5)
    im = torch.rand(3, H, W, generator=g).cuda()
    depth = (1.0 + 3.0 * torch.rand(1, H, W, generator=g)).cuda()
    frame = {'cam': cam, 'im': im, 'depth': depth, 'id': 1, 'w2c': torch.eye(4, device="cuda"), 'intrinsics': k}
    eng = FusedEngine(params, cam, gaussian_capacity=n, variables=variables)        # every edit that adds rows has to grow
    sil = (torch.rand(H, W, generator=g) < 0.3).float().cuda()
    added = eng.add_new_gaussians(frame, 0.5, 1, "projective", "isotropic", depth_sil=torch.stack([depth[0], 1.0 - sil]))
    assert added == int(sil.sum()) and eng.P == n + added
    variables['means2D_gradient_accum'].copy_(torch.rand(eng.P, generator=g).cuda() * 4e-4)
    variables['denom'].fill_(1.0)
    scales = torch.exp(params['log_scales'].detach()).max(dim=1).values
    radius = float(torch.quantile(scales, 0.5)) / 0.01
    dd = dict(start_after=0, remove_big_after=0, stop_after=100, densify_every=1, grad_thresh=2e-4, num_to_split_into=2,
              removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005, reset_opacities=False, reset_opacities_every=3000)
    P0 = eng.P
    assert eng.densify(1, dd, radius, accumulate=False) and eng.P != P0
    eng.prune_gaussians(0, dict(slam.REPLICA_PRUNE, removal_opacity_threshold=0.7), radius)
    assert 0 < eng.P
    eng.relearn_lists(frame, 1)
    eng.reset_map_optimizer()
    eng.mapping_iteration(frame, 1, slam.REPLICA_MAPPING)
    torch.cuda.synchronize()
    assert not eng.check_overflow() and np.isfinite(eng.loss())
