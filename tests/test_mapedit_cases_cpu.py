"""The edge cases of tests/mapedit_cases.py and their oracle, checked without a GPU.

 * Generator properties: every case has the property it was built for (the boundary is hit, the rank lands where intended, every
   compared value keeps its margin from the threshold, the depth errors are exact in float32), from numpy on the inputs alone.
 * The median: numpy.sort(err)[(HW - 1) // 2] with the NaN rule == torch.median of the float32 errors, bit for bit, on every plane.
 * The torch formulations (splatam_amd.slam: _add_from_render, get_pointcloud + initialize_params, remove_points, prune_gaussians,
   densify driving a real torch.optim.Adam) against the float64 statements of tests/mapedit_cases.py: same rows, same order, copied
   values bit for bit, computed values within the project's tolerance for these operations.  tests/test_mapedit_mirror.py pins the
   same functions to the reference's own code on its golden frames; this file is what lets tests/test_gpu_mapedit_edges.py trust
   them outside those frames.
"""
import numpy as np
import pytest
import torch

from splatam_amd import slam
from tests import mapedit_cases as mc
from tests.mapedit_cases import CHUNK, GAUSSIAN_KEYS, GRID, GROUP, MARGIN, ROUND, VAR_KEYS, WAVE

TOL = 2e-6                      # tests/test_gpu_mapedit.py: rtol = atol for back-projected rows, x max(1, |ref|max) for the split
CPU_ROWS = 2049                 # the mirror runs on the CPU up to this size, plus one case beyond the scan's first chunk


def _id(case):
    return "-".join(str(c) for c in case)


def _segments(mask, size):
    """Selected rows per segment of ``size`` rows (the last one may be partial) and the segment lengths."""
    n = mask.size
    starts = np.arange(0, n, size)
    return np.add.reduceat(mask.astype(np.int64), starts), np.minimum(size, n - starts)


# ---------------------------------------------------------------------------------------------------------------------
# generator properties
# ---------------------------------------------------------------------------------------------------------------------
def test_kept_cases_contain_what_is_mandatory():
    kept = set(mc.COMPACTION_CASES)
    assert len(kept) == len(mc.COMPACTION_CASES)
    for n in mc.SIZES:
        assert all((n, p) in kept for p in ("none", "all", "last", "random50")), n
    for p in mc.PATTERNS:
        assert (262145, p) in kept, p
        assert (1025, p) in kept or p in mc.CARRY_PATTERNS, p
    add = set(mc.ADD_CASES)
    for p in mc.PATTERNS:
        assert any(k == p and w * h == 262656 for (w, h, k, c) in add), p
        assert any(k == p and w * h == 1025 for (w, h, k, c) in add) or p in mc.CARRY_PATTERNS, p
    for k in mc.SPECIAL_FRAMES:
        assert {c for (w, h, kk, c) in add if kk == k} == {1, 3}, k
    dens = set(mc.DENSIFY_CASES)
    assert all((n, "mixed_2") in dens for n in mc.SIZES)
    assert all((n, k) in dens for n in (1025, 262145) for k in mc.DENSIFY_KINDS if k != "double_growth")
    assert {mc.DENSIFY_KINDS[k][0] for k in mc.DENSIFY_KINDS} == {1, 2, 3}
    # the sizes of 256, 257 and 258 workgroups: the scan's second chunk and its carry
    assert [(n + GROUP - 1) // GROUP for n in (262144, 262145, 263169)] == [256, 257, 258]
    assert 513 * 512 > 1024 * ROUND and (513 * 512 + GROUP - 1) // GROUP > 256


@pytest.mark.parametrize("case", mc.COMPACTION_CASES, ids=_id)
def test_mask_has_the_property_it_was_built_for(case):
    n, pattern = case
    m = mc.select_mask(n, pattern)
    assert m.dtype == bool and m.shape == (n,)
    assert np.array_equal(m, mc.select_mask(n, pattern))             # deterministic
    per64, len64 = _segments(m, WAVE)
    per256, len256 = _segments(m, ROUND)
    per1024, len1024 = _segments(m, GROUP)
    where = np.flatnonzero(m)
    if pattern == "none":
        assert where.size == 0
    elif pattern == "all":
        assert where.size == n
    elif pattern == "first":
        assert where.tolist() == [0]
    elif pattern == "last":
        assert where.tolist() == [n - 1]
    elif pattern in ("last_of_64", "last_of_256", "last_of_1024"):
        size, per, length = {"last_of_64": (WAVE, per64, len64), "last_of_256": (ROUND, per256, len256),
                             "last_of_1024": (GROUP, per1024, len1024)}[pattern]
        assert np.array_equal(per, (length == size).astype(np.int64))      # one per FULL segment ...
        assert np.all(where % size == size - 1)                             # ... on its last row: every row before it is unselected
    elif pattern == "first_of_1024":
        assert np.all(per1024 == 1) and np.all(where % GROUP == 0)
    elif pattern == "all_but_one_per_group":
        assert np.array_equal(per1024, len1024 - 1)
    elif pattern == "random50":
        if n >= 255:
            assert 0.4 < m.mean() < 0.6
            assert np.all(per64[len64 == WAVE] > 0) and np.all(per64[len64 == WAVE] < WAVE)   # every full wave is mixed
    elif pattern == "random1":
        assert 0 < m.mean() < 0.02
        assert np.any(per64 == 0) and np.any(per64 > 0)                    # empty waves next to occupied ones
    elif pattern == "one_full_group":
        assert per1024[0] == len1024[0] and per1024[1:].sum() == 0 and per1024.size > 1
    elif pattern == "first_256_groups":
        assert n > CHUNK and per1024[:256].sum() == CHUNK and per1024[256:].sum() == 0
    elif pattern == "after_256_groups":
        assert n > CHUNK and per1024[:256].sum() == 0 and np.all(per1024[256:] == len1024[256:])


def _placement(mask, carry=True, inclusive_rank=False, first_chunk_only=False):
    """Destination of every selected row as a compaction of this shape derives it -- per-workgroup counts, an exclusive scan over them
    in chunks of 256 with a running total, the waves before this one inside the workgroup, the rank among the lanes of the wave's
    ballot -- with three defects that can be switched on: the running total dropped, the lane's own bit counted into its rank, and a
    scan that stops after its first chunk (the later workgroups keep their raw counts as offsets)."""
    n = mask.size
    m = mask.astype(np.int64)
    per_group, _ = _segments(mask, GROUP)
    offset = np.zeros(per_group.size, dtype=np.int64)
    total = 0
    for c in range(0, per_group.size, 256):
        part = per_group[c:c + 256]
        offset[c:c + 256] = part if (first_chunk_only and c) else (total if carry else 0) + np.cumsum(part) - part
        total += int(part.sum())
    before = np.cumsum(m) - m                                               # selected rows before this one, anywhere
    i = np.arange(n)
    wave_first, group_first = (i // WAVE) * WAVE, (i // GROUP) * GROUP
    in_wave = before - before[wave_first] + (1 if inclusive_rank else 0)
    waves_before = before[wave_first] - before[group_first]
    return (offset[i // GROUP] + waves_before + in_wave)[mask]


def test_the_targeted_cases_tell_a_defect_from_sound_code():
    """The boundary cases are the ones that notice.  Without the carry a row is misplaced exactly where rows are selected on BOTH sides
    of workgroup 256 ("all", "random50", "all_but_one_per_group", the periodic patterns, at 262145 rows and more); where nothing is
    selected in the first 256 workgroups the carry is 0, and what those cases notice is a scan that never reaches its second chunk.
    A lane that counts its own bit moves every selected row, "last of 64" included, where it is the only selected lane of its wave.
    The upper median differs from the lower one exactly on the even-HW two-value, half-zero and half-inf planes."""
    for n, pattern in mc.COMPACTION_CASES:
        mask = mc.select_mask(n, pattern)
        want = np.arange(int(mask.sum()))
        assert np.array_equal(_placement(mask), want), (n, pattern)
        dropped = _placement(mask, carry=False)
        both_sides = bool(mask[:mc.CHUNK].any() and mask[mc.CHUNK:].any())
        assert np.array_equal(dropped, want) != both_sides, (n, pattern)    # (otherwise the carry is never read, or is 0)
        stopped = _placement(mask, first_chunk_only=True)
        assert np.array_equal(stopped, want) != bool(mask[mc.CHUNK:].any()), (n, pattern)
        if pattern == "after_256_groups":
            assert not np.any(stopped == want)                              # every row on a wrong slot
        if mask.any():
            assert not np.any(_placement(mask, inclusive_rank=True) == want), (n, pattern)
    for W, H, dist in mc.MEDIAN_CASES:
        gt, rd, props = mc.median_plane(W, H, dist)
        err = mc.depth_error(gt.numpy(), rd.numpy())
        if np.isnan(err).any():
            continue
        upper = np.sort(err)[err.size // 2]
        differs = upper != props['expected']
        if dist in ("two_lower", "half_zero", "inf_half") and err.size % 2 == 0:
            assert differs, (W, H, dist)
        if dist in ("equal", "mostly_zero", "two_upper") or err.size % 2 == 1:
            assert not differs, (W, H, dist)


@pytest.mark.parametrize("case", mc.MEDIAN_CASES, ids=_id)
def test_plane_has_its_rank_where_intended_and_numpy_median_is_torch_median(case):
    W, H, dist = case
    gt, rd, props = mc.median_plane(W, H, dist)
    hw, rank = W * H, (W * H - 1) // 2
    assert gt.shape == rd.shape == (hw,) and gt.dtype == rd.dtype == torch.float32
    err = mc.depth_error(gt.numpy(), rd.numpy())
    expected = props['expected']
    # torch.median of the float32 errors, formed as the reference forms them, bit for bit
    t_err = torch.abs(gt - rd) * (gt > 0)
    assert np.array_equal(t_err.numpy().view(np.uint32), err.view(np.uint32)) or np.isnan(err).any()
    t_med = np.float32(t_err.median().item())
    assert (np.isnan(t_med) and np.isnan(expected)) or t_med.view(np.uint32) == np.float32(expected).view(np.uint32), (t_med, expected)
    # the errors are exact in float32: the float64 difference is the same number
    with np.errstate(invalid="ignore"):
        exact = np.abs(gt.numpy().astype(np.float64) - rd.numpy().astype(np.float64)) * (gt.numpy() > 0)
    finite = np.isfinite(exact)
    assert np.array_equal(exact[finite], err[finite].astype(np.float64))
    srt = np.sort(err)                                                     # (NaN last)
    bits = err.view(np.uint32)
    if dist == "equal":
        assert np.all(err == expected) and expected == np.float32(0.25)
    elif dist == "mostly_zero":
        assert (gt.numpy() == 0).sum() > hw / 2 and expected == 0.0 and (hw <= 2 or srt[-1] > 0)
    elif dist == "half_zero":
        assert (err == 0).sum() == hw // 2 and expected == 0.0 and srt[rank + 1] > 0     # the lower median is the LAST zero
    elif dist == "half_zero_less_one":
        assert (err == 0).sum() == hw // 2 - 1 and expected == srt[hw // 2 - 1] > 0 and expected == err[err > 0].min()
    elif dist == "two_lower":
        assert srt[rank] == np.float32(0.125) and srt[rank + 1] == np.float32(0.375) and expected == np.float32(0.125)
    elif dist == "two_upper":
        assert srt[rank - 1] == np.float32(0.125) and srt[rank] == np.float32(0.375) and expected == np.float32(0.375)
    elif dist.startswith("bits_"):
        varying = np.bitwise_or.reduce(bits ^ bits[0])
        allowed = {"bits_low": 0x3ff, "bits_mid": 0x1ffc00, "bits_high": 0xffe00000}[dist]
        assert varying & ~np.uint32(allowed) == 0 and (hw < 17 or varying != 0)
        assert np.all(np.isfinite(err)) and np.all(err >= np.finfo(np.float32).tiny)
    elif dist == "inf_minority":
        assert np.isfinite(expected) and props['infs'] < hw / 2 and (hw <= 2 or np.isinf(srt[rank + 1 + (hw + 1) % 2]))
    elif dist == "inf_half":
        assert np.isfinite(expected) and props['infs'] * 2 == hw and np.isinf(srt[rank + 1])     # the lower median is the last finite error
    elif dist == "inf_majority":
        assert np.isinf(expected) and props['infs'] > hw / 2 and (hw <= 2 or np.isfinite(srt[rank - 1]))
    elif dist == "nan_one":
        assert np.isnan(expected) and np.isnan(rd.numpy()).sum() == 1
    elif dist == "zero_times_inf":
        assert np.isnan(expected) and not np.isnan(rd.numpy()).any() and not np.isnan(gt.numpy()).any()


def _margin(value, threshold):
    """Smallest relative distance of ``value`` from ``threshold``."""
    value = np.asarray(value, dtype=np.float64).reshape(-1)
    return np.inf if value.size == 0 else float(np.min(np.abs(value - threshold)) / abs(threshold))


@pytest.mark.parametrize("case", mc.ADD_CASES, ids=_id)
def test_add_frame_has_the_property_it_was_built_for(case):
    W, H, kind, cols = case
    frame, props = mc.add_frame(W, H, kind, cols)
    exp = mc.expected_add(frame)
    hw = W * H
    gt, rd, sil = frame['depth'].numpy().reshape(-1), frame['depth_sil'][0].numpy().reshape(-1), frame['depth_sil'][1].numpy().reshape(-1)
    k = frame['intrinsics'].numpy()
    assert k[0, 0] != k[1, 1] and frame['params']['log_scales'].shape == (mc.N0, cols)
    q = frame['params']['cam_unnorm_rots'].numpy()[0, :, mc.TIME_IDX]
    assert abs(np.linalg.norm(q) - 1) > 0.1 and np.abs(q[1:]).min() > 0.05 and np.abs(frame['params']['cam_trans'].numpy()[0, :, mc.TIME_IDX]).min() > 0.1
    assert all(float(v.abs().min()) > 0 for kk, v in frame['variables'].items() if kk != 'timestep') and float(frame['variables']['timestep'].max()) > 0
    # depths on the grid, within range; the errors exact; every compared value away from its threshold
    valid = gt > 0
    assert np.array_equal(gt * GRID, np.round(gt * GRID)) and np.all((gt[valid] >= 0.5) & (gt[valid] <= 5.0))
    fin = np.isfinite(rd)
    assert np.array_equal(rd[fin] * GRID, np.round(rd[fin] * GRID))
    assert _margin(sil, mc.SIL_THRES) >= MARGIN
    med = exp['median']
    if 'median' in props:
        assert med == props['median']
    with np.errstate(invalid="ignore"):
        candidates = fin & (rd > gt) & valid                               # pixels whose selection the 50 x median comparison decides
    if np.isfinite(med) and med > 0:
        assert _margin(exp['err'][candidates], 50.0 * float(med)) >= MARGIN
    by_sil, by_depth = sil < mc.SIL_THRES, exp['behind']
    if kind in mc.PATTERNS:
        assert np.array_equal(exp['pick'], mc.select_mask(hw, kind, seed="add")) and not by_depth.any() and exp['added'] == exp['non_presence']
    elif kind == "invalid_selected":
        assert exp['non_presence'] > 0 and exp['added'] == 0 and not by_depth.any()
        assert all(np.all(exp['variables'][v] == 0) for v in VAR_KEYS[:3]) and exp['params']['means3D'].shape[0] == mc.N0
    elif kind == "depth_rule":
        assert not by_sil.any() and 0 < by_depth.sum() == exp['added'] < candidates.sum()
        assert np.any((exp['err'] > 50 * med) & ~by_depth)               # a large error in front of the measurement does not select
    elif kind == "sil_rule":
        assert not by_depth.any() and candidates.all() and 0 < exp['added'] == by_sil.sum()
    elif kind == "nan_median":
        assert np.isnan(med) and not by_depth.any() and (exp['err'][candidates] >= 0.25).any() and 0 < exp['added'] == (by_sil & valid).sum()
    elif kind == "median_zero":
        assert med == 0.0 and (~valid).sum() > hw / 2 and not by_sil.any()
        assert 0 < exp['added'] == (candidates & (exp['err'] > 0)).sum() < valid.sum()
    # the computed values stay where the tolerance is meaningful
    assert np.abs(exp['params']['means3D']).max() <= 12.0


@pytest.mark.parametrize("case", mc.PRUNE_CASES, ids=_id)
def test_prune_state_keeps_its_margins(case):
    n, rule = case
    st = mc.prune_state(n, rule)
    op = 1 / (1 + np.exp(-st['params']['logit_opacities'].numpy().astype(np.float64)))
    scale = np.exp(st['params']['log_scales'].numpy().astype(np.float64))
    assert _margin(op, mc.PRUNE_OPACITY) >= MARGIN and _margin(scale, 0.1 * mc.PRUNE_RADIUS) >= MARGIN
    rem_op, rem_all = mc.expected_prune(st, False), mc.expected_prune(st, True)
    assert 0 < rem_op.sum() < rem_all.sum() < n
    if rule == "aniso":                                                     # the largest of three decides, whichever column holds it
        big = scale > 0.1 * mc.PRUNE_RADIUS
        assert scale.shape[1] == 3 and big.sum(axis=1).max() == 1 and all(big[:, c].any() for c in range(3))


@pytest.mark.parametrize("case", mc.DENSIFY_CASES, ids=_id)
def test_densify_state_has_the_property_it_was_built_for(case):
    n, kind = case
    st = mc.densify_state(n, kind)
    d, R = st['dict'], st['radius']
    to_clone, to_split, g, scale = mc.densify_selection(st)
    n_split = d['num_to_split_into']
    exp = mc.expected_densify(st, np.zeros((n_split * int(to_split.sum()), 3)))
    assert st['params']['log_scales'].shape == (n, 1)
    if d['grad_thresh'] > 0:
        assert _margin(g[g > 0], d['grad_thresh']) >= MARGIN
    assert _margin(scale, 0.01 * R) >= MARGIN
    assert _margin(exp['final_scale'], 0.1 * R) >= MARGIN                  # before AND after the split's division by 0.8 n
    if d['removal_opacity_threshold'] > 0:
        assert _margin(exp['opacity'], d['removal_opacity_threshold']) >= MARGIN
    acc, den = st['variables']['means2D_gradient_accum'].numpy(), st['variables']['denom'].numpy()
    if n >= 64 and kind not in ("clone:all", "split:all", "clone:first_256_groups", "split:first_256_groups"):
        assert ((acc == 0) & (den == 0)).any() and ((acc == 0) & (den > 0)).any()      # 0 / 0 rows and gradients of exactly 0
    if n > 1:
        assert np.unique(st['variables']['timestep'].numpy()).size > 1
    assert all(float(st[m][k].abs().min()) > 0 for m in ('exp_avg', 'exp_avg_sq') for k in GAUSSIAN_KEYS)
    C, S = exp['cloned'], exp['split']
    rows = exp['params']['means3D'].shape[0]
    if kind == "nothing":
        assert C == 0 and S == 0 and rows == n
    elif kind == "clone_only":
        assert C > 0 and S == 0
    elif kind == "split_only":
        assert C == 0 and S > 0
    elif kind == "thresh_0":
        assert d['grad_thresh'] == 0.0 and C + S == n and C > 0 and S > 0   # 0 / 0 and zero-gradient rows included
    elif kind.startswith("mixed") and n >= 63:
        assert C > 0 and S > 0
    elif kind == "double_growth":
        # one row short for the clones, the engine grows to 1.5 (n + C) + 1024 rows: the split's rows must not fit into that either
        assert C > 0 and n + C + n_split * S > int((n + C) * 1.5) + 1024
    elif ":" in kind:
        step, pattern = kind.split(":")
        mask = mc.select_mask(n, pattern, seed="densify")
        assert np.array_equal(to_clone if step == "clone" else to_split, mask) and (S if step == "clone" else C) == 0
    if d['removal_opacity_threshold'] == 0.0:
        assert rows == exp['peak'] - S                                     # the final prune removes nothing
    elif n >= 1025:
        faint = exp['opacity'] < d['removal_opacity_threshold']
        big = exp['final_scale'] > 0.1 * R
        assert faint.any() and big.any() and rows < exp['peak'] - S        # a known subset, by both rules
    assert rows == 0 or np.abs(exp['params']['means3D']).max() <= 12.0


# ---------------------------------------------------------------------------------------------------------------------
# the torch formulations on the edge cases
# ---------------------------------------------------------------------------------------------------------------------
def make_mirror(st, device="cpu"):
    """``st`` as splatam_amd.slam sees a map: Parameters, variables and a real Adam whose state holds the case's moments."""
    params = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in st['params'].items()}
    if 'cam_unnorm_rots' not in params:
        params['cam_unnorm_rots'] = torch.nn.Parameter(torch.tensor([[[1.0] * 2, [0.0] * 2, [0.0] * 2, [0.0] * 2]], device=device))
        params['cam_trans'] = torch.nn.Parameter(torch.zeros(1, 3, 2, device=device))
    variables = {k: v.clone().to(device) for k, v in st['variables'].items()}
    opt = slam.initialize_optimizer(params, slam.REPLICA_MAPPING['lrs'], tracking=False)
    for k in GAUSSIAN_KEYS:
        opt.state[params[k]] = {'step': torch.tensor(1.0), 'exp_avg': st['exp_avg'][k].clone().to(device),
                                'exp_avg_sq': st['exp_avg_sq'][k].clone().to(device)}
    return params, variables, opt


def mirror_result(params, variables, opt=None):
    out = {'params': {k: params[k].detach().cpu().numpy() for k in GAUSSIAN_KEYS},
           'variables': {k: variables[k].cpu().numpy() for k in VAR_KEYS}}
    if opt is not None:
        out['exp_avg'] = {k: opt.state[params[k]]['exp_avg'].cpu().numpy() for k in GAUSSIAN_KEYS}
        out['exp_avg_sq'] = {k: opt.state[params[k]]['exp_avg_sq'].cpu().numpy() for k in GAUSSIAN_KEYS}
    return out


def assert_rows(got, exp, relative_to_max=False, groups=('params', 'exp_avg', 'exp_avg_sq', 'variables')):
    """``got`` (float32 arrays) against an expected state: same shapes; float32 expectations (copied values) bit for bit; float64
    expectations (computed values) within TOL -- rtol = atol, or TOL x max(1, |ref|max) for the split -- and bit for bit on the rows
    ``exp['copied']`` marks as copies.  Returns the largest error of the computed values."""
    worst = 0.0
    for g in groups:
        if g not in got:
            continue
        for k, ref in exp[g].items():
            have = got[g][k]
            assert have.shape == ref.shape, (g, k, have.shape, ref.shape)
            if ref.dtype == np.float64:
                copied = exp['copied']
                np.testing.assert_array_equal(have[copied], ref[copied].astype(np.float32), err_msg=f"{g}/{k} (copied rows)")
                if relative_to_max:
                    bound = TOL * max(1.0, float(np.abs(ref).max())) if ref.size else 0.0
                    err = float(np.abs(have - ref).max()) if ref.size else 0.0
                    assert err <= bound, (g, k, err, bound)
                else:
                    np.testing.assert_allclose(have, ref, rtol=TOL, atol=TOL, err_msg=f"{g}/{k}")
                    err = float(np.abs(have - ref).max()) if ref.size else 0.0
                worst = max(worst, err)
            else:
                np.testing.assert_array_equal(have, ref, err_msg=f"{g}/{k}")
    return worst


def frame_data(frame, device="cpu"):
    return {'cam': None, 'im': frame['im'].to(device), 'depth': frame['depth'].to(device), 'id': frame['time_idx'],
            'intrinsics': frame['intrinsics'].clone(), 'w2c': torch.eye(4, device=device)}


def mirror_add(frame, device="cpu"):
    params, variables, _ = make_mirror(frame, device)
    dist = "isotropic" if frame['cols'] == 1 else "anisotropic"
    params, variables = slam._add_from_render(params, variables, frame_data(frame, device), frame['depth_sil'].to(device), frame['sil_thres'],
                                              frame['time_idx'], "projective", dist)
    return mirror_result(params, variables)


@pytest.mark.parametrize("case", mc.ADD_CASES, ids=_id)
def test_add_from_render_matches_the_float64_statement(case):
    frame, _ = mc.add_frame(*case)
    exp = mc.expected_add(frame)
    got = mirror_add(frame)
    assert got['params']['means3D'].shape[0] == mc.N0 + exp['added']
    assert_rows(got, exp)


@pytest.mark.parametrize("size", mc.PLANE_SIZES, ids=_id)
@pytest.mark.parametrize("n0", [0, mc.N0])
def test_pointcloud_and_initialize_params_match_the_float64_statement(size, n0):
    W, H = size
    cols = 1 if (W + n0) % 2 else 3
    frame = mc.valid_depth_frame(W, H, cols, n0)
    exp = mc.expected_valid_depth(frame)
    got = mirror_valid_depth(frame)
    n = int((frame['depth'] > 0).sum())
    assert exp['added'] == n and 0 < n < W * H or W * H <= 2
    assert_rows(got, exp, groups=('params', 'variables'))


def mirror_valid_depth(frame, device="cpu"):
    """get_pointcloud(mask = depth > 0) + initialize_params, appended to the frame's map (the variables as the first frame makes them)."""
    depth = frame['depth'].to(device)
    cloud, msd = slam.get_pointcloud(frame['im'].to(device), depth, frame['intrinsics'], frame['w2c'].to(device), mask=(depth > 0).reshape(-1),
                                     compute_mean_sq_dist=True)
    new, new_vars = slam.initialize_params(cloud, mc.NUM_FRAMES, msd, "isotropic" if frame['cols'] == 1 else "anisotropic")
    n = cloud.shape[0]
    old = frame['params']
    out = {'params': {k: torch.cat((old[k].to(device), new[k].detach())).cpu().numpy() for k in GAUSSIAN_KEYS}}
    if n:
        out['variables'] = {k: torch.cat((torch.zeros(old['means3D'].shape[0], device=device), new_vars[k])).cpu().numpy() for k in VAR_KEYS[:3]}
        out['variables']['timestep'] = torch.cat((frame['variables']['timestep'].to(device), new_vars['timestep'])).cpu().numpy()
    else:
        out['variables'] = {k: frame['variables'][k].numpy() for k in VAR_KEYS}
    return out


REMOVE_ON_CPU = [c for c in mc.COMPACTION_CASES if c[0] <= CPU_ROWS] + [(262145, "after_256_groups")]


@pytest.mark.parametrize("case", REMOVE_ON_CPU, ids=_id)
def test_remove_points_matches_boolean_indexing(case):
    n, pattern = case
    keep = mc.select_mask(n, pattern)
    st = mc.map_state(n, 1 + 2 * (n % 2), seed="remove")
    params, variables, opt = make_mirror(st)
    params, variables = slam.remove_points(torch.from_numpy(~keep), params, variables, opt)
    got = mirror_result(params, variables, opt)
    assert got['params']['means3D'].shape[0] == int(keep.sum())
    assert_rows(got, mc.compacted(st, keep))


def prune_dict(remove_big):
    return dict(slam.REPLICA_PRUNE, removal_opacity_threshold=mc.PRUNE_OPACITY, remove_big_after=0 if remove_big else 10 ** 9)


@pytest.mark.parametrize("case", [c for c in mc.PRUNE_CASES if c[0] <= CPU_ROWS] + [(262145, "aniso")], ids=_id)
def test_prune_gaussians_matches_the_float64_rules(case):
    n, rule = case
    st = mc.prune_state(n, rule)
    remove_big = rule != "opacity"
    params, variables, opt = make_mirror(st)
    variables['scene_radius'] = torch.tensor(mc.PRUNE_RADIUS)
    params, variables = slam.prune_gaussians(params, variables, opt, 0, prune_dict(remove_big))
    rem = mc.expected_prune(st, remove_big)
    assert_rows(mirror_result(params, variables, opt), mc.compacted(st, ~rem))


def draw_normals(count, seed, device="cpu"):
    """The standard-normal draws behind torch.normal(mean=zeros([count, 3]), std=...) under ``seed``: torch fills with N(0, 1) and
    scales, so the split's samples are these draws times the scales, whatever the scales are."""
    torch.manual_seed(seed)
    z = torch.zeros(count, 3, device=device)
    return torch.normal(mean=z, std=torch.ones_like(z)).cpu().numpy() if count else np.zeros((0, 3), dtype=np.float32)


def mirror_densify(st, seed, device="cpu"):
    """slam.densify on ``st``, seeded as tests/test_mapedit_mirror.py::test_densify_matches_reference seeds it, on a real Adam; this
    iteration's own gradient is zero (nothing seen), so the accumulated history is what decides."""
    params, variables, opt = make_mirror(st, device)
    n = params['means3D'].shape[0]
    variables['scene_radius'] = torch.tensor(st['radius'], device=device)
    variables['seen'] = torch.zeros(n, dtype=torch.bool, device=device)
    m2d = torch.zeros(n, 3, device=device, requires_grad=True)
    m2d.grad = torch.zeros(n, 3, device=device)
    variables['means2D'] = m2d
    torch.manual_seed(seed)
    params, variables = slam.densify(params, variables, opt, 1, st['dict'])
    return mirror_result(params, variables, opt)


@pytest.mark.parametrize("case", [c for c in mc.DENSIFY_CASES if c[0] <= CPU_ROWS] + [(262145, "mixed_2")], ids=_id)
def test_densify_matches_the_float64_statement(case):
    st = mc.densify_state(*case)
    _, to_split, _, _ = mc.densify_selection(st)
    exp = mc.expected_densify(st, draw_normals(st['dict']['num_to_split_into'] * int(to_split.sum()), 1234))
    got = mirror_densify(st, 1234)
    assert got['params']['means3D'].shape[0] == exp['params']['means3D'].shape[0]
    assert_rows(got, exp, relative_to_max=True)
    # timestep of every surviving row is its source row's (the reference's densify does not extend it: stated on the sources)
    assert np.array_equal(got['variables']['timestep'], st['variables']['timestep'].numpy()[exp['source']])
