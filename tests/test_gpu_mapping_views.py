"""Multi-view mapping at distinct keyframe poses (tests/util.py: multiview_scene): the set of Gaussians a mapping iteration sees
changes from one iteration to the next, as it does in SplaTAM's mapping loop (a random keyframe per iteration).

  1. the scene's partition of the map: rows seen by every keyframe, by some, by none, and rows behind the near plane of the
     forward view -- each a few per cent of the map, so that no comparison below runs over an empty set;
  2. one view at a real pose (the most rotated one, the forward one) against the C oracle: the staged comparison of
     tests/test_gpu_configs.py (_fused_stages) at config B, mapping and tracking;
  3. FusedEngine.mapping_batch at BASELINE config 3 (8 keyframe views per mapping step on B's map) against get_loss + autograd on
     the drop-in rasterizer per view, averaged, and one step of torch.optim.Adam; the same step over two emulated ranks; and list
     buckets learnt on one pose, used on the others;
  4. the Adam step on rows outside the view (zero gradient, non-zero moments), on the three paths that take it (F6's fused step,
     adam_map, mapping_batch), against a float64 restatement of torch.optim.Adam fed with the engine's own inputs."""
import time

import numpy as np
import pytest
import torch

from tests.test_gpu_configs import _check_pose_gradient, _fused_stages
from tests.test_gpu_fused import _cmp
from tests.util import FORWARD_VIEW, MOST_ROTATED_VIEW, assert_grad_calibrated, multiview_scene, view_partition

pytestmark = pytest.mark.gpu

KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
_SCENES = {}


def _scene(size, first_w2c=None):
    """The scene of one size, made once per session (every test works on clones of its parameters); ``first_w2c``: the map and all
    eight keyframes under a first-frame matrix other than the identity."""
    key = size if first_w2c is None else (size, np.asarray(first_w2c, dtype=np.float32).tobytes())
    if key not in _SCENES:
        _SCENES[key] = multiview_scene(size, seed=17, first_w2c=first_w2c)
    return _SCENES[key]


def _clone(params):
    return {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}


def _reference_views(params, variables, views, cfg):
    """get_loss + autograd on the drop-in rasterizer, view by view: the per-view gradients of the five Gaussian groups and the
    radii of the colour render."""
    from splatam_amd import slam
    grads, radii = [], []
    for fr, t in views:
        for p in params.values():
            p.grad = None
        loss, var, _ = slam.get_loss(params, fr, dict(variables), t, cfg['loss_weights'], cfg['use_sil_for_loss'], cfg['sil_thres'],
                                     cfg['use_l1'], cfg['ignore_outlier_depth_loss'], mapping=True)
        loss.backward()
        grads.append({k: params[k].grad.detach().clone() for k in KEYS})
        radii.append(var['seen'].cpu().numpy())
    for p in params.values():
        p.grad = None
    torch.cuda.synchronize()
    return grads, radii


def _probe(params, cam, views, cfg):
    """Exact lists (no buckets) on every view of an untouched copy of the map: the list capacity every view fits, each view's
    longest tile list, its gradients and its rendered planes."""
    from splatam_amd.fused import FusedEngine
    e = FusedEngine(_clone(params), cam)
    e.allow_buckets = False
    out = []
    for fr, t in views:
        for _ in range(4):
            e.loss_backward(fr, t, cfg, tracking=False)
            if not e.check_overflow():
                break
        else:
            raise AssertionError(f"view {t}: the lists could not be sized")
        assert e.tile_stride == 0
        out.append(dict(longest=e.max_list_hint, out6=e.buf['out6'].clone(), grads={k: e.grads[k].clone() for k in KEYS}))
    return e.capacity, out


def _flag(eng):
    return float(eng.buf['d_cam'][12]) != 0.0


@pytest.mark.parametrize("size", ["small", "B"])
def test_multiview_partition(size):
    from splatam_amd import slam
    params, variables, cam, k, views, c = _scene(size)
    _, radii = _reference_views(_clone(params), variables, views, slam.REPLICA_MAPPING)
    view_partition(radii, params, FORWARD_VIEW, what=size)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. one view against the C oracle at a real pose
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", [MOST_ROTATED_VIEW, FORWARD_VIEW])
@pytest.mark.parametrize("tracking", [False, True])
def test_view_at_a_real_pose_vs_oracle(view, tracking, monkeypatch):
    """The in-register transform_to_frame of F1 / F6 at a 20-degree pose and at one that puts a fifth of the map behind the near
    plane (the clamped rows of that view carry no gradient: tests/test_gpu_closeup.py covers the 1.3 tan(fov) clamp), staged
    (A)..(D) against the C oracle with the tolerances of tests/test_gpu_configs.py."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    t0 = time.time()
    params, variables, cam, k, views, c = _scene('B')
    fr, t = views[view - 1]
    assert t == view
    p = _clone(params)
    cfg = slam.REPLICA_TRACKING if tracking else slam.REPLICA_MAPPING
    eng = FusedEngine(p, cam)
    for _ in range(3):
        eng.loss_backward(fr, t, cfg, tracking=tracking)
        if not eng.check_overflow():
            break
    torch.cuda.synchronize()
    what = f"fused B view {view} {'tracking' if tracking else 'mapping'}"
    g32, g64 = _fused_stages(eng, p, variables, fr, (c['W'], c['H'], k), c, cfg, tracking, what, monkeypatch, time_idx=t)
    if tracking:
        _check_pose_gradient(eng, g32, g64, what, time_idx=t)
    else:
        tail = 2.0 if eng.depth_tie_pixels == 0 else 3.0
        for key in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
            assert_grad_calibrated(eng.grads[key].cpu().numpy(), g32[key], g64[key], what=f"{what} grad {key}", tail_factor=tail)
        assert float(eng.grads["unnorm_rotations"].abs().max()) == 0.0
    print(f"{what}: {time.time() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. mapping_batch at BASELINE config 3
# ------------------------------------------------------------------------------------------------------------------------------

def test_mapping_batch_config3_vs_autograd_and_adam(size='B', first_w2c=None):
    """8 keyframe views per mapping step on B's map (tests/test_gpu_world_frame.py: the small map under a general first-frame matrix): the averaged gradient, the moments on EVERY row (after one step
    exp_avg = 0.1 g and exp_avg_sq = 0.001 g^2), the parameters where the gradient is significant; rows no view sees keep a zero
    gradient, zero moments and bit-identical parameters.  Then the same step over two emulated ranks (5 + 3 views)."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, cam, k, views, c = _scene(size, first_w2c)
    cfg = slam.REPLICA_MAPPING
    t0 = time.time()
    ref = _clone(params)
    per_view, radii = _reference_views(ref, variables, views, cfg)
    groups, _ = view_partition(radii, params, FORWARD_VIEW, what=size, first_w2c=first_w2c)
    none = torch.as_tensor(groups['no view'], device="cuda")
    mean = {key: sum(g[key] for g in per_view) / len(views) for key in KEYS}
    opt = slam.initialize_optimizer(ref, cfg['lrs'], tracking=False)
    for key in KEYS:
        ref[key].grad = mean[key].clone()
    opt.step()
    capacity, _ = _probe(params, cam, views, cfg)
    p_one = _clone(params)
    e = FusedEngine(p_one, cam, capacity=capacity)
    e.mapping_batch(views, cfg)
    torch.cuda.synchronize()
    assert not _flag(e), "a view of the batch overflowed its lists"
    assert e.map_step == 1
    keys = ("means3D", "rgb_colors", "logit_opacities", "log_scales")
    for key in keys:
        st = opt.state[ref[key]]
        _cmp(e.grads[key], mean[key], f"(a) mean gradient {key}")
        _cmp(e.exp_avg[key] / 0.1, st['exp_avg'] / 0.1, f"(b) exp_avg / 0.1 {key}")
        _cmp(torch.sqrt(e.exp_avg_sq[key] / 0.001), torch.sqrt(st['exp_avg_sq'] / 0.001), f"(b) sqrt(exp_avg_sq / 0.001) {key}")
        assert float(e.grads[key][none].abs().max()) == 0.0, key
        assert float(e.exp_avg[key][none].abs().max()) == 0.0 and float(e.exp_avg_sq[key][none].abs().max()) == 0.0, key
        assert torch.equal(p_one[key].detach()[none], params[key].detach()[none]), key
        lr = cfg['lrs'][key]
        sig = mean[key].abs() > 1e-4 * mean[key].abs().max()
        diff = (p_one[key].detach() - ref[key].detach()).abs()[sig]
        print(f"(c) {key}: {int(sig.sum())} significant elements, max |p - p_ref| {float(diff.max()):.3e} (lr {lr:g}), "
              f"{float((diff > 0.05 * lr).float().mean()):.2e} beyond 0.05 lr")
        assert float((diff > 0.05 * lr).float().mean()) < 5e-3, (key, float(diff.max()), lr)
    assert torch.equal(p_one['unnorm_rotations'].detach(), params['unnorm_rotations'].detach())         # isotropic map
    # (d) two ranks: views 0..4 and 5..7; the "all-reduce" adds the other rank's accumulated sum
    p_a = _clone(params)
    e_a, e_b = FusedEngine(p_a, cam, capacity=capacity), FusedEngine(_clone(params), cam, capacity=capacity)
    other = None
    for fr, t in views[5:]:
        e_b.loss_backward(fr, t, cfg, tracking=False)
        other = e_b.reduce_flat.clone() if other is None else other + e_b.reduce_flat
    e_a.mapping_batch(views[:5], cfg, total_views=len(views), allreduce_sum=lambda red: red[red.numel() - other.numel():].add_(other))
    torch.cuda.synchronize()
    assert not _flag(e_a) and not _flag(e_b)
    for key in keys:
        _cmp(e_a.grads[key], e.grads[key], f"(d) two ranks: gradient {key}")
        _cmp(e_a.exp_avg[key], e.exp_avg[key], f"(d) two ranks: exp_avg {key}")
        _cmp(torch.sqrt(e_a.exp_avg_sq[key]), torch.sqrt(e.exp_avg_sq[key]), f"(d) two ranks: sqrt(exp_avg_sq) {key}")
        assert torch.equal(p_a[key].detach()[none], params[key].detach()[none]), key
        lr = cfg['lrs'][key]
        sig = e.grads[key].abs() > 1e-4 * e.grads[key].abs().max()
        diff = (p_a[key].detach() - p_one[key].detach()).abs()[sig]
        assert float((diff > 0.05 * lr).float().mean()) < 5e-3, (key, float(diff.max()), lr)
    print(f"mapping_batch at config 3: {time.time() - t0:.1f} s")


def test_buckets_learnt_on_one_pose_hold_or_flag_on_the_others():
    """Per-tile list buckets learnt (check_overflow()) on the keyframe with the shortest lists, then every other keyframe: each
    iteration either equals its exact-list iteration (same planes, same gradients) or raises the capacity flag -- and then the
    Adam step leaves map and moments as they were.  A bucket that silently truncates another pose's lists fails here."""
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, cam, k, views, c = _scene('B')
    cfg = slam.REPLICA_MAPPING
    capacity, exact = _probe(params, cam, views, cfg)
    longest = [x['longest'] for x in exact]
    s = int(np.argmin(longest))
    print(f"longest tile list per view {longest}: buckets learnt on view {views[s][1]}")
    p = _clone(params)
    eb = FusedEngine(p, cam, capacity=capacity)
    g = torch.Generator(device="cuda").manual_seed(5)
    for key in KEYS:                                 # moments that an Adam step would move
        eb.exp_avg[key].copy_(torch.randn(eb.exp_avg[key].shape, generator=g, device="cuda") * 1e-3)
        eb.exp_avg_sq[key].copy_(torch.rand(eb.exp_avg_sq[key].shape, generator=g, device="cuda") * 1e-6)
    held = flagged = 0
    for i, (fr, t) in enumerate(views):
        if i == s:
            continue
        eb.tile_stride, eb.max_list_hint = 0, 0
        eb.loss_backward(*views[s], cfg, tracking=False)
        assert not eb.check_overflow() and eb.tile_stride > 0 and eb.max_list_hint == longest[s]
        snap = ({key: p[key].detach().clone() for key in KEYS}, {key: eb.exp_avg[key].clone() for key in KEYS},
                {key: eb.exp_avg_sq[key].clone() for key in KEYS})
        eb.loss_backward(fr, t, cfg, tracking=False)
        torch.cuda.synchronize()
        if _flag(eb):
            flagged += 1
            eb.adam_map(cfg['lrs'])
            torch.cuda.synchronize()
            for key in KEYS:
                assert torch.equal(p[key].detach(), snap[0][key]), (t, key)
                assert torch.equal(eb.exp_avg[key], snap[1][key]) and torch.equal(eb.exp_avg_sq[key], snap[2][key]), (t, key)
            assert eb.settle("map") == 1 and eb.skipped_iterations == 1
        else:
            held += 1
            assert torch.equal(eb.buf['out6'], exact[i]['out6']), f"view {t}: bucketed lists render differently from exact lists"
            for key in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
                _cmp(eb.grads[key], exact[i]['grads'][key], f"view {t} on buckets of view {views[s][1]}: {key}", tol=1e-5)
    print(f"{held} views held on the learnt buckets, {flagged} raised the flag")
    assert held + flagged == len(views) - 1


# ------------------------------------------------------------------------------------------------------------------------------
# 4. Adam on rows outside the view
# ------------------------------------------------------------------------------------------------------------------------------

SEQUENCE = (4, 4, FORWARD_VIEW, 3)      # A, A, B, C: B and C leave ~15 % of A's rows out; ~20 % of the rows are first seen by B or C


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_adam_step(before, after, grad, t, lr, what, beta1=0.9, beta2=0.999, eps=1e-15):
    """Every element of one group against torch.optim.Adam restated in float64 on the engine's own inputs: parameter and moments
    before the step, the gradient it stored, its step count ``t``.  Returns the cases seen (element counts)."""
    p, m, v = (x.double().cpu().numpy() for x in before)
    p1, m1, v1 = (x.double().cpu().numpy() for x in after)
    g = grad.double().cpu().numpy()
    mr = beta1 * m + (1.0 - beta1) * g
    vr = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2s = 1.0 - beta1 ** t, np.sqrt(1.0 - beta2 ** t)
    denom = np.sqrt(vr) / bc2s + eps
    step = lr / bc1 * mr / denom
    pr = p - step
    untouched = (g == 0) & (m == 0) & (v == 0)
    momentum = (g == 0) & ~untouched
    first = (g != 0) & (m == 0) & (v == 0)
    # moments: a few float32 ulps of the terms they are formed from (m can cancel); the parameter: two ulps of itself + 1e-5 of the
    # step + what the moment's own rounding moves the step by
    tol_m = 4 * _ulp32(np.maximum(np.abs(beta1 * m), np.abs((1.0 - beta1) * g)))
    tol_v = 4 * _ulp32(vr)
    tol_p = 2 * _ulp32(p) + 1e-5 * np.abs(step) + lr / bc1 * tol_m / denom
    em, ev, ep = np.abs(m1 - mr), np.abs(v1 - vr), np.abs(p1 - pr)
    print(f"{what} (t {t}): {int(untouched.sum())} untouched, {int(momentum.sum())} on momentum only, {int(first.sum())} first gradients; "
          f"max err / tol: exp_avg {float((em / tol_m).max()):.2f}, exp_avg_sq {float((ev / tol_v).max()):.2f}, "
          f"param {float((ep / tol_p).max()):.2f}")
    assert (p1[untouched] == p[untouched]).all() and (m1[untouched] == 0).all() and (v1[untouched] == 0).all(), f"{what}: untouched rows moved"
    for name, err, tol in (("exp_avg", em, tol_m), ("exp_avg_sq", ev, tol_v), ("param", ep, tol_p)):
        bad = err > tol
        for case, sel in (("momentum-only", momentum), ("first gradient", first), ("other", ~(momentum | first | untouched))):
            assert not (bad & sel).any(), (f"{what}: {name} of {int((bad & sel).sum())} {case} elements off torch.optim.Adam, worst "
                                           f"err {float(err[bad & sel].max()):.3e} tol {float(tol[bad & sel][np.argmax(err[bad & sel])]):.3e}")
    assert not momentum.any() or (p1[momentum] != p[momentum]).mean() > 0.9, f"{what}: rows on momentum only did not move"
    return dict(untouched=int(untouched.sum()), momentum=int(momentum.sum()), first=int(first.sum()))


@pytest.mark.parametrize("path", ["F6 mapping step", "F8 loss_backward + adam_map", "mapping_batch"])
def test_adam_on_rows_outside_the_view(path):
    from splatam_amd import slam
    from splatam_amd.fused import FusedEngine
    params, variables, cam, k, views, c = _scene('small')
    cfg = slam.REPLICA_MAPPING
    capacity, _ = _probe(params, cam, [views[t - 1] for t in set(SEQUENCE)], cfg)
    p = _clone(params)
    eng = FusedEngine(p, cam, capacity=capacity)
    # the reference: torch.optim.Adam on the drop-in path's gradients, same views
    ref = _clone(params)
    opt = slam.initialize_optimizer(ref, cfg['lrs'], tracking=False)
    seen = {key: dict(untouched=0, momentum=0, first=0) for key in KEYS}
    snaps = []
    for step, t in enumerate(SEQUENCE, start=1):
        batch = [views[t - 1]] + ([views[FORWARD_VIEW - 1]] if path == "mapping_batch" and step == 4 else [])
        before = {key: (p[key].detach().clone(), eng.exp_avg[key].clone(), eng.exp_avg_sq[key].clone()) for key in KEYS}
        if path == "F6 mapping step":
            eng.mapping_iteration(*batch[0], cfg, keep_grads=True)
        elif path == "F8 loss_backward + adam_map":
            eng.loss_backward(*batch[0], cfg, tracking=False)
            eng.adam_map(cfg['lrs'])
        else:
            eng.mapping_batch(batch, cfg)
        torch.cuda.synchronize()
        assert not _flag(eng) and eng.map_step == step
        for key in KEYS:
            cases = _check_adam_step(before[key], (p[key].detach(), eng.exp_avg[key], eng.exp_avg_sq[key]), eng.grads[key], step,
                                     cfg['lrs'][key], f"{path} step {step} {key}")
            if key != "unnorm_rotations":
                for case in cases:
                    if case != "first" or step > 1:
                        seen[key][case] += cases[case]
        g_ref, _ = _reference_views(ref, variables, batch, cfg)
        for key in KEYS:
            ref[key].grad = sum(gv[key] for gv in g_ref) / len(batch)
        opt.step()
        opt.zero_grad(set_to_none=True)
        snaps.append({key: (p[key].detach().clone(), ref[key].detach().clone(), sum(gv[key] for gv in g_ref) / len(batch)) for key in KEYS})
    for key in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
        n = p[key].numel()
        print(f"{path} {key}: over the 4 steps {seen[key]} elements")
        assert seen[key]['momentum'] >= 0.02 * n and seen[key]['first'] >= 0.005 * n, (key, seen[key])
    # end to end, the rows that took steps 3 and 4 on momentum only: their two updates against torch.optim.Adam's on the reference
    # gradients (they depend on the moments of steps 1 and 2 alone)
    for key in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
        lr = cfg['lrs'][key]
        (pe2, pr2, _), (pe4, pr4, _) = snaps[1][key], snaps[3][key]
        g1, g3, g4 = snaps[0][key][2], snaps[2][key][2], snaps[3][key][2]
        mom = (g3 == 0) & (g4 == 0) & (g1.abs() > 1e-4 * g1.abs().max())
        de, dr = pe4 - pe2, pr4 - pr2
        diff = (de - dr).abs()[mom]
        print(f"{path} {key}: {int(mom.sum())} momentum-only elements with a significant first gradient, max |update - torch's| "
              f"{float(diff.max()):.3e} (lr {lr:g}), median |update| {float(dr.abs()[mom].median()):.3e}")
        assert int(mom.sum()) >= 0.01 * p[key].numel()
        assert float((diff > 0.05 * lr).float().mean()) < 5e-3, (key, float(diff.max()), lr)
