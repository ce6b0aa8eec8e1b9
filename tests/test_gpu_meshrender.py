"""The mesh render layer on the device (csrc/meshrender.hip through ``splatam_amd.mesh_render``), held to the header on the host
(tests/meshrender_math_shim.cpp), to the float64 restatement tests/meshrender_ref.py and to closed-form geometry:

  1. KERNEL = HEADER: ``render_depth`` bit-equal to the shim's plane on every case of ``meshrender_ref.render_cases``, at the default
     threshold between the triangle paths and with everything on either; two renders bit-equal; ``seen_counts`` equal to the shim's;
     ``splat_mesh_depth_compare`` against numpy on the kernel's own planes, twice the same bits.
  2. A CLOSED BOX FROM INSIDE at 96 x 64 (every triangle crosses z <= near and takes the wave path): no hole, every pixel within Z_BOUND
     of the closed form.  3. A CLOSED SPHERE FROM INSIDE at 67 x 45: no hole, every depth between the inscribed and circumscribed spheres'.
  4. THE SPHERE FROM OUTSIDE at 2 m (the one-lane path): holes and depths against the float64 ray caster, the nearest pixel at 2 - r.
  5. REJECTIONS.  6. / 7. SEEN COUNTS, frusta alone and with ``occlusion="self"`` planes.  8. / 9. ``cull_mesh``.  10. ``depth_l1``, and
  culling in the map's frame as ``run --cull`` does it.  11. ``sample_views``.  12. HANDS OFF a live engine.  13. THE COMMAND LINE.

Z_BOUND = 4 x the largest |z32 - z64| / z64 tests/test_meshrender_cpu.py observes on the host (2.2e-6; profiles/mesh_render.md 1)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshrender_ref as R
from test_meshrender_cpu import load_shim, shim_render, shim_seen

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = R.render_cases()
EPS = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def shim():
    return load_shim()


@pytest.fixture(scope="module")
def rendered():
    """name -> the device's plane of every case (numpy), rendered once."""
    from splatam_amd import mesh_render as MR
    out = {}
    for name, (v, f, w2c, intr, size) in CASES.items():
        out[name] = MR.render_depth(_dev(v), _dev(f), w2c, intr, size, near=R.NEAR).cpu().numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. kernel = header
@pytest.mark.parametrize("name", sorted(CASES))
def test_render_equals_the_header_bit_for_bit(shim, rendered, name):
    from splatam_amd import mesh_render as MR
    v, f, w2c, intr, size = CASES[name]
    want = shim_render(shim, v, f, w2c, intr, size)
    assert np.array_equal(rendered[name].view(np.uint32), want.view(np.uint32)), int((rendered[name] != want).sum())
    from splatam_amd import _capi
    dv, df = _dev(v), _dev(f)
    L = _capi.lib()
    chunk = torch.full((4, size[1], size[0]), -1.0, device="cuda")
    try:
        for k, split in enumerate((1, 1 << 30)):                         # every face by the wave; every face with a box by one lane
            assert L.splat_debug_option(5, split) in (0, 1)
            MR.render_depth(dv, df, w2c, intr, size, near=R.NEAR, out=chunk[k + 1])
            torch.cuda.synchronize()
            assert (chunk[0] == -1.0).all() and (chunk[k + 2:] == -1.0).all()     # a plane of a chunk: the planes before and after untouched
            assert np.array_equal(_bits(chunk[k + 1]), want.view(np.uint32)), split
        L.splat_debug_option(5, 0)
        assert L.splat_debug_option(6, 1) == 0                           # a filtering load in front of the atomic: the same plane
        MR.render_depth(dv, df, w2c, intr, size, near=R.NEAR, out=chunk[1])
        assert np.array_equal(_bits(chunk[1]), want.view(np.uint32))
    finally:
        L.splat_debug_option(5, 0)
        L.splat_debug_option(6, 0)
    again = MR.render_depth(dv, df, w2c, intr, size, near=R.NEAR)
    assert np.array_equal(_bits(again), rendered[name].view(np.uint32))


def test_compare_against_numpy_and_bit_reproducible(rendered):
    from splatam_amd import mesh_render as MR
    a, b = rendered["sphere-outside-96x64"], rendered["sphere-inside-96x64"].copy()
    b[5:9, 7:50] = 0.0                                                   # holes on either side, and pixels where both have depth
    a64, b64 = a.astype(np.float64).reshape(-1), b.astype(np.float64).reshape(-1)
    rows = torch.zeros(2, 8, dtype=torch.float64, device="cuda")
    for k in range(2):
        MR.compare_depth(_dev(a), _dev(b), rows[k])
    got = rows.cpu().numpy()
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))
    both = (a64 > 0) & (b64 > 0)
    d = np.abs(a64 - b64)
    n = a64.size
    assert got[0, 2] == both.sum() > 0 and got[0, 3] == (a64 == 0).sum() > 0 and got[0, 4] == (b64 == 0).sum() > 0 and got[0, 5] == n
    assert got[0, 6] == d.max() and got[0, 7] == 0
    assert abs(got[0, 0] - d.sum()) <= n * 2.0 ** -53 * d.sum() and abs(got[0, 1] - d[both].sum()) <= n * 2.0 ** -53 * d[both].sum()
    small = torch.zeros(8, dtype=torch.float64, device="cuda")           # fewer pixels than one workgroup has lanes
    MR.compare_depth(_dev(a.reshape(-1)[:37]), _dev(b.reshape(-1)[:37]), small)
    assert small[5].item() == 37 and abs(small[0].item() - d[:37].sum()) <= 37 * 2.0 ** -53 * max(d[:37].sum(), 1e-300)


# ---------------------------------------------------------------------------------------------------------------- 2. - 4. closed forms
def test_closed_box_from_inside(rendered):
    v, f, w2c, intr, size = CASES["box-inside-96x64"]
    got = rendered["box-inside-96x64"].astype(np.float64)
    want = R.box_depth(v.astype(np.float64).min(axis=0), v.astype(np.float64).max(axis=0), w2c, intr, size)
    assert (got > 0).all(), int((got == 0).sum())
    err = np.abs(got - want) / want
    print(f"box from inside: max relative error {err.max():.3e} (bound {R.Z_BOUND:.3e})")
    assert (err <= R.Z_BOUND).all()


def test_closed_sphere_from_inside_has_no_pinholes(rendered):
    v, f, w2c, intr, size = CASES["sphere-inside-67x45"]
    got = rendered["sphere-inside-67x45"].astype(np.float64)
    assert (got > 0).all(), int((got == 0).sum())
    inner = R.sphere_depth(R.inscribed_radius(v, f), w2c, intr, size)
    outer = R.sphere_depth(R.SPHERE_R * (1 + 2.0 ** -22), w2c, intr, size)
    assert (got >= inner * (1 - R.Z_BOUND)).all() and (got <= outer * (1 + R.Z_BOUND)).all()


@pytest.mark.parametrize("name", ["sphere-outside-67x45", "sphere-outside-96x64"])
def test_sphere_from_outside_against_the_ray_caster(rendered, name):
    v, f, w2c, intr, size = CASES[name]
    depth, fragile = R.oracle(name)
    assert fragile.mean() <= R.MAX_EXCUSED
    got = rendered[name].astype(np.float64)
    ok = ~fragile
    assert ((got == 0) == (depth == 0))[ok].all() and (got == 0)[ok].sum() == (depth == 0)[ok].sum() > 0
    both = ok & (depth > 0)
    err = np.abs(got - depth)[both] / depth[both]
    print(f"{name}: max relative error {err.max():.3e}, {int(fragile.sum())} fragile pixels")
    assert (err <= R.Z_BOUND).all()
    # the nearest pixel: every point of the mesh lies inside the sphere, so no depth is below 2 - r; the pixel nearest the axis looks at most
    # 0.71 pixel off it and meets the mesh no farther than the inscribed sphere is there, r_in's chord error e plus the sag x^2 / 2 r_in
    r_in = R.inscribed_radius(v, f)
    x = 0.71 / min(intr[0], intr[1]) * (2.0 - r_in)
    sag = 1.05 * x * x / (2 * r_in)
    nearest = got[got > 0].min()
    print(f"{name}: nearest depth {nearest:.6f}, 2 - r = {2.0 - R.SPHERE_R:.6f}, chord error {R.SPHERE_R - r_in:.2e}, sag {sag:.2e}")
    assert (2.0 - R.SPHERE_R) * (1 - R.Z_BOUND) <= nearest <= (2.0 - r_in + sag) * (1 + R.Z_BOUND), (nearest, r_in, sag)


# ---------------------------------------------------------------------------------------------------------------- 5. rejections
def test_rejections(rendered):
    from splatam_amd import _capi
    from splatam_amd import mesh_render as MR
    v, f, w2c, intr, size = CASES["sphere-outside-67x45"]
    behind = w2c.copy()
    behind[2, :] *= -1
    assert (MR.render_depth(_dev(v), _dev(f), behind, intr, size) == 0).all()
    v2 = np.concatenate((v, np.array([[np.nan, 0, 0], [0, 0, 0.1], [0.1, 0, 0.1]], dtype=np.float32)))
    f2 = np.concatenate((np.array([[0, 1, len(v2)], [-1, 0, 1], [len(v), len(v) + 1, len(v) + 2]], dtype=np.int32), f))
    got = MR.render_depth(_dev(v2), _dev(f2), w2c, intr, size, near=R.NEAR)
    assert np.array_equal(_bits(got), rendered["sphere-outside-67x45"].view(np.uint32))
    # no faces, no vertices: a plane of zeros, as documented
    for vv, ff in ((v[:0], f[:0]), (v, f[:0]), (v[:0], f)):
        out = torch.full((size[1], size[0]), 7.0, device="cuda")
        MR.render_depth(_dev(vv.reshape(-1, 3)), _dev(ff.reshape(-1, 3)), w2c, intr, size, out=out)
        assert (out == 0).all()
    with pytest.raises(ValueError):
        MR.render_depth(_dev(v), _dev(f), w2c, intr, size, near=0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MR.render_depth(torch.from_numpy(v), torch.from_numpy(f), w2c, intr, size)
    with pytest.raises(RuntimeError):
        MR.render_depth(_dev(v), _dev(f), w2c, intr, size, out=torch.empty(3, 3, device="cuda"))
    L = _capi.lib()
    view = MR._view(intr, size)
    view.w2c = _dev(w2c).data_ptr()
    plane = torch.full((size[1], size[0]), 7.0, device="cuda")
    assert L.splat_mesh_depth(None, 0, None, 0, view, None, None) == 1                       # nowhere to render to
    view.near_z = 0.0
    assert L.splat_mesh_depth(None, 0, None, 0, view, plane.data_ptr(), None) == 1
    view.near_z, view.fx = 0.01, 0.0
    assert L.splat_mesh_depth(None, 0, None, 0, view, plane.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert (plane == 7.0).all()                                          # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- 6. / 7. seen counts
SEEN_SIZE, SEEN_F = (67, 45), 57.0


@pytest.fixture(scope="module")
def ring():
    v, f = R.sphere()
    return v, f, R.ring_views(8, 2.0), R.pinhole(*SEEN_SIZE, SEEN_F)


def test_seen_counts_frusta_alone(shim, ring):
    from splatam_amd import mesh_render as MR
    v, f, views, intr = ring
    want, excused = R.seen_counts(v, views, intr, SEEN_SIZE)
    assert excused.mean() <= R.MAX_EXCUSED
    got = MR.seen_counts(_dev(v), _dev(views), intr, SEEN_SIZE).cpu().numpy()
    assert np.array_equal(got, shim_seen(shim, v, views, intr, SEEN_SIZE))
    assert np.array_equal(got[~excused], want[~excused]) and got.max() == 8      # the whole sphere lies inside every view's frustum
    tight = R.pinhole(*SEEN_SIZE, 4 * SEEN_F)                            # a longer lens: the frusta cut the sphere
    want, excused = R.seen_counts(v, views, tight, SEEN_SIZE)
    assert excused.mean() <= R.MAX_EXCUSED
    got = MR.seen_counts(_dev(v), _dev(views), tight, SEEN_SIZE).cpu().numpy()
    assert np.array_equal(got, shim_seen(shim, v, views, tight, SEEN_SIZE)) and np.array_equal(got[~excused], want[~excused])
    assert 0 < (got == 0).sum() < len(v)


def test_seen_counts_with_occlusion(shim, ring):
    from splatam_amd import mesh_render as MR
    v, f, views, intr = ring
    dv, df = _dev(v), _dev(f)
    planes = torch.stack([MR.render_depth(dv, df, m, intr, SEEN_SIZE, near=R.NEAR) for m in views])
    eps = 0.03
    got = MR.seen_counts(dv, _dev(views), intr, SEEN_SIZE, depth=planes, eps=eps).cpu().numpy()
    assert np.array_equal(got, shim_seen(shim, v, views, intr, SEEN_SIZE, depth=planes.cpu().numpy(), eps=eps))
    want, excused = R.seen_counts(v, views, intr, SEEN_SIZE, depth=planes.cpu().numpy(), eps=eps)
    assert excused.mean() <= R.MAX_EXCUSED and np.array_equal(got[~excused], want[~excused])
    free = MR.seen_counts(dv, _dev(views), intr, SEEN_SIZE).cpu().numpy()
    assert (got <= free).all() and (got < free).any()
    # the far hemisphere of every view -- every vertex on the side of the centre away from the camera -- is never seen from that view:
    # the ray to such a vertex first crosses a chord of the sphere of 0.2 m and more, eps is 0.03
    for k, m in enumerate(views):
        one = MR.seen_counts(dv, _dev(m), intr, SEEN_SIZE, depth=planes[k:k + 1].contiguous(), eps=eps).cpu().numpy()
        origin = -(m[:3, :3].astype(np.float64).T @ m[:3, 3].astype(np.float64))
        far = v.astype(np.float64) @ origin < 0
        assert far.sum() > 1900 and (one[far] == 0).all(), (k, int(one[far].sum()))
    edge5 = MR.seen_counts(dv, _dev(views), intr, SEEN_SIZE, edge=5, depth=planes, eps=eps).cpu().numpy()
    assert (edge5 <= got).all()
    acc = torch.zeros(len(v), dtype=torch.int32, device="cuda")
    for s in range(0, 8, 3):
        MR.seen_counts(dv, _dev(views[s:s + 3]), intr, SEEN_SIZE, depth=planes[s:s + 3].contiguous(), eps=eps, out=acc)
    assert np.array_equal(acc.cpu().numpy(), got)
    # ... and cull_mesh(occlusion="self") counts the same: what survives is what these counts say
    culled = MR.cull_mesh((dv, df, None), views, intr, SEEN_SIZE, occlusion="self", eps=eps, chunk=3)
    keep = (got > 0)[f].all(axis=1)
    assert culled.faces.shape[0] == keep.sum() and 0 < keep.sum()


# ---------------------------------------------------------------------------------------------------------------- 8. / 9. cull_mesh
def _cube_view():
    return R.look_at((1.3, 0.07, 0.05), (0.3, 0.0, 0.0), roll=0.3), R.pinhole(96, 64, 330.0), (96, 64)


def test_cull_mesh_cuts_a_cube():
    from splatam_amd import mesh_render as MR
    v, f, c = R.grid_cube()
    w2c, intr, size = _cube_view()
    seen, excused = R.seen_counts(v, w2c[None], intr, size)
    assert not excused.any()
    want_all, want_any = (seen > 0)[f].all(axis=1), (seen > 0)[f].any(axis=1)
    assert 0 < want_all.sum() < want_any.sum() < len(f)
    got = MR.cull_mesh((v, f, c), w2c[None], intr, size)
    gv, gf, gc = (t.cpu().numpy() for t in got)
    assert len(gf) == want_all.sum() and gf.min() == 0 and gf.max() == len(gv) - 1 and gf.dtype == np.int32
    assert np.array_equal(gv[gf], v[f[want_all]])                        # the same triangles, in the same order
    used = np.unique(f[want_all])
    assert np.array_equal(gv, v[used]) and np.array_equal(gc, c[used])   # renumbered densely in order, colours with their vertices
    anyv, anyf, _ = (t.cpu().numpy() for t in MR.cull_mesh((_dev(v), _dev(f), _dev(c)), w2c[None], intr, size, rule="any"))
    assert np.array_equal(anyv[anyf], v[f[want_any]])
    kept = {tuple(map(tuple, t)) for t in gv[gf]}
    assert kept <= {tuple(map(tuple, t)) for t in anyv[anyf]}
    with pytest.raises(ValueError):
        MR.cull_mesh((v, f, c), w2c[None], intr, size, rule="most")


def test_cull_mesh_everything_and_nothing():
    from splatam_amd import mesh_render as MR
    v, f, c = R.grid_cube()
    w2c, intr, size = _cube_view()
    wide = (30.0, 30.0, intr[2], intr[3])
    everything = MR.cull_mesh((v, f, c), w2c[None], wide, size)
    assert np.array_equal(everything.vertices.cpu().numpy(), v) and np.array_equal(everything.faces.cpu().numpy(), f)
    assert np.array_equal(everything.colors.cpu().numpy(), c)
    away = w2c.copy()
    away[2, :] *= -1
    nothing = MR.cull_mesh((v, f, c), away[None], intr, size)
    assert tuple(nothing.vertices.shape) == (0, 3) and tuple(nothing.faces.shape) == (0, 3) and tuple(nothing.colors.shape) == (0, 3)
    none = MR.cull_mesh((v, f, None), np.zeros((0, 4, 4)), intr, size)
    assert none.faces.shape[0] == 0 and none.colors is None


# ---------------------------------------------------------------------------------------------------------------- 10. depth_l1
def _centre_views():
    """Three views from the centre; the first looks at the sphere mesh's face 0, which lies at +x."""
    return np.stack([R.look_at((0.0, 0.0, 0.0), t, roll=a) for t, a in (((1.0, 0.03, 0.02), 0.3), ((-0.4, 1.0, 0.5), 1.7), ((0.2, -0.3, -1.0), 2.9))])


def test_depth_l1():
    from splatam_amd import mesh_render as MR
    from tests.util import rigid_w2c
    import meshscore_ref as S
    size, intr = (67, 45), R.pinhole(67, 45, 40.0)
    views = _centre_views()
    rec, gt = S.sphere_mesh(4, 0.45), S.sphere_mesh(4, 0.47)
    same = MR.depth_l1(rec, rec, views, intr, size)
    assert same["depth_l1_cm"] == 0.0 and same["depth_l1_valid_cm"] == 0.0 and same["holes_gt"] == same["holes_rec"] == 0 and same["views"] == 3
    # From the centre the depth along the ray d = (dx, dy, 1) is rho / |d|, rho the mesh's radius along it: r - e_mesh <= rho <= r with
    # e_mesh = r - r_in the chord error (profiles/mesh_score.md 1).  So d_gt - d_rec lies in [0.02 - e_gt, 0.02 + e_rec] / |d|, and a view's
    # mean in that band times m = mean 1 / |d| over the pixels -- computed, the same for every view.
    e_rec, e_gt = 0.45 - R.inscribed_radius(*rec), 0.47 - R.inscribed_radius(*gt)
    got = MR.depth_l1(rec, gt, views, intr, size)
    m = float(np.mean(1.0 / np.linalg.norm(R.rays(intr, size), axis=1)))
    print(f"depth L1 {got['depth_l1_valid_cm']:.5f} cm, chord errors {100 * e_rec:.5f} / {100 * e_gt:.5f} cm, mean 1/|d| {m:.5f}")
    assert (2.0 - 100 * e_gt) * m * (1 - 1e-6) <= got["depth_l1_valid_cm"] <= (2.0 + 100 * e_rec) * m * (1 + 1e-6)
    assert got["depth_l1_cm"] == got["depth_l1_valid_cm"] and got["holes_gt"] == got["holes_rec"] == 0
    # ... and through a long lens, where |d| = 1 to within 1.4e-4, the band is [2 - e, 2 + e] cm itself, e = e_rec + e_gt
    long_lens = R.pinhole(*size, 2000.0)
    tele = MR.depth_l1(rec, gt, views, long_lens, size)
    e = 100 * (e_rec + e_gt)
    print(f"long lens: depth L1 {tele['depth_l1_valid_cm']:.5f} cm, e = {e:.5f} cm")
    assert 2.0 - e <= tele["depth_l1_valid_cm"] <= 2.0 + e and tele["holes_gt"] == tele["holes_rec"] == 0
    # a face removed: the hole is charged its full depth
    holed = MR.depth_l1((rec[0], rec[1][1:]), gt, views, intr, size)
    assert holed["holes_rec"] > 0 and holed["holes_gt"] == 0 and holed["depth_l1_cm"] > holed["depth_l1_valid_cm"] > 0
    # a rigid motion undone by `transform`: the vertices come back within one float32 rounding of their magnitude each way
    M = rigid_w2c(0.7, (1.0, -2.0, 0.5), (0.3, -0.2, 0.5)).astype(np.float64)
    moved = (rec[0].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    back = MR.depth_l1((moved, rec[1]), gt, views, intr, size, transform=np.linalg.inv(M))
    bound = 8 * EPS * float(np.abs(moved).max()) * 100.0 * 4             # cm; depth moves at most 1 / cos(grazing) <= 4 times the vertex
    assert abs(back["depth_l1_valid_cm"] - got["depth_l1_valid_cm"]) <= bound, (back, got, bound)
    assert back["holes_rec"] == 0
    with pytest.raises(ValueError):
        MR.depth_l1(rec, gt, np.zeros((0, 4, 4)), intr, size)


def test_culling_in_the_map_frame_takes_the_ground_truth_there():
    """What ``run --cull`` does: the reconstruction and the poses live in the map's frame, the ground truth in the world's; the inverse
    of the first frame's camera-to-world pose brings it over.  Two concentric spheres seen from their centre keep the same faces (the
    same subdivision, vertices on the same rays), so accuracy and completion stay the 2 cm between them; with the transform applied the
    wrong way round the spheres would lie 2 x 0.6 m apart."""
    from splatam_amd import mesh_score as S
    from tests.util import rigid_w2c
    import meshscore_ref as SR
    rec, gt_map = SR.sphere_mesh(3, 0.45), SR.sphere_mesh(3, 0.47)
    T = rigid_w2c(0.7, (1.0, -2.0, 0.5), (0.3, -0.2, 0.5)).astype(np.float64)          # the first frame's camera-to-world pose
    gt_world = ((gt_map[0].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32), gt_map[1], None)
    poses = np.stack([R.look_at((0.0, 0.0, 0.0), t) for t in ((1, 0, 0), (0, 1, 0), (0, 0, 1))])        # in the map's frame
    intr, size = (30.0, 30.5, 33.1, 22.1), (67, 45)
    got = S.score_culled_in_map_frame((rec[0], rec[1], None), gt_world, poses, intr, size, gt_transform=T, samples=20_000)
    whole = S.score_mesh((rec[0], rec[1], None), gt_world, samples=20_000, transform=T)
    print({k: (got[k], whole[k]) for k in ("accuracy_cm", "completion_cm", "completion_ratio")})
    e = 100 * max(0.45 - R.inscribed_radius(*rec), 0.47 - R.inscribed_radius(*gt_map))
    assert 2.0 - e <= got["accuracy_cm"] <= 2.0 + e and 2.0 - e <= got["completion_cm"] <= 2.0 + e
    k = np.array([[30.0, 0, 33.1], [0, 30.5, 22.1], [0, 0, 1]])
    assert S.score_culled_in_map_frame((rec[0], rec[1], None), gt_world, poses, k, size, gt_transform=T, samples=20_000) == got
    away = poses.copy()
    away[:, 2, :] *= -1
    away[:, :3, 3] = (0.0, 0.0, -5.0)                                                  # every camera 5 m off, looking away
    with pytest.raises(ValueError, match="see nothing of the reconstruction"):
        S.score_culled_in_map_frame((rec[0], rec[1], None), gt_world, away, intr, size, gt_transform=T)


# ---------------------------------------------------------------------------------------------------------------- 11. sample_views
def test_sample_views():
    from splatam_amd import mesh_render as MR
    v, f = R.box()
    size, intr = (67, 45), R.pinhole(67, 45, 40.0)
    a = MR.sample_views((v, f, None), 5, intr, size, seed=3, chunk=4)
    b = MR.sample_views((v, f, None), 5, intr, size, seed=3, chunk=7)
    assert tuple(a.shape) == (5, 4, 4) and torch.equal(a, b) and not torch.equal(a, MR.sample_views((v, f, None), 5, intr, size, seed=4))
    for m in a:
        assert (MR.render_depth(_dev(v), _dev(f), m, intr, size) > 0).all()
    tri = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32), None)
    with pytest.raises(ValueError, match="0 of 3 hole-free views after 12 candidates"):
        MR.sample_views(tri, 3, intr, size, max_tries=12, chunk=5)


# ---------------------------------------------------------------------------------------------------------------- 12. hands off
def test_cull_and_depth_l1_leave_a_live_engine_untouched():
    from splatam_amd import mesh as M
    from splatam_amd import mesh_render as MR
    from splatam_amd.fused import PARAM_ORDER
    from test_gpu_meshscore import H, W, _engine
    eng, intr = _engine()
    main = eng._camera
    with torch.no_grad():
        mesh = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, voxel_size=0.05, sil_thres=0.5, depth_max=6.0)
    torch.cuda.synchronize()
    assert mesh.faces.shape[0] > 500

    def snapshot():
        s = {f"param {n}": eng.params[n].detach().clone() for n in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        s.update({f"exp_avg {n}": eng.exp_avg[n].clone() for n in PARAM_ORDER})
        s.update({f"exp_avg_sq {n}": eng.exp_avg_sq[n].clone() for n in PARAM_ORDER})
        s.update({f"variables {n}": eng.variables[n].clone() for n in ('max_2D_radius', 'timestep', 'means2D_gradient_accum', 'denom')})
        s.update({f"rendered {i}": t.clone() for i, t in enumerate(eng.rendered())})
        s.update({f"main {n}": main.buf[n].clone() for n in ('status', 'd_cam')})
        s.update({f"mesh {n}": getattr(mesh, n).clone() for n in ("vertices", "faces", "colors")})
        return s
    before = snapshot()
    views = np.stack([np.eye(4), R.rotated((0.05, 0.0, 0.02), 0.1, (0, 1, 0.2))])
    culled = MR.cull_mesh(mesh, views, intr, (W, H), occlusion="self")
    score = MR.depth_l1(culled, mesh, views, intr, (W, H))
    same = MR.depth_l1(mesh, mesh, views, intr, (W, H))
    torch.cuda.synchronize()
    after = snapshot()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    for name, t in before.items():
        assert torch.equal(bits(t), bits(after[name])), name
    assert eng._camera is main
    assert 0 < culled.faces.shape[0] <= mesh.faces.shape[0] and score["views"] == 2 and score["holes_rec"] >= score["holes_gt"]
    assert same["depth_l1_cm"] == 0.0 and same["holes_rec"] == same["holes_gt"] < 2 * W * H


# ---------------------------------------------------------------------------------------------------------------- 13. command line
def test_the_command_culls_and_adds_depth_l1(tmp_path):
    from splatam_amd import mesh_render as MR
    from splatam_amd import mesh_score as S
    from splatam_amd.export import save_mesh_ply
    import meshscore_ref as SR
    # the ground truth: a sphere, and around it a shell that no pose inside can see -- what occlusion-aware culling is there to remove
    rec, inner, shell = SR.sphere_mesh(3, 0.45), SR.sphere_mesh(3, 0.47), SR.sphere_mesh(3, 0.8)
    gt = (np.concatenate((inner[0], shell[0])), np.concatenate((inner[1], shell[1] + len(inner[0]))))
    save_mesh_ply(str(tmp_path / "rec.ply"), *rec)
    save_mesh_ply(str(tmp_path / "gt.ply"), *gt)
    dirs = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))    # a cube map from the centre
    w2c = np.stack([R.look_at((0.0, 0.0, 0.0), t) for t in dirs]).astype(np.float64)
    np.savetxt(str(tmp_path / "traj.txt"), np.linalg.inv(w2c).reshape(6, 16))
    root = os.path.dirname(HERE)
    base = [sys.executable, "-m", "splatam_amd.mesh_score", str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "--samples", "5000", "--seed", "3"]
    new = ["--cull-poses", str(tmp_path / "traj.txt"), "--cull-size", "67x45", "--cull-intrinsics", "20", "20.5", "33.1", "22.1", "--occlusion",
           "--depth-l1", "4"]
    run = lambda args: subprocess.run(args, cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE,  # noqa: E731
                                      stderr=subprocess.PIPE, text=True)
    done = run(base + new)
    assert done.returncode == 0, done.stdout + done.stderr
    intr, size = (20.0, 20.5, 33.1, 22.1), (67, 45)
    poses = MR.load_poses(str(tmp_path / "traj.txt"))
    score = S.score_with_views(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), samples=5000, seed=3, cull_w2c=poses, intrinsics=intr, size=size,
                               occlusion=True, depth_l1_views=4)
    assert done.stdout.strip() == S.format_score(score).strip(), done.stdout
    lines = done.stdout.splitlines()
    assert len(lines) == 5 and lines[4].startswith("Depth L1: ") and score["views"] == 4
    # what the functions return, put together by hand
    g0 = MR.to_device_mesh(str(tmp_path / "gt.ply"))
    planes = torch.stack([MR.render_depth(g0.vertices, g0.faces, m, intr, size) for m in poses])
    r = MR.cull_mesh(str(tmp_path / "rec.ply"), poses, intr, size, occlusion=planes)
    g = MR.cull_mesh(g0, poses, intr, size, occlusion="self")
    assert g.faces.shape[0] == len(inner[1]) and r.faces.shape[0] == len(rec[1])      # the shell is gone, the rest is whole
    by_hand = S.score_mesh(r, g, samples=5000, seed=3)
    by_hand.update(MR.depth_l1(r, g, MR.sample_views(g, 4, intr, size, seed=3), intr, size))
    assert by_hand == score
    assert score["depth_l1_cm"] == score["depth_l1_valid_cm"] > 0.5 and 1.5 < score["completion_cm"] < 2.5     # (2 cm apart; the shell: 33 cm)
    # without the new options: format_score of score_mesh, byte for byte, and no fifth line
    plain = run(base)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    want = S.score_mesh(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), samples=5000, seed=3)
    assert "depth_l1_cm" not in want and plain.stdout == S.format_score(want) + "\n" and len(plain.stdout.splitlines()) == 4
    assert want["completion_cm"] > 10.0
    refused = run(base + ["--occlusion"])
    assert refused.returncode != 0 and "--occlusion needs --cull-poses" in refused.stderr
