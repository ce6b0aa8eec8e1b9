"""The mesh render layer without a GPU: splatam_amd/csrc/meshrender_math.h compiled for the host (tests/meshrender_math_shim.cpp: the
loop bodies of the kernels of csrc/meshrender.hip) against the float64 restatement tests/meshrender_ref.py.

1. RENDER: on every case of ``meshrender_ref.render_cases`` (a closed box and a closed sphere from inside, the sphere from outside, each
   at 96 x 64 and 67 x 45) the oracle flags at most 1 % of the pixels as fragile -- asserted on the oracle's flags before the header's
   plane is looked at -- and elsewhere the header has a hole exactly where the oracle has one and |z32 - z64| / z64 <= Z_BOUND, 4 x the
   largest value observed over these cases (printed per case; profiles/mesh_render.md 1).  The plane does not depend on the threshold
   between the two triangle paths (1, the default, everything small), and both kinds of face occur.
2. CLOSED MESHES: no hole from inside the box and the sphere (the antisymmetric edge planes), the box within Z_BOUND of its closed form.
3. SEEN: the header's counts equal the float64 brute force except on the vertices the oracle excuses (at most 1 %, asserted first), without
   planes, with rendered planes and eps, and with a margin; counts accumulate over chunks of views.
4. REJECTIONS and PLUMBING: faces out of range, NaN vertices, a mesh behind the camera; the binding declares the entry points and the
   header documents them; ``mesh_render``'s host-side helpers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import meshrender_ref as R
from tests.util import host_shim

F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def load_shim():
    lib = host_shim("meshrender_math_shim", "meshrender_math.h")
    lib.mr_default_split.restype = C.c_int
    lib.mr_render.restype = C.c_int
    lib.mr_render.argtypes = [F32P, C.c_int32, I32P, C.c_int32, F32P, F32P, C.c_int, C.c_int, C.c_float, C.c_int, F32P, I32P,
                              C.POINTER(C.c_longlong)]
    lib.mr_seen_counts.restype = C.c_int
    lib.mr_seen_counts.argtypes = [F32P, C.c_int32, F32P, C.c_int32, F32P, C.c_int, C.c_int, C.c_int, F32P, C.c_float, I32P]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None and a.size else None


def shim_render(shim, vertices, faces, w2c, intr, size, near=R.NEAR, split=0, kinds=False):
    v, f = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    m, k = np.ascontiguousarray(w2c, np.float32).reshape(16), np.array(intr, dtype=np.float32)
    depth, kind, tested = np.empty((size[1], size[0]), dtype=np.float32), np.zeros(max(len(f), 1), dtype=np.int32), C.c_longlong(0)
    assert shim.mr_render(_p(v, F32P), len(v), _p(f, I32P), len(f), _p(m, F32P), _p(k, F32P), size[0], size[1], near, split, _p(depth, F32P),
                          _p(kind, I32P), C.byref(tested)) == 0
    return (depth, kind[:len(f)], tested.value) if kinds else depth


def shim_seen(shim, vertices, w2c, intr, size, edge=0, depth=None, eps=0.0, seen=None):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    m, k = np.ascontiguousarray(w2c, np.float32).reshape(-1, 16), np.array(intr, dtype=np.float32)
    d = None if depth is None else np.ascontiguousarray(depth, np.float32)
    seen = np.zeros(len(v), dtype=np.int32) if seen is None else seen
    assert shim.mr_seen_counts(_p(v, F32P), len(v), _p(m, F32P), len(m), _p(k, F32P), size[0], size[1], edge, _p(d, F32P) if d is not None else None,
                               eps, _p(seen, I32P)) == 0
    return seen


def relative_error(got, depth, fragile):
    """The largest |z32 - z64| / z64 over the pixels that are not fragile; asserts that holes agree there."""
    ok = ~fragile
    assert ((got == 0) == (depth == 0))[ok].all(), f"{int((((got == 0) != (depth == 0)) & ok).sum())} pixels differ in being a hole"
    both = ok & (depth > 0)
    return float((np.abs(got.astype(np.float64) - depth) / np.where(both, depth, 1.0))[both].max()) if both.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- 1. render
@pytest.mark.parametrize("name", sorted(R.render_cases()))
def test_header_against_the_ray_caster(shim, name):
    v, f, w2c, intr, size = R.render_cases()[name]
    depth, fragile = R.oracle(name)
    assert fragile.mean() <= R.MAX_EXCUSED, f"{name}: the oracle excuses {fragile.mean():.4f} of the pixels"
    got, kinds, tested = shim_render(shim, v, f, w2c, intr, size, kinds=True)
    err = relative_error(got, depth, fragile)
    print(f"{name}: max |z32 - z64| / z64 = {err:.3e} ({int(fragile.sum())} of {fragile.size} pixels fragile; "
          f"{int((kinds == 1).sum())} small, {int((kinds == 2).sum())} large, {int((kinds == 0).sum())} rejected faces; {tested} pixel tests)")
    assert R.Z_BOUND is not None and abs(R.Z_BOUND - 4 * R.Z_OBSERVED) <= 1e-12 * R.Z_BOUND
    assert err <= R.Z_BOUND, (name, err)
    for split in (1, 1 << 30):                                           # everything large; everything with a known box small
        other, _, _ = shim_render(shim, v, f, w2c, intr, size, split=split, kinds=True)
        assert np.array_equal(other.view(np.uint32), got.view(np.uint32)), split
    if name.startswith("box-inside"):
        assert not (kinds == 1).any() and (kinds == 2).sum() >= 3        # a room from inside: every triangle in view crosses z <= near
    if name.startswith("sphere-outside"):
        assert (kinds == 1).sum() > 0.4 * len(f) and (kinds == 0).sum() == 0


def test_default_split_is_the_documented_one(shim):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "splat_hip.h")).read()
    assert shim.mr_default_split() == 16 and "holds at most 16 pixels" in header and "0 = the library's 16" in header


# ---------------------------------------------------------------------------------------------------------------- 2. closed meshes
@pytest.mark.parametrize("size", sorted(R.SIZES))
def test_closed_meshes_have_no_pinholes(shim, size):
    tag = f"{size[0]}x{size[1]}"
    v, f, w2c, intr, _ = R.render_cases()[f"box-inside-{tag}"]
    got = shim_render(shim, v, f, w2c, intr, size).astype(np.float64)
    want = R.box_depth(v.astype(np.float64).min(axis=0), v.astype(np.float64).max(axis=0), w2c, intr, size)
    assert (got > 0).all()
    assert (np.abs(got - want) <= R.Z_BOUND * want + 2.0 ** -24).all(), float((np.abs(got - want) / want).max())
    v, f, w2c, intr, _ = R.render_cases()[f"sphere-inside-{tag}"]
    got = shim_render(shim, v, f, w2c, intr, size).astype(np.float64)
    assert (got > 0).all()
    inner, outer = R.sphere_depth(R.inscribed_radius(v, f), w2c, intr, size), R.sphere_depth(R.SPHERE_R * (1 + 2.0 ** -22), w2c, intr, size)
    assert (got >= inner * (1 - R.Z_BOUND)).all() and (got <= outer * (1 + R.Z_BOUND)).all()


def test_shared_edge_planes_are_exact_negatives(shim):
    """A ray through a shared edge: the pixel whose ray passes exactly through the diagonal of a square made of two triangles is covered,
    whichever way round the triangles name the edge."""
    v = np.array([[-3, -3, 2], [3, -3, 2], [3, 3, 2], [-3, 3, 2]], dtype=np.float32)
    intr, size = (8.0, 8.0, 8.0, 8.0), (17, 17)                          # pixel (i, i) looks along the diagonal exactly
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 1, 2], [2, 0, 3]], [[2, 1, 0], [0, 2, 3]], [[1, 2, 0], [3, 0, 2]]):
        got = shim_render(shim, v, np.array(faces, dtype=np.int32), np.eye(4, dtype=np.float32), intr, size)
        assert (got == 2.0).all(), faces


# ---------------------------------------------------------------------------------------------------------------- 3. seen
def _seen_case():
    v, f = R.sphere()
    size = (67, 45)
    return v, f, R.ring_views(8, 2.0), R.pinhole(*size, 57.0), size


@pytest.mark.parametrize("mode", ["frusta", "planes", "planes-edge"])
def test_seen_counts_against_the_brute_force(shim, mode):
    v, f, views, intr, size = _seen_case()
    edge, eps = (5, 0.03) if mode == "planes-edge" else (0, 0.03)
    planes = None
    if mode != "frusta":
        planes = np.stack([shim_render(shim, v, f, m, intr, size) for m in views])
    want, excused = R.seen_counts(v, views, intr, size, edge=edge, depth=planes, eps=eps)
    assert excused.mean() <= R.MAX_EXCUSED, excused.mean()
    got = shim_seen(shim, v, views, intr, size, edge=edge, depth=planes, eps=eps)
    print(f"{mode}: {int(excused.sum())} of {len(v)} vertices excused, {int((got != want).sum())} differ, counts {int(got.min())}..{int(got.max())}")
    assert np.array_equal(got[~excused], want[~excused])
    assert got.max() > 0 and (got.max() <= len(views))
    if planes is not None:                                               # occlusion can only take away, and chunks accumulate
        free = shim_seen(shim, v, views, intr, size, edge=edge)
        assert (got <= free).all() and (got < free).any()
        acc = np.zeros(len(v), dtype=np.int32)
        for s in range(0, len(views), 3):
            shim_seen(shim, v, views[s:s + 3], intr, size, edge=edge, depth=planes[s:s + 3], eps=eps, seen=acc)
        assert np.array_equal(acc, got)


# ---------------------------------------------------------------------------------------------------------------- 4. rejections, plumbing
def test_rejected_faces_render_nothing_and_disturb_nothing(shim):
    v, f, w2c, intr, size = R.render_cases()["sphere-outside-67x45"]
    base = shim_render(shim, v, f, w2c, intr, size)
    v2 = np.concatenate((v, np.array([[np.nan, 0, 0], [0, 0, 0.1], [0.1, 0, 0.1]], dtype=np.float32)))
    f2 = np.concatenate((f, np.array([[0, 1, len(v2)], [-1, 0, 1], [len(v), len(v) + 1, len(v) + 2]], dtype=np.int32)))
    got, kinds, _ = shim_render(shim, v2, f2, w2c, intr, size, kinds=True)
    assert np.array_equal(got, base) and (kinds[-3:] == 0).all()
    behind = w2c.copy()
    behind[2, :] *= -1                                                   # the mesh at z < 0
    assert (shim_render(shim, v, f, behind, intr, size) == 0).all()
    assert (shim_render(shim, v[:0], f[:0], w2c, intr, size) == 0).all()


def test_header_under_address_and_ub_sanitizers(tmp_path):
    """The shim's host functions as a stand-alone program (its own main) built with -fsanitize=address,undefined: a mesh with an
    out-of-range face, a NaN and an infinite vertex, a triangle through the camera centre, one across z = 0, a 1 x 1 image, zero views.
    Any sanitizer report or wrong answer is a non-zero exit.  The runtimes are linked statically; nothing loaded into python is
    involved."""
    exe = str(tmp_path / "meshrender_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DMESHRENDER_SHIM_MAIN", "-o", exe,
                           os.path.join(os.path.dirname(__file__), "meshrender_math_shim.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout


def test_binding_and_header_name_the_entry_points():
    from splatam_amd import _capi
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "splat_hip.h")).read()
    L = _capi.lib()
    for name in ("splat_mesh_depth", "splat_mesh_seen", "splat_mesh_depth_compare"):
        assert hasattr(L, name) and name in _capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert L.splat_sizeof(b"SplatMeshView") == C.sizeof(_capi.SplatMeshView) > 0
    assert _capi.SPLAT_MESH_COMPARE_PARTIALS == 6 * int(re.search(r"#define SPLAT_MESH_COMPARE_ROWS (\d+)", header).group(1))
    assert L.splat_abi_version() == 17
    # refusals need no device: nothing is launched
    view = _capi.SplatMeshView()
    assert L.splat_mesh_depth(None, 0, None, 0, None, None, None) == 1
    assert L.splat_mesh_depth(None, 0, None, 0, C.byref(view), 1 << 12, None) == 1          # a zero-size image
    view.width, view.height, view.fx, view.fy, view.near_z, view.w2c = 8, 8, 1.0, 1.0, 0.0, 1 << 12
    assert L.splat_mesh_depth(None, 0, None, 0, C.byref(view), 1 << 12, None) == 1          # near = 0
    view.near_z = 0.01
    assert L.splat_mesh_depth(None, 3, 1 << 12, 1, C.byref(view), 1 << 12, None) == 1       # vertices promised, none given
    assert L.splat_mesh_seen(1 << 12, 3, C.byref(view), 1 << 12, 1, -1, None, 0.0, 1 << 12, None) == 1     # a negative margin
    assert L.splat_mesh_seen(1 << 12, 3, C.byref(view), None, 1, 0, None, 0.0, 1 << 12, None) == 1         # views promised, none given
    assert L.splat_mesh_depth_compare(None, None, 4, 1 << 12, 1 << 12, None) == 1


def test_host_side_helpers(tmp_path):
    from splatam_amd import mesh_render as MR
    assert MR.parse_size("1200x680") == (1200, 680)
    assert MR._intrinsics(np.array([[600.0, 0, 599.5], [0, 601.0, 339.5], [0, 0, 1]])) == MR._intrinsics((600.0, 601.0, 599.5, 339.5))
    with pytest.raises(ValueError):
        MR._intrinsics((0.0, 600.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        MR.parse_size("1200")
    c2w = np.stack([np.linalg.inv(m.astype(np.float64)) for m in R.ring_views(5, 2.0)])
    path = tmp_path / "traj.txt"
    np.savetxt(path, c2w.reshape(5, 16))
    w2c = MR.load_poses(path, every=2)
    assert w2c.shape == (3, 4, 4) and np.allclose(w2c[1], np.linalg.inv(c2w[2]), atol=1e-12)
    with pytest.raises(ValueError, match="16 numbers"):
        (tmp_path / "bad.txt").write_text("1 2 3\n")
        MR.load_poses(tmp_path / "bad.txt")
    a, b = MR.candidate_views((-1, -1, -1), (1, 1, 1), 6, seed=3), MR.candidate_views((-1, -1, -1), (1, 1, 1), 6, seed=3)
    assert a.shape == (6, 4, 4) and np.array_equal(a, b) and not np.array_equal(a, MR.candidate_views((-1, -1, -1), (1, 1, 1), 6, seed=4))
    R3 = a[:, :3, :3]
    assert np.allclose(R3 @ R3.transpose(0, 2, 1), np.eye(3), atol=1e-12)
    origins = -(R3.transpose(0, 2, 1) @ a[:, :3, 3:]).reshape(-1, 3)
    assert (np.abs(origins) <= 0.7 + 1e-12).all()                        # inside the box shrunk by 0.7 about its centre


def test_new_options_are_refused_without_what_they_need(capsys):
    from splatam_amd import mesh_score, run
    with pytest.raises(SystemExit):
        run.main(["experiment.py", "--mesh", "--cull"])
    assert "--cull needs --gt-mesh" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh_score.main(["rec.ply", "gt.ply", "--occlusion"])
    assert "--occlusion needs --cull-poses" in capsys.readouterr().err
    plain = dict(accuracy_cm=1.0, completion_cm=2.0, completion_ratio=3.0, fscore=0.5, precision=0.4, recall=0.6, samples=10)
    assert len(mesh_score.format_score(plain).splitlines()) == 4        # no Depth L1 line unless depth_l1 was asked for
    more = dict(plain, depth_l1_cm=1.5, depth_l1_valid_cm=1.25, holes_gt=0, holes_rec=3, views=4)
    assert mesh_score.format_score(more).startswith(mesh_score.format_score(plain) + "\nDepth L1: 1.5000 cm")
