"""The mesh shade layer without a GPU: splatam_amd/csrc/meshshade_math.h compiled for the host (tests/meshshade_math_shim.cpp: the loop
bodies of the kernels of csrc/meshshade.hip) against the float64 restatement tests/meshshade_ref.py.

1. NORMALS: every vertex interior to a side of ``grid_cube()`` has EXACTLY its axis normal; on the sphere, the box and the grid cube the
   header's normals lie within ANGLE_BOUND of the unquantised float64 definition (4 x the largest angle observed, printed); a permutation
   of the faces gives the same bits and reversing every face the same bits with the sign flipped; faces out of range, NaN vertices, a
   repeated index, an oversized face and an unreferenced vertex add nothing.
2. VISIBILITY: on every case of ``meshrender_ref.render_cases`` the high words of the keys are the bits of the header's own depth plane
   (``mr_render``), for a split of 1, the default and "everything small"; off the oracle's fragile pixels (at most 1 %, asserted first
   on the oracle's flags) the face is the float64 ray caster's nearest face; on them it names a face the oracle hits within Z_BOUND of
   the nearest.
3. SHADING: for every mode, smooth on and off and samples 1, 2, 3 the bytes differ from the restatement's by at most B (the largest
   difference observed + 1, printed) off the fragile pixels; flat pictures hold exactly their oracle face's bytes; background pixels hold
   view_byte(bg); depth mode is view_pixel_bytes of the depth plane byte for byte; S == 0, a zero interpolated normal and a mesh
   without colours take the documented fallbacks.
4. PLUMBING: binding and header; the supersampled camera; the argument parser; ``save_mesh_ply(normals=...)``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import meshrender_ref as R
import meshshade_ref as S
from test_meshrender_cpu import load_shim as load_render_shim
from test_meshrender_cpu import shim_render
from tests.util import host_shim

F32P, I32P, I64P, U64P, U8P = (C.POINTER(t) for t in (C.c_float, C.c_int32, C.c_int64, C.c_uint64, C.c_uint8))


def load_shim():
    lib = host_shim("meshshade_math_shim", "meshshade_math.h", "meshrender_math.h", "meshclean_math.h", "meshscore_math.h", "view_math.h")
    lib.msh_vertex_normals.restype = C.c_int
    lib.msh_vertex_normals.argtypes = [F32P, C.c_int32, I32P, C.c_int32, I64P, F32P]
    lib.msh_visibility.restype = C.c_int
    lib.msh_visibility.argtypes = [F32P, C.c_int32, I32P, C.c_int32, F32P, F32P, C.c_int, C.c_int, C.c_float, C.c_int, U64P]
    lib.msh_shade.restype = C.c_int
    lib.msh_shade.argtypes = [F32P, C.c_int32, I32P, C.c_int32, F32P, F32P, F32P, F32P, C.c_int, C.c_int, C.c_float, U64P, I32P, F32P, U8P, U8P, F32P,
                              I32P, F32P]
    lib.msh_view_depth_bytes.restype = None
    lib.msh_view_depth_bytes.argtypes = [F32P, C.c_longlong, C.c_float, C.c_float, U8P, U8P]
    lib.msh_view_bytes.restype = None
    lib.msh_view_bytes.argtypes = [F32P, C.c_longlong, U8P]
    lib.msh_barycentrics_at.restype = C.c_int
    lib.msh_barycentrics_at.argtypes = [F32P, C.c_int32, I32P, F32P, F32P, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, F32P]
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


@pytest.fixture(scope="module")
def render_shim():
    return load_render_shim()


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None and a.size else None


def _mesh(vertices, faces):
    return np.ascontiguousarray(vertices, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def shim_normals(shim, vertices, faces):
    v, f = _mesh(vertices, faces)
    accum, out = np.empty((len(v), 3), dtype=np.int64), np.empty((len(v), 3), dtype=np.float32)
    assert shim.msh_vertex_normals(_p(v, F32P), len(v), _p(f, I32P), len(f), _p(accum, I64P), _p(out, F32P)) == 0
    return out


def key_camera(intr, size, samples):
    """(float32 intrinsics [4], (width, height)) of the key plane, as the Python layer forms them."""
    from splatam_amd import mesh_view
    k, ksize = mesh_view.supersampled(intr, size, samples)
    return np.array(k, dtype=np.float32), ksize


def shim_visibility(shim, vertices, faces, w2c, intr, size, samples=1, near=R.NEAR, split=0):
    v, f = _mesh(vertices, faces)
    k, (W, H) = key_camera(intr, size, samples)
    m = np.ascontiguousarray(w2c, np.float32).reshape(16)
    keys = np.empty((H, W), dtype=np.uint64)
    assert shim.msh_visibility(_p(v, F32P), len(v), _p(f, I32P), len(f), _p(m, F32P), _p(k, F32P), W, H, near, split, _p(keys, U64P)) == 0
    return keys


def shim_shade(shim, vertices, faces, colors, normals, w2c, intr, size, samples, keys, mode, smooth=True, normal_frame=0, bg=S.BG, albedo=S.ALBEDO,
               ambient=S.AMBIENT, depth_range=S.DEPTH_RANGE, lut=None, planes=False, near=R.NEAR):
    v, f = _mesh(vertices, faces)
    k, _ = key_camera(intr, size, samples)
    m = np.ascontiguousarray(w2c, np.float32).reshape(16)
    c = None if colors is None else np.ascontiguousarray(colors, np.float32)
    n = None if normals is None else np.ascontiguousarray(normals, np.float32)
    ints = np.array([S.MODE_ID[mode], samples, 1 if smooth else 0, normal_frame], dtype=np.int32)
    floats = np.array([*bg, *albedo, ambient, *depth_range], dtype=np.float32)
    lut = np.ascontiguousarray(lut, np.uint8) if lut is not None else None
    W, H = size
    rgb = np.empty((H, W, 3), dtype=np.uint8)
    depth, face, normal = (np.empty((H, W), np.float32), np.empty((H, W), np.int32), np.empty((H, W, 3), np.float32)) if planes else (None,) * 3
    keys = np.ascontiguousarray(keys, np.uint64)
    assert shim.msh_shade(_p(v, F32P), len(v), _p(f, I32P), len(f), _p(c, F32P) if c is not None else None, _p(n, F32P) if n is not None else None,
                          _p(m, F32P), _p(k, F32P), W, H, near, _p(keys, U64P), _p(ints, I32P), _p(floats, F32P),
                          _p(lut, U8P) if lut is not None else None, _p(rgb, U8P), _p(depth, F32P) if planes else None,
                          _p(face, I32P) if planes else None, _p(normal, F32P) if planes else None) == 0
    return (rgb, dict(depth=depth, face=face, normal=normal)) if planes else rgb


def view_bytes(shim, values):
    x = np.ascontiguousarray(values, np.float32).reshape(-1)
    out = np.empty(x.size, dtype=np.uint8)
    shim.msh_view_bytes(_p(x, F32P), x.size, _p(out, U8P))
    return out.reshape(np.shape(values))


def jet():
    from splatam_amd.view import jet_lut
    return jet_lut()


def normal_meshes():
    gv, gf, _ = R.grid_cube()
    return {"grid-cube": (gv, gf), "sphere": R.sphere()[:2], "box": R.box()[:2]}


# ---------------------------------------------------------------------------------------------------------------- 1. normals
def test_grid_cube_normals_are_exactly_the_axes(shim):
    v, f, _ = R.grid_cube()
    n = shim_normals(shim, v, f)
    lo, hi = v.min(axis=0), v.max(axis=0)
    on = (v == lo) | (v == hi)                                           # [V, 3]: on which sides a vertex lies
    interior = on.sum(axis=1) == 1
    assert interior.sum() > 50
    axis = on[interior].argmax(axis=1)
    got = n[interior]
    assert (np.abs(got[np.arange(len(got)), axis]) == 1.0).all()
    other = np.ones_like(got, dtype=bool)
    other[np.arange(len(got)), axis] = False
    assert (got[other] == 0.0).all()
    high = (v[interior] == hi)[np.arange(len(got)), axis]
    for a in range(3):                                                   # one winding per side: one normal per side
        for side in (False, True):
            group = got[(axis == a) & (high == side)]
            assert len(group) > 0 and (group == group[0]).all(), (a, side)


def test_normals_against_the_float64_definition(shim):
    worst = 0.0
    for name, (v, f) in normal_meshes().items():
        got, want = shim_normals(shim, v, f), S.vertex_normals(v, f)
        assert (np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0) < 1e-6).all(), name
        a = float(S.angles(got, want).max())
        print(f"{name}: max angle between the header's normals and the float64 definition = {a:.3e} rad")
        worst = max(worst, a)
    print(f"largest angle observed: {worst:.4e} rad (ANGLE_OBSERVED = {S.ANGLE_OBSERVED})")
    assert S.ANGLE_BOUND is not None and abs(S.ANGLE_BOUND - 4 * S.ANGLE_OBSERVED) <= 1e-12 * S.ANGLE_BOUND
    assert worst <= S.ANGLE_BOUND, worst


def test_normals_do_not_depend_on_face_order_or_on_winding_but_for_the_sign(shim):
    for name, (v, f) in normal_meshes().items():
        base = shim_normals(shim, v, f)
        perm = np.random.default_rng(5).permutation(len(f))
        assert np.array_equal(shim_normals(shim, v, f[perm]).view(np.uint32), base.view(np.uint32)), name
        flipped = shim_normals(shim, v, f[:, ::-1])
        assert np.array_equal(flipped.view(np.uint32), (-base).view(np.uint32) & np.where(base == 0, np.uint32(0x7fffffff), np.uint32(0xffffffff))), name


def test_normals_of_rejected_faces_and_unreferenced_vertices(shim):
    v, f = R.sphere()[:2]
    base = shim_normals(shim, v, f)
    V = len(v)
    v2 = np.concatenate((v, np.array([[np.nan, 0, 0], [7, 7, 7], [1e20, 0, 0], [0, 1e20, 0], [np.inf, 0, 0]], dtype=np.float32)))
    extra = np.array([[0, 1, len(v2)], [-1, 0, 1], [0, 1, V], [2, 2, 3], [0, V + 2, V + 3], [0, 1, V + 4]], dtype=np.int32)
    got = shim_normals(shim, v2, np.concatenate((extra, f)))
    assert np.array_equal(got[:V].view(np.uint32), base.view(np.uint32))         # none of them added anything to a vertex of the sphere
    assert (got[V:] == 0).all()                                                   # NaN, unreferenced, oversized face, infinite
    assert (shim_normals(shim, v, f[:0]) == 0).all()
    assert shim_normals(shim, v[:0], f[:0]).shape == (0, 3)
    two = np.array([[0, 1, 2], [2, 1, 0]], dtype=np.int32)                        # faces that cancel
    assert (shim_normals(shim, v[:3], two) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 2. visibility
@pytest.mark.parametrize("name", sorted(R.render_cases()))
def test_keys_hold_the_depth_plane_and_the_nearest_face(shim, render_shim, name):
    v, f, w2c, intr, size = R.render_cases()[name]
    depth64, fragile = R.oracle(name)
    assert fragile.mean() <= R.MAX_EXCUSED, f"{name}: the oracle excuses {fragile.mean():.4f} of the pixels"
    mine = S.oracle(name, 1)
    assert np.array_equal(mine[3], fragile) and np.allclose(mine[0], depth64, rtol=1e-12, atol=0)         # the same ray caster, with names
    keys = shim_visibility(shim, v, f, w2c, intr, size)
    plane = shim_render(render_shim, v, f, w2c, intr, size)
    hi, lo = (keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(0xffffffff)).astype(np.uint32)
    none = keys == np.uint64(0xffffffffffffffff)
    assert np.array_equal(np.where(none, np.uint32(0), hi), plane.view(np.uint32))
    for split in (1, 1 << 30):
        assert np.array_equal(shim_visibility(shim, v, f, w2c, intr, size, split=split), keys), split
    ids = np.where(none, -1, lo.astype(np.int64))
    assert (ids < len(f)).all()
    ok = ~fragile
    print(f"{name}: {int((ids != mine[1])[ok].sum())} of {int(ok.sum())} robust pixels name another face; {int(fragile.sum())} fragile")
    assert np.array_equal(ids[ok], mine[1][ok])
    check = fragile & ~none
    if check.any():
        z, lam_lo = S.face_at(v, f, w2c, intr, size, np.where(check, ids, 0))
        nearest = np.where(depth64 > 0, depth64, np.inf)
        assert (lam_lo[check] >= -R.TOL_BARY).all()
        assert (z[check] >= R.NEAR).all() and (z[check] <= nearest[check] * (1 + R.Z_BOUND)).all()   # (no farther than the oracle's nearest)


def test_lowest_face_index_wins_a_shared_edge(shim):
    v = np.array([[-3, -3, 2], [3, -3, 2], [3, 3, 2], [-3, 3, 2]], dtype=np.float32)
    intr, size = (8.0, 8.0, 8.0, 8.0), (17, 17)                          # pixel (i, i) looks along the diagonal exactly
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 3], [0, 1, 2]], [[2, 1, 0], [2, 0, 3]]):
        keys = shim_visibility(shim, v, np.array(faces, dtype=np.int32), np.eye(4, dtype=np.float32), intr, size)
        assert ((keys >> np.uint64(32)) == 0x40000000).all()
        assert (np.diagonal(keys) & np.uint64(0xffffffff) == 0).all(), faces


# ---------------------------------------------------------------------------------------------------------------- 3. shading
VARIANTS = [(mode, smooth, frame) for mode in S.MODES for smooth in (True, False) for frame in ((0, 1) if mode == "normal" else (0,))]


_CASE_CACHE = {}


def case_inputs(shim, name, samples):
    """(keys, normals32, normals64, colours, oracle) of a case: made once, shared."""
    key = (name, samples)
    if key not in _CASE_CACHE:
        v, f, w2c, intr, size = R.render_cases()[name]
        _CASE_CACHE[key] = (shim_visibility(shim, v, f, w2c, intr, size, samples), shim_normals(shim, v, f), S.vertex_normals(v, f), S.case_colors(name),
                            S.oracle(name, samples))
    return _CASE_CACHE[key]


@pytest.mark.parametrize("samples", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(R.render_cases()))
def test_bytes_against_the_float64_restatement(shim, name, samples):
    v, f, w2c, intr, size = R.render_cases()[name]
    keys, n32, n64, colours, (depth64, face64, lam64, fragile_s) = case_inputs(shim, name, samples)
    assert fragile_s.mean() <= R.MAX_EXCUSED, f"{name} x{samples}: the oracle excuses {fragile_s.mean():.4f} of the sub-pixels"
    fragile = S.reduce_any(fragile_s, samples)
    none = keys == np.uint64(0xffffffffffffffff)
    z32 = np.where(none, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).view(np.float32)
    lut = jet()
    bg_bytes = view_bytes(shim, np.array(S.BG, dtype=np.float32))
    worst = 0
    for mode, smooth, frame in VARIANTS:
        got = shim_shade(shim, v, f, colours, n32, w2c, intr, size, samples, keys, mode, smooth=smooth, normal_frame=frame, lut=lut)
        want, decision = S.shade(v, f, colours, n64, w2c, intr, size, samples, face64, lam64, z32, mode, smooth=smooth, normal_frame=frame, lut=lut)
        excused = fragile | decision
        assert excused.mean() <= 2 * R.MAX_EXCUSED, (name, mode, excused.mean())
        diff = np.abs(got.astype(np.int64) - np.rint(want * 255.0).astype(np.int64)).max(axis=2)
        worst_here = int(diff[~excused].max())
        print(f"{name} x{samples} {mode}{'' if smooth else ' flat'}{' camera' if frame else ''}: max |byte - restatement| = {worst_here} "
              f"({int(excused.sum())} of {excused.size} pixels excused)")
        worst = max(worst, worst_here)
        assert S.B is not None and S.B == S.BYTES_OBSERVED + 1
        assert worst_here <= S.B, (name, samples, mode, smooth, frame, worst_here)
        background = S.reduce_any(face64 < 0, samples) & ~S.reduce_any(face64 >= 0, samples) & ~fragile
        assert (got[background] == bg_bytes).all(), (name, mode)
    print(f"{name} x{samples}: largest byte difference observed = {worst} (BYTES_OBSERVED = {S.BYTES_OBSERVED})")


@pytest.mark.parametrize("name", sorted(R.render_cases()))
def test_flat_pictures_hold_exactly_their_faces_bytes(shim, name):
    """With smooth off a pixel's normal is its face's alone: the picture in normal mode holds, at every robust pixel, the bytes of the
    oracle face's own normal -- computed here from the header's float32 cross product of the world-frame vertices."""
    v, f, w2c, intr, size = R.render_cases()[name]
    keys, n32, _, colours, (_, face64, _, fragile) = case_inputs(shim, name, 1)
    got, planes = shim_shade(shim, v, f, colours, n32, w2c, intr, size, 1, keys, "normal", smooth=False, planes=True)
    ok = ~fragile & (face64 >= 0)
    assert np.array_equal(planes['face'][~fragile], face64[~fragile])
    g = f[face64[ok]]
    a, b, c = (v[g[:, k]].astype(np.float32) for k in range(3))
    ab, ac = b - a, c - a
    fn = np.stack((ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]), axis=1)
    length = np.sqrt((fn[:, 0] * fn[:, 0] + fn[:, 1] * fn[:, 1]) + fn[:, 2] * fn[:, 2])
    unit = fn / length[:, None]
    assert unit.dtype == np.float32
    assert np.array_equal(planes['normal'][ok].view(np.uint32), unit.view(np.uint32))
    assert np.array_equal(got[ok], view_bytes(shim, (unit + np.float32(1)) * np.float32(0.5)))
    assert (planes['face'][face64 < 0][~fragile[face64 < 0]] == -1).all()


@pytest.mark.parametrize("name", sorted(R.render_cases()))
def test_depth_mode_and_the_depth_plane(shim, render_shim, name):
    v, f, w2c, intr, size = R.render_cases()[name]
    keys, n32, _, colours, _ = case_inputs(shim, name, 1)
    lut = jet()
    got, planes = shim_shade(shim, v, f, colours, n32, w2c, intr, size, 1, keys, "depth", lut=lut, planes=True)
    plane = shim_render(render_shim, v, f, w2c, intr, size)
    assert np.array_equal(planes['depth'].view(np.uint32), plane.view(np.uint32))
    want = np.empty((plane.size, 3), dtype=np.uint8)
    shim.msh_view_depth_bytes(_p(plane, F32P), plane.size, S.DEPTH_RANGE[0], S.DEPTH_RANGE[1], _p(lut, U8P), _p(want, U8P))
    hit = plane > 0
    assert np.array_equal(got[hit], want.reshape(*plane.shape, 3)[hit])
    assert (got[~hit] == view_bytes(shim, np.array(S.BG, dtype=np.float32))).all()
    assert len(np.unique(got[hit].reshape(-1, 3), axis=0)) > 3                    # (the range spreads the case over the table)


def test_documented_fallbacks(shim):
    # S == 0: a face seen exactly edge-on from the camera centre's plane -- all three vertices on a line through the centre's ray
    v = np.array([[0, 0, 1], [0, 0, 2], [0, 0, 3], [-1, -1, 2], [1, -1, 2], [0, 1, 2]], dtype=np.float32)
    eye, intr, size = np.eye(4, dtype=np.float32), (8.0, 8.0, 4.0, 4.0), (9, 9)
    k = np.array(intr, dtype=np.float32)
    lam = np.zeros(3, dtype=np.float32)
    idx = np.array([0, 1, 2], dtype=np.int32)
    assert shim.msh_barycentrics_at(_p(v, F32P), len(v), _p(idx, I32P), _p(eye.reshape(16), F32P), _p(k, F32P), 9, 9, 0.01, 4, 4, _p(lam, F32P)) == 0
    assert (lam == np.float32(1) / np.float32(3)).all()
    idx = np.array([3, 4, 5], dtype=np.int32)
    assert shim.msh_barycentrics_at(_p(v, F32P), len(v), _p(idx, I32P), _p(eye.reshape(16), F32P), _p(k, F32P), 9, 9, 0.01, 4, 4, _p(lam, F32P)) == 0
    assert abs(float(lam.sum()) - 1) < 1e-6 and (lam > 0).all() and abs(lam[2] - 0.5) < 1e-6      # the centre ray: halfway up the median
    # a zero interpolated normal: vertex normals that cancel at the pixel -> the face's own normal, as with smooth off
    f = np.array([[3, 4, 5]], dtype=np.int32)
    keys = shim_visibility(shim, v, f, eye, intr, size)
    zero = np.zeros((len(v), 3), dtype=np.float32)
    flat, pf = shim_shade(shim, v, f, None, None, eye, intr, size, 1, keys, "shaded", smooth=False, planes=True)
    smooth0, p0 = shim_shade(shim, v, f, None, zero, eye, intr, size, 1, keys, "shaded", smooth=True, planes=True)
    none, pn = shim_shade(shim, v, f, None, None, eye, intr, size, 1, keys, "shaded", smooth=True, planes=True)
    assert np.array_equal(flat, smooth0) and np.array_equal(flat, none)
    hit = pf['face'] == 0
    assert hit.sum() > 5 and (np.abs(pf['normal'][hit]) == np.array([0, 0, 1], dtype=np.float32)).all()
    assert np.array_equal(pf['normal'], p0['normal']) and np.array_equal(pf['normal'], pn['normal'])
    # a mesh without colours: colour modes show the albedo
    plain = shim_shade(shim, v, f, None, None, eye, intr, size, 1, keys, "color")
    assert (plain[hit] == view_bytes(shim, np.array(S.ALBEDO, dtype=np.float32))).all()
    assert (plain[~hit] == view_bytes(shim, np.array(S.BG, dtype=np.float32))).all()
    assert np.array_equal(shim_shade(shim, v, f, None, None, eye, intr, size, 1, keys, "shaded-color"), flat)
    # a head light on a wall seen square on: L = 1 at the centre whatever the winding
    for faces in (f, f[:, ::-1].copy()):
        img = shim_shade(shim, v, faces, None, None, eye, intr, size, 1, shim_visibility(shim, v, faces, eye, intr, size), "shaded", smooth=False)
        assert (img[4, 4] == view_bytes(shim, np.array(S.ALBEDO, dtype=np.float32))).all()
    # an empty mesh, keys of a foreign plane: a picture of the background
    empty = shim_shade(shim, v[:0], f[:0], None, None, eye, intr, size, 1, keys, "shaded")
    assert (empty == view_bytes(shim, np.array(S.BG, dtype=np.float32))).all()


def test_header_under_address_and_ub_sanitizers(tmp_path):
    """The shim's host functions as a stand-alone program (its own main) built with -fsanitize=address,undefined: faces out of range,
    NaN and infinite vertices, an oversized face, keys that name faces past the end and faces that render nothing, every mode, samples
    1..4, an empty mesh.  Any sanitizer report or wrong answer is a non-zero exit.  The runtimes are linked statically; nothing loaded
    into python is involved."""
    exe = str(tmp_path / "meshshade_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DMESHSHADE_SHIM_MAIN", "-o", exe,
                           os.path.join(os.path.dirname(__file__), "meshshade_math_shim.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout


# ---------------------------------------------------------------------------------------------------------------- 4. plumbing
def test_binding_and_header_name_the_entry_points():
    from splatam_amd import _capi
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "splat_hip.h")).read()
    L = _capi.lib()
    for name in ("splat_mesh_vertex_normals", "splat_mesh_visibility", "splat_mesh_shade"):
        assert hasattr(L, name) and name in _capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert L.splat_sizeof(b"SplatMeshShade") == C.sizeof(_capi.SplatMeshShade) > 0
    assert L.splat_abi_version() == 17
    for k, name in enumerate(("COLOR", "SHADED", "SHADED_COLOR", "NORMAL", "DEPTH")):
        assert int(re.search(rf"#define SPLAT_MESH_SHADE_{name} (\d+)", header).group(1)) == getattr(_capi, f"SPLAT_MESH_SHADE_{name}") == k
    assert [S.MODE_ID[m] for m in S.MODES] == [0, 1, 2, 3, 4]
    # refusals need no device: nothing is launched
    P = 1 << 12
    assert L.splat_mesh_vertex_normals(None, 3, P, 1, P, P, None) == 1                      # vertices promised, none given
    assert L.splat_mesh_vertex_normals(P, 3, None, 1, P, P, None) == 1
    assert L.splat_mesh_vertex_normals(P, -1, None, 0, P, P, None) == 1
    assert L.splat_mesh_vertex_normals(None, 0, None, 0, None, None, None) == 0             # an empty mesh: no launch
    view = _capi.SplatMeshView()
    view.width, view.height, view.fx, view.fy, view.near_z, view.w2c = 8, 8, 1.0, 1.0, 0.01, P
    assert L.splat_mesh_visibility(None, 0, None, 0, C.byref(view), None, None) == 1        # no keys
    assert L.splat_mesh_visibility(None, 0, None, 0, None, P, None) == 1
    args = _capi.SplatMeshShade()
    args.mode, args.samples = 1, 1
    assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), None, C.byref(args), P, None, None, None, None) == 1     # NULL keys
    assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), P, None, P, None, None, None, None) == 1
    assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), P, C.byref(args), None, None, None, None, None) == 1
    for samples in (0, 5, 3):                                                                # 3 does not divide 8
        args.samples = samples
        assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), P, C.byref(args), P, None, None, None, None) == 1, samples
    args.samples = 2
    assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), P, C.byref(args), P, P, None, None, None) == 1           # planes, samples 2
    args.samples, args.mode = 1, 5
    assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), P, C.byref(args), P, None, None, None, None) == 1
    args.mode = 4                                                                            # depth mode without a table
    assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), P, C.byref(args), P, None, None, None, None) == 1
    args.mode = 1
    view.width, view.height = 1 << 15, 1 << 15                                               # 2^30 pixels
    assert L.splat_mesh_visibility(None, 0, None, 0, C.byref(view), P, None) == 1
    assert L.splat_mesh_shade(None, 0, None, 0, None, None, C.byref(view), P, C.byref(args), P, None, None, None, None) == 1


def test_sub_pixel_centres_average_to_the_pixel_centre():
    from splatam_amd import mesh_view
    intr, size = R.pinhole(67, 45, 57.0), (67, 45)
    for s in (1, 2, 3, 4):
        (fx, fy, cx, cy), (W, H) = mesh_view.supersampled(intr, size, s)
        assert (W, H) == (67 * s, 45 * s)
        i, j = np.arange(67, dtype=np.float64), np.arange(45, dtype=np.float64)
        sub = np.arange(s, dtype=np.float64)
        x = ((i[:, None] * s + sub[None, :]) - cx) / fx
        y = ((j[:, None] * s + sub[None, :]) - cy) / fy
        assert np.allclose(x.mean(axis=1), (i - intr[0 + 2]) / intr[0], rtol=0, atol=1e-12)
        assert np.allclose(y.mean(axis=1), (j - intr[3]) / intr[1], rtol=0, atol=1e-12)
        assert S.supersampled(intr, size, s) == ((fx, fy, cx, cy), (W, H))
    with pytest.raises(ValueError):
        mesh_view.supersampled(intr, size, 5)


def test_argument_parser(tmp_path, capsys):
    from splatam_amd import mesh, mesh_view, run
    p = mesh_view._parser()
    a = p.parse_args(["m.ply", "--out", "d", "--poses", "traj.txt", "--size", "640x480", "--intrinsics", "500", "501", "319.5", "239.5", "--mode",
                      "shaded-color", "--flat", "--every", "3", "--samples", "2", "--black"])
    assert (a.mesh, a.out, a.poses, a.params, a.size, a.intrinsics) == ("m.ply", "d", "traj.txt", None, (640, 480), [500.0, 501.0, 319.5, 239.5])
    assert (a.mode, a.flat, a.every, a.samples, a.black, a.transform) == ("shaded-color", True, 3, 2, True, None)
    d = p.parse_args(["m.ply", "--out", "d", "--params", "params.npz"])
    assert (d.mode, d.flat, d.every, d.samples, d.black, d.size) == ("shaded", False, 1, 1, False, None)
    for bad in (["m.ply", "--out", "d"], ["m.ply", "--out", "d", "--poses", "a", "--params", "b"], ["m.ply", "--out", "d", "--params", "b", "--samples", "5"],
                ["m.ply", "--out", "d", "--params", "b", "--mode", "wireframe"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):
        mesh_view.main(["m.ply", "--out", "d", "--poses", "traj.txt"])
    assert "--poses needs --size and --intrinsics" in capsys.readouterr().err
    m = mesh._parser().parse_args(["params.npz", "--out", "mesh.ply", "--views", "pics", "--views-mode", "normal"])
    assert (m.views, m.views_mode) == ("pics", "normal")
    assert mesh._parser().parse_args(["params.npz", "--out", "mesh.ply"]).views is None
    with pytest.raises(SystemExit):
        mesh.main(["params.npz", "--out", "mesh.ply", "--views-mode", "normal"])
    assert "--views-mode needs --views" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run.main(["experiment.py", "--mesh-views", "pics"])
    assert "--mesh-views needs --mesh" in capsys.readouterr().err


def test_save_mesh_ply_with_normals(tmp_path):
    from splatam_amd.export import load_mesh_ply, save_mesh_ply
    v, f, colours = R.grid_cube()
    n = S.vertex_normals(v, f).astype(np.float32)
    plain, same, with_n = tmp_path / "plain.ply", tmp_path / "same.ply", tmp_path / "normals.ply"
    save_mesh_ply(plain, v, f, colours)
    save_mesh_ply(same, v, f, colours, normals=None)
    assert plain.read_bytes() == same.read_bytes()
    save_mesh_ply(with_n, v, f, colours, normals=n)
    data = with_n.read_bytes()
    head, body = data[:data.index(b"end_header\n") + 11], data[data.index(b"end_header\n") + 11:]
    assert b"property float nx\nproperty float ny\nproperty float nz\n" in head
    assert head.replace(b"property float nx\nproperty float ny\nproperty float nz\n", b"") == plain.read_bytes()[:len(head) - 54]
    table = np.frombuffer(body, dtype=[('p', '<f4', (3,)), ('n', '<f4', (3,)), ('c', 'u1', (3,))], count=len(v))
    assert np.array_equal(table['n'], n) and np.array_equal(table['p'], v)
    v2, f2, c2 = load_mesh_ply(with_n)
    v1, f1, c1 = load_mesh_ply(plain)
    assert np.array_equal(v2, v1) and np.array_equal(f2, f1) and np.array_equal(c2, c1)
    with pytest.raises(ValueError, match="normals"):
        save_mesh_ply(with_n, v, f, colours, normals=n[:-1])
