"""Marching cubes without a GPU: the cubes part of splatam_amd/csrc/tsdf_math.h (and its table, csrc/tsdf_cubes_table.h) compiled for the
host (tests/tsdf_cubes_shim.cpp) against tests/tsdf_cubes_ref.py, a restatement of the RULE -- face cycles seen from outside, one
directed segment per run of inside corners, loops from their lowest edge, fans -- written independently of the header.

1. TABLE: all 256 rows equal the restatement's, entry for entry (count, edges, order, winding); the facts are recomputed, not trusted:
   at most 5 triangles a row, 820 in all, loops of at most 7 edges, 88 masks whose count differs from their complement's.
2. PER MASK: the edges used are the edges whose ends differ in sign; the triangles' boundary is the rule's directed face segments,
   each once; fan diagonals cancel.
3. CLOSURE ACROSS FACES: for every axis and every ordered pair of masks that agree on the shared face's four corners, the directed
   segments the two cells put on that face are exact reverses.
4. MESHES on the 29 x 25 x 27 grid of tests/test_tsdf_math_cpu.py: sphere (Euler characteristic 2) and torus (0) are closed
   manifolds with positive volume, the sphere's vertices within L^2 / (8 (r - L)) of the sphere; the vertices are exactly the
   tetrahedra mesh's on axis edges, bit for bit; exact zeros keep the mesh balanced and their zero-area triangles; an unseen plane
   opens the mesh only next to it; sign noise stays a closed oriented cycle.
5. The shim as a stand-alone program under the address and undefined-behaviour sanitizers.
6. INTERFACE: ``method`` defaults to "tetrahedra" everywhere, ``clean`` is still ``extract_mesh``'s last parameter, unknown methods are
   refused before any device work, the commands parse the option, the binding and the header name the entry points."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_cubes_ref as Q
import tsdf_ref as R
from tests.util import host_shim

F32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int64)
HERE = os.path.dirname(os.path.abspath(__file__))
TOPO_DIMS, TOPO_VOXEL, TOPO_ORIGIN = (29, 25, 27), 0.05, (-0.7, -0.6, -0.65)
SPHERE_C, SPHERE_R = (0.013, 0.021, -0.017), 0.45


def load_cubes_shim():
    lib = host_shim("tsdf_cubes_shim", "tsdf_math.h", "tsdf_cubes_table.h")
    lib.tc_table.restype = None
    lib.tc_table.argtypes = [C.c_void_p]
    lib.tc_edge.restype = None
    lib.tc_edge.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.tc_cell_pattern.restype = C.c_int
    lib.tc_cell_pattern.argtypes = [C.c_int, I64P]
    lib.tc_triangles.restype = C.c_longlong
    lib.tc_triangles.argtypes = [C.c_int] * 3 + [F32P, C.c_float, F32P, F32P, C.c_float, I64P, C.c_longlong]
    lib.tc_vertices.restype = None
    lib.tc_vertices.argtypes = [C.c_int] * 3 + [F32P, C.c_float] + [F32P] * 4 + [I64P, C.c_longlong, F32P, F32P]
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_cubes_shim()


def _f(a):
    return a.ctypes.data_as(F32P)


def shim_table(shim):
    t = np.zeros((256, 16), dtype=np.int8)
    shim.tc_table(t.ctypes.data)
    return t


def shim_cubes(shim, vol, origin, voxel, min_weight=1.0, capacity=None):
    """(keys [min(n, capacity), 3], n) of the host model of the cubes pass."""
    nz, ny, nx = vol["tsdf"].shape
    o = np.array(origin, np.float32)
    tsdf, weight = np.ascontiguousarray(vol["tsdf"], np.float32), np.ascontiguousarray(vol["weight"], np.float32)
    args = (nx, ny, nz, _f(o), voxel, _f(tsdf), _f(weight), min_weight)
    if capacity is None:
        capacity = shim.tc_triangles(*args, None, 0)
    keys = np.full((max(capacity, 1), 3), -1, dtype=np.int64)
    n = shim.tc_triangles(*args, keys.ctypes.data_as(I64P), capacity)
    return keys[:min(n, capacity)], n


def shim_vertices(shim, vol, origin, voxel, keys):
    nz, ny, nx = vol["tsdf"].shape
    o, keys = np.array(origin, np.float32), np.ascontiguousarray(keys, np.int64)
    pos, col = np.zeros((len(keys), 3), np.float32), np.zeros((len(keys), 3), np.float32)
    arrays = [np.ascontiguousarray(vol[k], np.float32) for k in ("tsdf", "r", "g", "b")]
    shim.tc_vertices(nx, ny, nz, _f(o), voxel, *(_f(a) for a in arrays), keys.ctypes.data_as(I64P), len(keys), _f(pos), _f(col))
    return pos, col


def host_mesh(shim, vol, origin, voxel, min_weight=1.0):
    """The canonical mesh of the host model: (unique keys, vertices, faces int32 sorted lexicographically, colours) -- what
    ``_Surface.extract`` makes of the device's keys."""
    keys, n = shim_cubes(shim, vol, origin, voxel, min_weight)
    assert n == len(keys)
    uniq, inverse = np.unique(keys.reshape(-1), return_inverse=True)
    faces = inverse.reshape(-1, 3)
    faces = faces[np.lexsort((faces[:, 2], faces[:, 1], faces[:, 0]))].astype(np.int32)
    pos, col = shim_vertices(shim, vol, origin, voxel, uniq)
    return uniq, pos, faces, col


# ---------------------------------------------------------------------------------------------------------------- 1. table
def test_all_256_rows_equal_the_rule(shim):
    got, want = shim_table(shim), Q.table()
    for mask in range(256):
        assert got[mask].tolist() == want[mask].tolist(), mask
    corners = (C.c_int * 2)()
    for e, (ca, cb) in enumerate(Q.EDGES):
        shim.tc_edge(e, corners)
        assert tuple(corners) == (ca, cb), e


def test_facts_of_the_table_recomputed(shim):
    t = shim_table(shim)
    counts = t[:, 0].astype(int)
    assert counts.max() == 5 and counts.min() == 0 and counts.sum() == 820
    assert max(len(l) for m in range(256) for l in Q.loops(m)) == 7
    assert sum(1 for m in range(256) if counts[m] != counts[255 - m]) == 88
    assert counts[0] == 0 == counts[255]
    for mask in range(256):                                 # a count is the loops' edges less two each; nothing behind the count
        assert counts[mask] == sum(len(l) - 2 for l in Q.loops(mask))
        assert not t[mask, 1 + 3 * counts[mask]:].any()


def test_every_mask_uses_the_crossed_edges_and_bounds_the_face_segments(shim):
    t = shim_table(shim)
    keys = np.zeros((5, 3), dtype=np.int64)
    for mask in range(256):
        tris = t[mask, 1:1 + 3 * t[mask, 0]].reshape(-1, 3).tolist()
        crossed = {e for e, (ca, cb) in enumerate(Q.EDGES) if ((mask >> ca) & 1) != ((mask >> cb) & 1)}
        assert {e for tri in tris for e in tri} == crossed, mask
        d = Q.directed_edges(tris)
        net = {}
        for (a, b), n in d.items():                         # fan diagonals occur once in each direction and cancel
            k = n - d.get((b, a), 0)
            if k > 0:
                net[(a, b)] = k
        assert all(n == 1 for n in net.values()) and sorted(net) == sorted(Q.segments(mask)), mask
        # the header's functions say what the table says
        n = shim.tc_cell_pattern(mask, keys.ctypes.data_as(I64P))
        assert n == len(tris), mask
        want = [[R.edge_key((2, 2, 2), (0, 0, 0), *Q.EDGES[e]) for e in tri] for tri in tris]
        assert keys[:n].tolist() == want, mask


# ---------------------------------------------------------------------------------------------------------------- 3. closure
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_neighbouring_cells_put_reversed_segments_on_their_shared_face(shim, axis):
    """The cell on the low side sees the face as its +axis face, the cell on the high side as its -axis face; an edge of the face is
    named by its two grid points, which are corner c of the high cell and corner c | 1 << axis of the low cell."""
    t = shim_table(shim)
    bit = 1 << axis
    face_lo = [c for c in range(8) if c & bit]              # the low cell's corners on the face; c ^ bit: the high cell's
    f_plus = next(n for n, (a, s, _) in enumerate(Q.FACES) if a == axis and s == 1)
    f_minus = next(n for n, (a, s, _) in enumerate(Q.FACES) if a == axis and s == 0)

    def table_segments(mask, on_side):
        """The net directed edges of the table's triangles between crossings that lie on the face."""
        tris = t[mask, 1:1 + 3 * t[mask, 0]].reshape(-1, 3).tolist()
        on = {e for e, (ca, cb) in enumerate(Q.EDGES) if (ca & bit) == on_side and (cb & bit) == on_side}
        d = Q.directed_edges(tris)
        return sorted((a, b) for (a, b), n in d.items() if a in on and b in on and n > d.get((b, a), 0))

    def to_high(e):                                         # the low cell's edge on the face -> the high cell's number for it
        ca, cb = Q.EDGES[e]
        return Q.EDGE_OF[(ca ^ bit, cb ^ bit)]

    other = [c for c in range(8) if not c & bit]
    checked = 0
    for pattern in range(16):
        lows, highs = [], []
        for rest in range(16):
            lo = sum(((pattern >> n) & 1) << c for n, c in enumerate(face_lo)) | sum(((rest >> n) & 1) << c for n, c in enumerate(other))
            hi = sum(((pattern >> n) & 1) << (c ^ bit) for n, c in enumerate(face_lo)) | sum(((rest >> n) & 1) << (c | bit) for n, c in enumerate(other))
            lows.append(lo)
            highs.append(hi)
        # the TABLE's triangles, the cell's own fan diagonals cancelled: what the low cell leaves on the face is the reverse of what
        # the high cell leaves there, for every pair of completions
        reversed_hi = [sorted((b, a) for a, b in table_segments(hi, 0)) for hi in highs]
        for lo in lows:
            seg_lo = sorted((to_high(a), to_high(b)) for a, b in table_segments(lo, bit))
            for hi, rev in zip(highs, reversed_hi):
                assert seg_lo == rev, (axis, lo, hi)
                checked += 1
        # ... and both are the rule's segments on that face, the ambiguous patterns (the face's two diagonals) included: a pair of
        # edges lies on one face only, so a fan diagonal along the face cancels within its cell and is not taken for a segment
        for lo, hi in zip(lows, highs):
            assert table_segments(lo, bit) == sorted(Q.face_segments(lo, f_plus)), (axis, lo)
            assert table_segments(hi, 0) == sorted(Q.face_segments(hi, f_minus)), (axis, hi)
        assert len(table_segments(lows[0], bit)) == (0 if pattern in (0, 15) else 2 if pattern in (6, 9) else 1)
    assert checked == 16 * 16 * 16


# ---------------------------------------------------------------------------------------------------------------- 4. meshes
def _checked(shim, vol, min_weight=1.0):
    keys, n = shim_cubes(shim, vol, TOPO_ORIGIN, TOPO_VOXEL, min_weight)
    assert n == len(keys)
    assert keys.tolist() == Q.triangles(vol["tsdf"], vol["weight"], min_weight).tolist()      # (cell order, table order: equal as lists)
    uniq, faces = np.unique(keys.reshape(-1), return_inverse=True)
    pos, col = shim_vertices(shim, vol, TOPO_ORIGIN, TOPO_VOXEL, uniq)
    return uniq, faces.reshape(-1, 3), pos, col


def _areas(pos, faces):
    p = pos.astype(np.float64)[faces]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


@pytest.fixture(scope="module")
def sphere():
    return R.field_volume(R.sphere_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, SPHERE_R))


def test_sphere_is_a_closed_manifold_with_euler_characteristic_2(shim, sphere):
    uniq, faces, pos, col = _checked(shim, sphere)
    V, E, F, closed = R.topology(faces)                     # closed: every directed edge once and its reverse once
    print(f"sphere: {F} triangles, {V} vertices")
    assert closed and V - E + F == 2 and F > 1000
    vol = R.signed_volume(pos, faces)
    assert vol > 0 and abs(vol - 4 / 3 * np.pi * SPHERE_R ** 3) < 0.02 * 4 / 3 * np.pi * SPHERE_R ** 3
    L = np.sqrt(3) * TOPO_VOXEL                             # the bound the tetrahedra test uses (its longest edge; an axis edge is shorter)
    off = np.abs(np.linalg.norm(pos.astype(np.float64) - np.array(SPHERE_C), axis=1) - SPHERE_R)
    print(f"largest |distance - r| {off.max():.3e} (bound {L * L / (8 * (SPHERE_R - L)):.3e})")
    assert off.max() <= L * L / (8 * (SPHERE_R - L))


def test_torus_is_a_closed_manifold_with_euler_characteristic_0(shim):
    vol = R.field_volume(R.torus_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, 0.4, 0.15))
    _, faces, pos, _ = _checked(shim, vol)
    V, E, F, closed = R.topology(faces)
    assert closed and V - E + F == 0 and F > 1000
    assert R.signed_volume(pos, faces) > 0


def test_vertices_are_the_tetrahedra_vertices_on_axis_edges_bit_for_bit(shim, sphere):
    tets = host_shim("tsdf_math_shim", "tsdf_math.h", "tsdf_cubes_table.h")       # the tetrahedra's host model (tests/tsdf_math_shim.cpp)
    tets.tm_triangles.restype = C.c_longlong
    tets.tm_triangles.argtypes = [C.c_int] * 3 + [F32P, C.c_float, F32P, F32P, C.c_float, I64P, C.c_longlong]
    tets.tm_vertices.restype = None
    tets.tm_vertices.argtypes = [C.c_int] * 3 + [F32P, C.c_float] + [F32P] * 4 + [I64P, C.c_longlong, F32P, F32P]
    nz, ny, nx = sphere["tsdf"].shape
    o = np.array(TOPO_ORIGIN, np.float32)
    args = (nx, ny, nz, _f(o), TOPO_VOXEL, _f(sphere["tsdf"]), _f(sphere["weight"]), 1.0)
    n = tets.tm_triangles(*args, None, 0)
    tet_keys = np.zeros((n, 3), dtype=np.int64)
    assert tets.tm_triangles(*args, tet_keys.ctypes.data_as(I64P), n) == n
    tet_uniq = np.unique(tet_keys.reshape(-1))
    uniq, faces, pos, col = _checked(shim, sphere)
    axis = np.isin(tet_uniq & 7, (1, 2, 4))
    assert np.array_equal(uniq, tet_uniq[axis]) and 0 < axis.sum() < len(tet_uniq)
    tet_pos, tet_col = np.zeros((len(tet_uniq), 3), np.float32), np.zeros((len(tet_uniq), 3), np.float32)
    tets.tm_vertices(nx, ny, nz, _f(o), TOPO_VOXEL, *(_f(sphere[k]) for k in ("tsdf", "r", "g", "b")), tet_uniq.ctypes.data_as(I64P), len(tet_uniq),
                     _f(tet_pos), _f(tet_col))
    assert pos.tobytes() == tet_pos[axis].tobytes() and col.tobytes() == tet_col[axis].tobytes()
    print(f"cubes {len(faces)} triangles, {len(uniq)} vertices; tetrahedra {n} triangles, {len(tet_uniq)} vertices")
    assert 3 * len(faces) <= n + n // 10 and 3 * len(uniq) <= len(tet_uniq) + len(tet_uniq) // 10      # about a third


def test_corners_that_are_exactly_zero_keep_the_mesh_balanced(shim):
    field = R.sphere_field(TOPO_DIMS, TOPO_ORIGIN, TOPO_VOXEL, SPHERE_C, SPHERE_R).astype(np.float32)
    zero = np.abs(field) < 0.004
    assert zero.sum() == 156
    field[zero] = 0.0
    _, faces, pos, _ = _checked(shim, R.field_volume(field))
    ok, multiple = Q.balanced(faces)
    assert ok
    assert R.signed_volume(pos, faces) > 0
    assert (_areas(pos, faces) == 0).sum() > 0              # kept: dropping them would open the mesh


def test_an_unseen_plane_opens_the_mesh_only_next_to_it(shim, sphere):
    vol = dict(sphere, weight=sphere["weight"].copy())
    slab = 14                                               # the plane x = origin + 14 voxel cuts the sphere
    vol["weight"][:, :, slab] = 0.0
    uniq, faces, pos, _ = _checked(shim, vol)
    for key in uniq.tolist():                               # no vertex on a grid edge that touches the plane
        a, b = R.decode_key(TOPO_DIMS, key)
        assert a[0] != slab and b[0] != slab
    boundary = R.boundary_edges(faces)
    assert len(boundary) > 20
    planes = (np.float32(TOPO_ORIGIN[0]) + np.float32(TOPO_VOXEL) * np.float32(slab - 1), np.float32(TOPO_ORIGIN[0]) + np.float32(TOPO_VOXEL) * np.float32(slab + 1))
    for a, b in boundary:                                   # open only in cells that touch it: the boundary runs in the planes beside it
        assert pos[a, 0] == pos[b, 0] and pos[a, 0] in planes, (pos[a], pos[b])
    # a capacity below the need: the count still reports the need and nothing beyond the capacity is written
    full, n = shim_cubes(shim, vol, TOPO_ORIGIN, TOPO_VOXEL)
    part, n2 = shim_cubes(shim, vol, TOPO_ORIGIN, TOPO_VOXEL, capacity=n // 2)
    assert n2 == n and len(part) == n // 2 and np.array_equal(part, full[:n // 2])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sign_noise_is_a_closed_oriented_cycle(shim, seed):
    vol = Q.noise_volume((14, 13, 12), seed)
    keys, n = shim_cubes(shim, vol, (0.0, 0.0, 0.0), 1.0)
    assert n == len(keys) > 1000 and keys.tolist() == Q.triangles(vol["tsdf"], vol["weight"]).tolist()
    ok, multiple = Q.balanced(keys)
    print(f"noise seed {seed}: {n} triangles, {len(Q.directed_edges(keys))} directed edges, {multiple} used more than once")
    assert ok


# ---------------------------------------------------------------------------------------------------------------- 5. sanitizers
def test_the_shim_as_a_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main): all 256 masks, a volume with no surface, a 2 x 2 x 2 volume and the noise volume.
    Any sanitizer report or wrong answer is a non-zero exit.  The runtimes are linked statically and the program runs in the
    environment as it is: nothing of it is changed, and nothing loaded into python is involved."""
    exe = str(tmp_path / "tsdf_cubes_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DTSDF_CUBES_MAIN", "-o", exe, os.path.join(HERE, "tsdf_cubes_shim.cpp")])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.startswith("ok: 820 table triangles"), (done.stdout, done.stderr)


# ---------------------------------------------------------------------------------------------------------------- 6. interface
def test_method_defaults_to_tetrahedra_at_every_entry():
    from splatam_amd import mesh as M
    from splatam_amd import run
    from splatam_amd.session import SlamSession
    for f in (M._Surface.extract, M.TsdfVolume.extract, M.SparseTsdfVolume.extract, M.extract_mesh, M.mesh_from_params, SlamSession.extract_mesh):
        assert inspect.signature(f).parameters["method"].default == "tetrahedra", f
    ex = inspect.signature(M.extract_mesh).parameters
    assert list(ex)[-1] == "clean" and list(ex)[-2] == "method" and ex["clean"].default is None
    assert list(inspect.signature(M._Surface.extract).parameters) == ["self", "min_weight", "capacity", "method"]
    assert M._parser().parse_args(["p.npz", "--out", "m.ply"]).method == "tetrahedra"
    assert run._parser().parse_args(["e.py", "--mesh"]).mesh_method is None
    assert M.METHODS == ("tetrahedra", "cubes")


def test_an_unknown_method_is_refused_before_any_device_work():
    from splatam_amd import mesh as M
    from splatam_amd.session import SlamSession

    class Untouchable:                                      # any attribute access would be device work on its way
        def __getattr__(self, name):
            raise AssertionError(f"touched {name}")

    for bad in ("cube", "mc", None, 1):
        with pytest.raises(ValueError, match="unknown surface method"):
            M.extract_mesh(Untouchable(), [0], (8, 8), (1.0, 1.0, 4.0, 4.0), method=bad)
        with pytest.raises(ValueError, match="unknown surface method"):
            M._Surface.extract(Untouchable(), method=bad)
        with pytest.raises(ValueError, match="unknown surface method"):
            M.mesh_from_params("no_such_params.npz", "no_such.ply", method=bad)
        with pytest.raises(ValueError, match="unknown surface method"):
            SlamSession.extract_mesh(Untouchable(), method=bad)
    assert M.check_method("cubes") == "cubes" and M.check_method("tetrahedra") == "tetrahedra"


def test_the_commands_parse_the_method_and_refuse_unknown_values(capsys):
    from splatam_amd import mesh, run
    assert mesh._parser().parse_args(["p.npz", "--out", "m.ply", "--method", "cubes"]).method == "cubes"
    assert mesh._parser().parse_args(["p.npz", "--out", "m.ply", "--method", "tetrahedra", "--sparse"]).method == "tetrahedra"
    assert run._parser().parse_args(["e.py", "--mesh", "--mesh-method", "cubes"]).mesh_method == "cubes"
    with pytest.raises(SystemExit):
        mesh.main(["p.npz", "--out", "m.ply", "--method", "dual"])
    assert "--method" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run.main(["e.py", "--mesh", "--mesh-method", "dual"])
    assert "--mesh-method" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run.main(["e.py", "--mesh-method", "cubes"])
    assert "--mesh-method needs --mesh" in capsys.readouterr().err


def test_binding_and_header_name_the_entry_points():
    from splatam_amd import _capi
    header = open(os.path.join(HERE, "..", "include", "splat_hip.h")).read()
    L = _capi.lib()
    for name in ("splat_tsdf_cubes", "splat_tsdf_sparse_cubes", "splat_tsdf_cubes_table"):
        assert hasattr(L, name) and name in _capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert L.splat_abi_version() == 17 and _capi.ABI_VERSION == 17
    # refusals and the table need no device: nothing is launched
    assert L.splat_tsdf_cubes(None, 1.0, None, 0, None, None) == 1 and L.splat_tsdf_sparse_cubes(None, 1.0, None, 0, None, None) == 1
    assert L.splat_tsdf_cubes_table(None) == 1
    from splatam_amd.mesh import cubes_table
    assert cubes_table().tolist() == Q.table().tolist()
