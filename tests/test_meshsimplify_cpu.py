"""The mesh simplification layer without a GPU: splatam_amd/csrc/meshsimplify_math.h compiled for the host
(tests/meshsimplify_math_shim.cpp: the loop bodies of the kernels of csrc/meshsimplify.hip, its atomics as plain loads and stores)
against the numpy restatement tests/meshsimplify_ref.py.

1. KEYS AND IDS: negative coordinates, x = j cell exactly, +-0, denormals, NaN / inf, |i| = 2^20 - 1 against 2^20; ids equal the
   restatement's for the given and a shuffled vertex order.
2. SUMS: the count and all 16 int64 words per cluster equal the restatement's EXACTLY, faces in the given, reversed and shuffled order,
   on a welded 24 x 24-per-side unit cube shifted by 0.013 at cell 0.05 / 0.1 / 0.17, a 48-ring unit sphere and a jittered tilted
   planar grid with a boundary; a face inside one cluster adds once, one across two once to each; |d| <= sqrt(3) / 2 throughout.
3. PLACEMENT: on the cube the restatement flags NO fragile cluster, and the header's points (cyclic Jacobi) equal the ``eigh`` solve
   within POSITION_BOUND cells; the cube's facts to 1e-6 m; ``placement="mean"`` misses the corners by more than cell / 4; the
   plane's interior vertices lie on the plane.  The unit sphere is NOT usable for the comparison of positions: at tau = 1e-3 its third
   eigenvalue sits on the threshold (most of its clusters are fragile, the restatement says so and the test asserts it), so two
   correct solvers may take different branches there.  It serves items 2, 4 and 5 only.
4. INVARIANTS, every case and both placements.
5. CANONICAL OUTPUT: vertices and faces permuted give the same vertex and colour bytes and the same set of faces.
6. EDGE SEMANTICS.
7. The header as a stand-alone program under the address and undefined-behaviour sanitizers.
8. PLUMBING."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import meshsimplify_ref as Q

# The largest |p_header - p_eigh| seen on the machine the layer was written on (profiles/mesh_simplify.md): 0 on the axis-aligned cube
# at the three cell sizes and on the plane (diagonal quadrics, and means that already lie on the plane), 7.2e-16 cells on the same
# cube turned by 0.35 rad about (1, 2, 3), where the quadrics are full matrices.  Ten times the largest, and in no case above 1e-6
# cell, which is below the output's own float32 rounding.
POSITION_BOUND = min(10 * 7.2e-16, 1e-6)
CUBE_SHIFT = 0.013
CELLS = (0.05, 0.1, 0.17)


@pytest.fixture(scope="module")
def shim():
    return Q.load_shim()


def colours_of(v, seed=1):
    return np.random.default_rng(seed).random((len(v), 3)).astype(np.float32)


def cases():
    out = {}
    v, f = Q.welded_cube(24, (CUBE_SHIFT,) * 3)
    for cell in CELLS:
        out[f"cube-{cell}"] = (v, f, colours_of(v), cell, True)
    v, f = Q.uv_sphere(48)
    out["sphere-0.1"] = (v, f, None, 0.1, True)
    v, f = Q.torus()
    out["torus-0.17"] = (v, f, colours_of(v), 0.17, True)
    v, f = Q.tilted_plane()
    out["plane-0.1"] = (v, f, colours_of(v), 0.1, False)
    return out


CASES = cases()
_results = {}


def solved(shim, name, placement="quadric", dedupe=True):
    """(restatement, header) results with details, each computed once."""
    key = (name, placement, dedupe)
    if key not in _results:
        v, f, c, cell, _ = CASES[name]
        _results[key] = (Q.simplify(v, f, c, cell, placement, dedupe, details=True), Q.simplify(v, f, c, cell, placement, dedupe, shim=shim, details=True))
    return _results[key]


# ---------------------------------------------------------------------------------------------------------------- 1. keys and ids
def test_keys_floor_signs_exact_multiples_and_the_range(shim):
    cell = 0.25
    L, tiny = 1 << 20, np.float32(1e-45)
    edge = np.float32(2.0 ** 18)                                        # 2^20 cells of 0.25
    v = np.array([[0.0, -0.0, tiny], [-tiny, 0.25, -0.25], [0.5, -0.5, 0.7499999], [-0.2500001, 1e-40, -1e-40],
                  [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],
                  [edge - 0.25, -(edge - 0.25), 0], [edge, 0, 0], [0, -edge, 0], [0, 0, -(edge + 0.25)]], dtype=np.float32)
    got, want = Q.shim_keys(shim, v, cell), Q.keys(v, cell)
    assert np.array_equal(got, want)
    key = lambda ix, iy, iz: ((iz + L) << 42) | ((iy + L) << 21) | (ix + L)         # noqa: E731
    assert got[0] == key(0, 0, 0)                                       # +-0 and the smallest denormal: cell 0
    assert got[1] == key(-1, 1, -1)                                     # the smallest negative denormal: cell -1; x = j cell: cell j, both signs
    assert got[2] == key(2, -2, 2) and got[3] == key(-2, 0, -1)
    assert (got[4:7] == -1).all()
    assert got[7] == key(L - 1, -(L - 1), 0) and (got[8:] == -1).all()   # |i| = 2^20 - 1 is inside, 2^20 is not
    assert got[got >= 0].max() < 1 << 63 and len(set(got[[0, 1, 2, 3, 7]])) == 5
    rng = np.random.default_rng(4)
    w = (rng.normal(size=(5000, 3)) * 3).astype(np.float32)
    w[::7] = np.round(w[::7] / 0.1) * np.float32(0.1)
    for c in (0.1, 0.013, 1.0, 1e-3):
        assert np.array_equal(Q.shim_keys(shim, w, c), Q.keys(w, c)), c


def test_ids_are_ranks_of_the_keys_in_any_vertex_order(shim):
    rng = np.random.default_rng(6)
    v, _ = Q.welded_cube(24, (CUBE_SHIFT,) * 3)
    v = np.concatenate((v, np.array([[np.nan, 0, 0], [1e30, 0, 0]], dtype=np.float32)))
    k = Q.shim_keys(shim, v, 0.1)
    ids = Q.cluster_ids(k)
    live = k >= 0
    assert (ids[~live] == -1).all() and (~live).sum() == 2
    order = np.argsort(k[live], kind="stable")
    assert (np.diff(ids[live][order]) >= 0).all() and ids.max() + 1 == len(np.unique(k[live])) == 602
    assert np.array_equal(np.unique(k[live])[ids[live]], k[live])        # ascending key order
    perm = rng.permutation(len(v))
    assert np.array_equal(Q.cluster_ids(Q.shim_keys(shim, v[perm], 0.1)), ids[perm])
    # ... and the module's own glue (a stable sort, a flag, a prefix sum) on the host
    import torch
    from splatam_amd.mesh_simplify import cluster_ids
    assert np.array_equal(cluster_ids(torch.from_numpy(k)).numpy(), ids)
    assert np.array_equal(cluster_ids(torch.from_numpy(k[perm])).numpy(), ids[perm])
    assert cluster_ids(torch.zeros(0, dtype=torch.int64)).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- 2. sums
@pytest.mark.parametrize("name", list(CASES))
def test_sums_equal_the_restatement_for_every_face_order(shim, name):
    v, f, c, cell, _ = CASES[name]
    cluster = Q.cluster_ids(Q.keys(v, cell))
    count, acc, refused, ds = Q.sums(v, f, c, cell, cluster)
    assert refused == 0 and len(ds) > len(f) / 2 and (ds <= np.sqrt(3) / 2).all()
    orders = {"given": f, "reversed": f[::-1], "shuffled": f[np.random.default_rng(3).permutation(len(f))]}
    for order, faces in orders.items():
        got_count, got, got_refused, worst, contributions = Q.shim_sums(shim, v, faces, c, cell, cluster)
        assert np.array_equal(got_count, count) and got_refused == 0, (name, order)
        assert np.array_equal(got, acc), (name, order, np.argwhere(got != acc)[:4])
        assert worst == ds.max() <= np.sqrt(3) / 2 and contributions == len(ds)
    assert count.sum() == len(v) and (acc[count == 0] == 0).all()
    area = acc[:, [6, 9, 11]].sum(axis=1)                               # the trace of area n n^T: the area, once per cluster a face touches
    assert (area[count > 0] > 0).all() and (acc[:, 15] >= 0).all()
    print(f"{name}: {int((count > 0).sum())} clusters, {len(ds)} contributions of {len(f)} faces, largest |d| {ds.max():.6f}")


def test_a_face_adds_once_per_distinct_cluster(shim):
    cell = 1.0
    v = np.array([[0.1, 0.1, 0.2], [0.8, 0.2, 0.3], [0.3, 0.7, 0.6], [1.4, 0.3, 0.2], [1.2, 0.8, 0.9]], dtype=np.float32)
    cluster = Q.cluster_ids(Q.keys(v, cell))
    assert cluster.tolist() == [0, 0, 0, 1, 1]
    for face, adds in (([0, 1, 2], [1, 0]), ([0, 1, 3], [1, 1]), ([3, 0, 4], [1, 1]), ([3, 4, 3], [0, 0])):
        f = np.array([face], dtype=np.int32)
        _, acc, _, worst, contributions = Q.shim_sums(shim, v, f, None, cell, cluster)
        assert np.array_equal(acc, Q.sums(v, f, None, cell, cluster)[1])
        area2 = np.linalg.norm(np.cross(v[face[1]].astype(np.float64) - v[face[0]], v[face[2]].astype(np.float64) - v[face[0]]))
        traces = acc[:2, [6, 9, 11]].sum(axis=1) * 2.0 ** -40
        assert contributions == sum(adds) and np.allclose(traces, 0.5 * area2 * np.array(adds), atol=3 * 2.0 ** -40), (face, traces)


# ---------------------------------------------------------------------------------------------------------------- 3. placement
def cube_surface_distance(p):
    """0 for a point on the surface of the shifted unit cube."""
    q = p.astype(np.float64) - CUBE_SHIFT
    inside_box = np.maximum(np.maximum(-q, q - 1.0), 0.0).max(axis=1)   # how far outside
    to_face = np.minimum(np.abs(q), np.abs(q - 1.0)).min(axis=1)        # how far from the nearest face's plane
    return np.maximum(inside_box, to_face)


@pytest.mark.parametrize("cell", CELLS)
def test_placement_on_the_cube(shim, cell):
    name = f"cube-{cell}"
    ref, got = solved(shim, name)
    rp, gp = ref[4]["placed"], got[4]["placed"]
    live = rp["live"]
    assert live.sum() == {0.05: 2402, 0.1: 602, 0.17: 152}[cell]
    assert not rp["fragile"].any(), "the cube must have no cluster where rounding decides a branch"
    diff = np.abs(rp["p"][live] - gp["p"][live]).max()
    print(f"{name}: largest |p_header - p_eigh| {diff:.3e} cells over {int(live.sum())} clusters (bound {POSITION_BOUND:.3e})")
    assert diff <= POSITION_BOUND
    assert np.array_equal(rp["rank"], gp["rank"]) and np.array_equal(rp["fallback"], gp["fallback"])
    nv, nf, nc, report = got[:4]
    assert report["fallbacks"] == 0 and report["cells"] == report["vertices_kept"] == len(nv) == live.sum()
    assert cube_surface_distance(nv).max() <= 1e-6                      # every output vertex is on the cube's surface
    on = (np.abs(nv.astype(np.float64) - CUBE_SHIFT) < 1e-6) | (np.abs(nv.astype(np.float64) - CUBE_SHIFT - 1) < 1e-6)
    rank = gp["rank"][live]
    assert np.array_equal(on.sum(axis=1), rank)                         # on three face planes: a corner; on two: an edge; on one: a face
    assert (rank == 3).sum() == 8 == report["rank3"] and report["rank2"] == (rank == 2).sum() > 0 and report["rank1"] == (rank == 1).sum() > 0
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64) + CUBE_SHIFT
    miss = np.array([np.abs(nv.astype(np.float64) - k).max(axis=1).min() for k in corners])
    print(f"{name}: corners missed by at most {miss.max():.3e} m, rms plane distance {report['rms_plane_distance_m']:.3e} m")
    assert miss.max() <= 1e-6
    assert report["rms_plane_distance_m"] < 1e-6 and ref[3]["rms_plane_distance_m"] < 1e-6
    # the mean instead: the corner vertices miss the corners by more than cell / 4 -- the quadrics do the work
    mv = solved(shim, name, "mean")[1][0]
    # (a corner that is ALONE in its cell -- all eight at cell 0.05, finer than 1.2 of the cube's 1/24 quads, and the far corner at
    # 0.1 -- is its own mean; every corner that shares its cell is missed)
    at = np.array([np.abs(nv.astype(np.float64) - k).max(axis=1).argmin() for k in corners])           # the corners' clusters
    assert len(mv) == len(nv) and (rank[at] == 3).all()
    mean_miss = np.abs(mv[at].astype(np.float64) - corners).max(axis=1)
    shared = got[4]["count"][live][at] > 1
    print(f"{name}: with the mean the {int(shared.sum())} corners that share their cell are missed by "
          f"{mean_miss[shared].min() if shared.any() else 0:.4f} .. {mean_miss.max():.4f} m (cell / 4 = {cell / 4:.4f})")
    assert shared.sum() == {0.05: 0, 0.1: 7, 0.17: 8}[cell]
    assert (mean_miss[shared] > cell / 4).all() and (mean_miss[~shared] <= 1e-6).all()
    assert solved(shim, name, "mean")[1][3]["rank1"] == 0 and solved(shim, name, "mean")[1][3]["rms_plane_distance_m"] == 0.0


@pytest.mark.parametrize("cell", CELLS)
def test_placement_on_the_turned_cube(shim, cell):
    """The same cube turned by 0.35 rad about (1, 2, 3): full 3 x 3 quadrics, so the Jacobi sweeps and ``eigh`` both have work to do."""
    from tests.util import rigid_w2c
    v, f = Q.welded_cube(24, (CUBE_SHIFT,) * 3)
    M = rigid_w2c(0.35, (1.0, 2.0, 3.0), (0.1, -0.07, 0.2)).astype(np.float64)
    v = (v.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    ref, got = (Q.simplify(v, f, None, cell, shim=s, details=True) for s in (None, shim))
    rp, gp = ref[4]["placed"], got[4]["placed"]
    live = rp["live"]
    assert not rp["fragile"].any() and np.array_equal(ref[4]["sums"], got[4]["sums"])
    diff = np.abs(rp["p"][live] - gp["p"][live]).max()
    print(f"turned cube, cell {cell}: largest |p_header - p_eigh| {diff:.3e} cells over {int(live.sum())} clusters (bound {POSITION_BOUND:.3e})")
    assert diff <= POSITION_BOUND
    assert np.array_equal(rp["rank"], gp["rank"]) and np.array_equal(rp["fallback"], gp["fallback"]) and got[3]["rank3"] == 8
    assert np.array_equal(ref[1], got[1]) and np.abs(ref[0].astype(np.float64) - got[0]).max() <= 1e-6 * cell + 2.0 ** -23 * 2


def test_the_sphere_is_fragile_and_the_plane_is_not(shim):
    ref, got = solved(shim, "sphere-0.1")
    fragile, live = ref[4]["placed"]["fragile"], ref[4]["placed"]["live"]
    print(f"sphere: {int(fragile.sum())} of {int(live.sum())} clusters are fragile")
    assert fragile.sum() > live.sum() / 2                               # why it takes no part in the comparison of positions
    ref, got = solved(shim, "plane-0.1")
    rp, gp = ref[4]["placed"], got[4]["placed"]
    assert not rp["fragile"].any() and (gp["rank"][gp["live"]] == 1).all()
    diff = np.abs(rp["p"][rp["live"]] - gp["p"][gp["live"]]).max()
    print(f"plane: largest |p_header - p_eigh| {diff:.3e} cells (bound {POSITION_BOUND:.3e})")
    assert diff <= POSITION_BOUND
    nv = got[0].astype(np.float64)
    off = np.abs((nv - Q.PLANE_POINT) @ Q.PLANE_NORMAL)
    print(f"plane: vertices off the plane by at most {off.max():.3e} m")
    assert off.max() <= 1e-6                                            # interior and boundary alike: a plane's quadric has rank 1


# ---------------------------------------------------------------------------------------------------------------- 4. invariants
@pytest.mark.parametrize("placement", ("quadric", "mean"))
@pytest.mark.parametrize("name", list(CASES))
def test_invariants(shim, name, placement):
    v, f, c, cell, closed = CASES[name]
    for dedupe in (True, False):
        ref, got = solved(shim, name, placement, dedupe)
        assert np.array_equal(ref[1], got[1])                           # the faces are integers: the same from both
        for out in (ref, got):
            Q.check_invariants(v, f, c, cell, out[:3], dedupe, closed)
        report = got[3]
        assert report["vertices"] == len(v) and report["faces"] == len(f)
        assert report["vertices_kept"] == len(got[0]) < len(v) and report["faces_kept"] == len(got[1]) < len(f)
        if c is not None:
            assert got[2].shape == got[0].shape and got[2].min() >= 0 and got[2].max() <= 1
            assert np.array_equal(ref[2], got[2])                       # colours are means of integers: the same bits
    assert len(solved(shim, name, placement, False)[1][1]) >= len(solved(shim, name, placement, True)[1][1])


def test_dedupe_keeps_the_face_of_lowest_index(shim):
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.4, 0.5], [1.4, 0.6, 0.5], [0.4, 1.6, 0.5]], dtype=np.float32)
    f = np.array([[4, 5, 3], [0, 1, 2], [2, 0, 1], [0, 2, 1], [3, 4, 5]], dtype=np.int32)
    nv, nf, _, rep = Q.simplify(v, f, None, 1.0, shim=shim)
    assert nf.tolist() == [[0, 1, 2], [0, 2, 1]] and rep["faces_kept"] == 2          # faces 0 and 3 (the opposite-wound twin is not paired off)
    nv, nf, _, rep = Q.simplify(v, f, None, 1.0, dedupe=False, shim=shim)
    assert nf.tolist() == [[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 2, 1], [0, 1, 2]]


# ---------------------------------------------------------------------------------------------------------------- 5. canonical output
@pytest.mark.parametrize("name", ("cube-0.1", "sphere-0.1", "plane-0.1"))
def test_output_does_not_depend_on_the_order_of_the_input(shim, name):
    v, f, c, cell, _ = CASES[name]
    rng = np.random.default_rng(17)
    perm = rng.permutation(len(v))
    if c is None:
        pv, pf = Q.renumbered(v, f, perm)
        pc = None
    else:
        pv, pf, pc = Q.renumbered(v, f, perm, c)
    pf = pf[rng.permutation(len(pf))]
    for dedupe in (True, False):
        a = solved(shim, name, "quadric", dedupe)[1]
        b = Q.simplify(pv, pf, pc, cell, dedupe=dedupe, shim=shim)
        assert a[0].tobytes() == b[0].tobytes()
        assert (a[2] is None and b[2] is None) or a[2].tobytes() == b[2].tobytes()
        key = lambda t: np.unique(t, axis=0, return_counts=True)        # noqa: E731
        ka, kb = key(a[1]), key(b[1])
        assert np.array_equal(ka[0], kb[0]) and np.array_equal(ka[1], kb[1])


# ---------------------------------------------------------------------------------------------------------------- 6. edge semantics
def edge_mesh():
    v = np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [np.nan, 0.1, 0.1], [2.1, 0.1, 0.1], [3.1, 0.1, 0.1], [4.1, 0.1, 0.1],
                  [9.0, 9.0, 9.0], [1.2, 1.2, 0.3]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 0, 1], [0, 1, 9], [-1, 0, 1], [0, 3, 1], [4, 5, 6], [1, 8, 2], [2 ** 31 - 1, 0, 1]], dtype=np.int32)
    c = np.linspace(0, 1, 27, dtype=np.float32).reshape(9, 3)
    return v, f, c


@pytest.mark.parametrize("placement", ("quadric", "mean"))
def test_edge_semantics(shim, placement):
    v, f, c = edge_mesh()
    nv, nf, nc, rep, d = Q.simplify(v, f, c, 1.0, placement, shim=shim, details=True)
    ref = Q.simplify(v, f, c, 1.0, placement)
    # the repeated index, the two indices out of range and the NaN vertex lose their faces; the others stay
    assert d["keep"].tolist() == [True, False, False, False, False, True, True, False]
    assert np.array_equal(nf, ref[1]) and np.array_equal(nc, ref[2]) and np.abs(nv.astype(np.float64) - ref[0]).max() < 1e-6
    # the zero-area face across three cells adds nothing to the quadrics and still survives as a face
    g = d["cluster"][[4, 5, 6]]
    assert (d["sums"][g, 6:] == 0).all() and len(set(g)) == 3
    if placement == "quadric":
        assert (d["placed"]["fallback"][g] == 1).all() and rep["fallbacks"] >= 3
        assert np.array_equal(nv[nf[1]], v[[4, 5, 6]])                  # ... at the means, which are the vertices themselves
    # the unreferenced vertex (7) has a cluster and no place in the output; the NaN vertex has neither
    assert d["cluster"][7] >= 0 and d["cluster"][3] == -1 and len(nv) == 7 and rep["cells"] == 8
    assert not np.isin(nv, v[7]).all(axis=1).any()
    assert rep["vertices"] == 9 and rep["faces"] == 8 and rep["faces_kept"] == 3 and rep["vertices_kept"] == 7
    without = Q.simplify(v, f, None, 1.0, placement, shim=shim)
    assert without[2] is None and without[0].tobytes() == nv.tobytes() and np.array_equal(without[1], nf)


def test_empty_inputs_one_cell_and_refusals(shim):
    v, f, c = edge_mesh()
    none = np.zeros((0, 3), dtype=np.int32)
    for mesh in ((v, none, c), (v[:0], none, None), (v[:0], f, c[:0])):
        nv, nf, nc, rep = Q.simplify(*mesh, 1.0, shim=shim)
        assert nv.shape == (0, 3) and nf.shape == (0, 3) and rep["faces_kept"] == 0 and rep["cells"] == 0
    nv, nf, nc, rep = Q.simplify(v[:3], f[:1], c[:3], 10.0, shim=shim)    # everything in one cell: the empty mesh
    assert nv.shape == (0, 3) and nf.shape == (0, 3) and nc.shape == (0, 3) and rep["cells"] == 1 and rep["faces_kept"] == 0
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            Q.simplify(v, f, c, bad, shim=shim)
    with pytest.raises(ValueError, match="2\\^20"):
        Q.simplify(v, f, c, 1e-6, shim=shim)                            # 9 m / 1e-6 m: a key out of range
    big = np.array([[-3e19, -3e19, 0], [3e19, -3e19, 0], [0, 3e19, 0]], dtype=np.float32)
    with pytest.raises(ValueError, match="area"):
        Q.simplify(big, np.array([[0, 1, 2]], dtype=np.int32), None, 1e14, shim=shim)


# ---------------------------------------------------------------------------------------------------------------- 7. sanitizers
def test_header_under_address_and_ub_sanitizers(tmp_path):
    """The shim's host functions as a stand-alone program (its own main) built with -fsanitize=address,undefined, on the degenerate
    inputs of item 6 and more: V = 0 and F = 0, repeated and out-of-range indices (INT32_MIN / INT32_MAX among them), vertices and
    colours that are NaN, infinite, -0 and denormal, a face of infinite area, clusters that are not the call's own, and placement from
    words that mean nothing.  Any sanitizer report or wrong answer is a non-zero exit.  The runtimes are linked statically; nothing
    loaded into python is involved."""
    exe = str(tmp_path / "meshsimplify_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DMESHSIMPLIFY_SHIM_MAIN", "-o", exe,
                           os.path.join(os.path.dirname(__file__), "meshsimplify_math_shim.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout


# ---------------------------------------------------------------------------------------------------------------- 8. plumbing
ENTRIES = ("splat_mesh_simplify_keys", "splat_mesh_simplify_vertices", "splat_mesh_simplify_quadrics", "splat_mesh_simplify_place",
           "splat_mesh_simplify_faces")


def test_binding_and_header_name_the_entry_points(shim):
    from splatam_amd import _capi
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "splat_hip.h")).read()
    L = _capi.lib()
    for name in ENTRIES:
        assert hasattr(L, name) and name in _capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert _capi.SPLAT_MESH_SIMPLIFY_SUMS == int(re.search(r"#define SPLAT_MESH_SIMPLIFY_SUMS (\d+)", header).group(1)) == shim.sqs_num_sums() == 16
    assert L.splat_abi_version() == 17 and _capi.ABI_VERSION == 17 and "#define SPLAT_ABI_VERSION 17 " in header
    p = 1 << 12
    # refusals need no device: nothing is launched

    def refused(fn, ok, nulls, negatives, cell_at):
        for k in nulls:
            args = list(ok)
            args[k] = None
            assert fn(*args) == 1, (fn.__name__, k)
        for k in negatives:
            args = list(ok)
            args[k] = -1
            assert fn(*args) == 1, (fn.__name__, k)
        for bad in (0.0, -0.1, float("inf"), float("nan")):
            args = list(ok)
            args[cell_at] = bad
            assert fn(*args) == 1, (fn.__name__, bad)

    refused(L.splat_mesh_simplify_keys, [p, 4, 0.1, p, None], (0, 3), (1,), 2)
    refused(L.splat_mesh_simplify_vertices, [p, p, 4, p, 0.1, p, p, None], (0, 3, 5, 6), (2,), 4)
    refused(L.splat_mesh_simplify_quadrics, [p, 4, p, 4, p, 0.1, p, p, None], (0, 2, 4, 6, 7), (1, 3), 5)
    refused(L.splat_mesh_simplify_place, [p, p, p, 4, 0.1, 1, p, p, p, p, p, None], (0, 1, 2, 6, 8, 9, 10), (3,), 4)
    assert L.splat_mesh_simplify_place(p, p, p, 4, 0.1, 2, p, p, p, p, p, None) == 1          # a placement that does not exist
    ok = [p, 4, 4, p, p, None]
    for k, bad in ((0, None), (3, None), (4, None), (1, -1), (2, -1)):
        args = list(ok)
        args[k] = bad
        assert L.splat_mesh_simplify_faces(*args) == 1, k
    # empty inputs succeed without a launch (there is no device here to launch on)
    assert L.splat_mesh_simplify_keys(None, 0, 0.1, None, None) == 0
    assert L.splat_mesh_simplify_vertices(None, None, 0, None, 0.1, None, None, None) == 0
    assert L.splat_mesh_simplify_quadrics(None, 0, None, 0, None, 0.1, None, None, None) == 0
    assert L.splat_mesh_simplify_place(None, None, None, 0, 0.1, 1, None, None, None, None, None, None) == 0
    assert L.splat_mesh_simplify_faces(None, 0, 0, None, None, None) == 0


def test_there_is_no_cpu_path():
    import torch
    from splatam_amd import mesh_simplify as MS
    v, f = Q.welded_cube(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MS.simplify_mesh((v, f, None), 0.5, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        MS.cell_keys(torch.from_numpy(v), 0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            MS.simplify_mesh((v, f, None), bad)
    with pytest.raises(ValueError, match="placement"):
        MS.simplify_mesh((v, f, None), 0.5, placement="median")


def test_simplification_is_off_by_default_and_signatures_stay(capsys):
    from splatam_amd import mesh as M
    from splatam_amd import mesh_clean as MC
    from splatam_amd import mesh_render as MR
    from splatam_amd import mesh_score as S
    from splatam_amd import mesh_simplify as MS
    from splatam_amd import run
    # what the existing tests say of the signatures
    ex = inspect.signature(M.extract_mesh).parameters
    assert list(ex)[-2:] == ["method", "clean"] and ex["clean"].default is None and ex["method"].default == "tetrahedra"
    assert [(k, p.default) for k, p in inspect.signature(MC.clean_mesh).parameters.items()][1:] == [
        ("min_vertices", 200), ("min_faces", 0), ("min_area", 0.0), ("min_extent", 0.0), ("keep_largest", None), ("transform", None),
        ("device", "cuda:0"), ("report", False)]
    assert [(k, p.default) for k, p in inspect.signature(S.score_mesh).parameters.items()][2:] == [
        ("samples", 200_000), ("threshold", 0.05), ("seed", 0), ("transform", None), ("device", "cuda:0"), ("cell", None), ("align", False)]
    assert list(inspect.signature(S.score_with_views).parameters)[-1] == "align"
    assert [(k, p.default) for k, p in inspect.signature(MR.cull_mesh).parameters.items()][4:] == [
        ("occlusion", None), ("eps", 0.03), ("edge", 0), ("rule", "all"), ("chunk", 16), ("transform", None), ("near", MR.NEAR), ("device", "cuda:0")]
    assert [(k, p.default) for k, p in inspect.signature(MS.simplify_mesh).parameters.items()][1:] == [
        ("cell", inspect.Parameter.empty), ("placement", "quadric"), ("dedupe", True), ("transform", None), ("device", "cuda:0"), ("report", False)]
    # off by default
    from_params = inspect.signature(M.mesh_from_params).parameters
    assert from_params["simplify"].default is None and from_params["simplification"].default is None
    assert M._parser().parse_args(["p.npz", "--out", "m.ply"]).simplify is None
    assert run._parser().parse_args(["experiment.py"]).simplify_mesh is None
    args = M._parser().parse_args(["p.npz", "--out", "m.ply", "--simplify", "0.03", "--simplify-placement", "mean"])
    assert args.simplify == 0.03 and args.simplify_placement == "mean"
    with pytest.raises(SystemExit):
        M.main(["params.npz", "--out", "mesh.ply", "--simplify-placement", "mean"])
    assert "--simplify-placement needs --simplify" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run.main(["experiment.py", "--simplify-mesh", "0.03"])
    assert "--simplify-mesh needs --mesh" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        MS.main(["in.ply", "out.ply"])                                  # --cell is required
    assert "--cell" in capsys.readouterr().err
    args = MS._parser().parse_args(["in.ply", "out.ply", "--cell", "0.02"])
    assert args.placement == "quadric" and not args.no_dedupe and args.transform is None
    # the options
    for off in (None, False):
        assert MS.simplify_options(off) is None
    assert MS.simplify_options(0.03) == {"cell": 0.03} and MS.simplify_options(dict(cell=1, placement="mean")) == {"cell": 1.0, "placement": "mean"}
    for bad in (True, "0.03", dict(placement="mean"), dict(cell=0.03, size=2), 0, -1.0, dict(cell=0.03, placement="median")):
        with pytest.raises(ValueError):
            MS.simplify_options(bad)
    report = dict(vertices=1000, faces=2000, vertices_kept=100, faces_kept=210, cells=120, fallbacks=2, rank1=90, rank2=20, rank3=8,
                  rms_plane_distance_m=0.00012346)
    assert MS.format_simplification(report) == ("Simplification: 100 of 1000 vertices (10.00 %), 210 of 2000 faces (10.50 %), 120 cells "
                                                "(plane 90, edge 20, corner 8, mean 2), RMS distance from the replaced planes 0.1235 mm")
    assert "decimation" not in MC.__doc__.split("Not here:")[1]
