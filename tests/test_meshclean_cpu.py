"""The mesh cleaning layer without a GPU: splatam_amd/csrc/meshclean_math.h compiled for the host (tests/meshclean_math_shim.cpp: the loop
bodies of the kernels of csrc/meshclean.hip, its atomics as plain loads and stores) against the numpy restatement tests/meshclean_ref.py.

1. LABELS: find / link / flatten through the shim equal the restatement EXACTLY -- the smallest vertex index of every component, not
   merely the same partition -- for the faces in the given, the reversed and a seeded shuffled order, with ``parent[v] <= v`` asserted
   after every link; links from candidates that are no roots (what a lane with stale answers does) keep the invariant and the labels.
   Where scipy is installed the restatement's partition is cross-checked against ``scipy.sparse.csgraph.connected_components``.
2. STATISTICS: counts and boxes equal the restatement's; the quantised area equals the sum of the double areas within
   ``num_faces 2^-41`` (half a quantum per face: rint); the float-bit key is monotone over negative, zero, positive and denormal values
   and its own inverse.
3. The header as a stand-alone program under the address and undefined-behaviour sanitizers, on degenerate inputs.
4. PLUMBING: the entry points exist, the ABI is still 17, NULL pointers and negative sizes are refused, ``device="cpu"`` raises the
   module's "no CPU path" error, and without ``clean`` the signature defaults and result keys of ``score_mesh``, ``extract_mesh`` and
   ``cull_mesh`` are as they were."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import meshclean_ref as K
import meshscore_ref as R
from tests.util import host_shim

F32P, I32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def load_shim():
    lib = host_shim("meshclean_math_shim", "meshclean_math.h", "meshscore_math.h")
    lib.mcs_link.restype = C.c_int
    lib.mcs_link.argtypes = [I32P, C.c_int32, C.c_int32, I32P, C.c_int]
    lib.mcs_invariant.restype = C.c_int
    lib.mcs_invariant.argtypes = [I32P, C.c_int32]
    lib.mcs_flatten.restype = None
    lib.mcs_flatten.argtypes = [I32P, C.c_int32]
    lib.mcs_link_roots.restype = None
    lib.mcs_link_roots.argtypes = [I32P, C.c_int32, C.c_int32]
    lib.mcs_find.restype = C.c_int32
    lib.mcs_find.argtypes = [I32P, C.c_int32]
    lib.mcs_stats.restype = None
    lib.mcs_stats.argtypes = [F32P, C.c_int32, I32P, C.c_int32, I32P, I32P, I32P, I64P, I32P, I32P]
    lib.mcs_float_key.restype = C.c_int32
    lib.mcs_float_key.argtypes = [C.c_float]
    lib.mcs_key_float.restype = C.c_float
    lib.mcs_key_float.argtypes = [C.c_int32]
    lib.mcs_area_quanta.restype = C.c_int64
    lib.mcs_area_quanta.argtypes = [C.c_double]
    lib.mcs_area_bad.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _p(a, t):
    return a.ctypes.data_as(t)


def shim_labels(shim, V, faces, check=True):
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    parent = np.empty(V, dtype=np.int32)
    assert shim.mcs_link(_p(f, I32P), len(f), V, _p(parent, I32P), int(check)) == 0, "parent[v] <= v was violated after a link"
    forest = parent.copy()
    shim.mcs_flatten(_p(parent, I32P), V)
    assert shim.mcs_invariant(_p(parent, I32P), V) == 0
    return parent, forest


def shim_stats(shim, vertices, faces, labels):
    v, f = np.ascontiguousarray(vertices, dtype=np.float32), np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    lab, V = np.ascontiguousarray(labels, dtype=np.int32), len(vertices)
    nv, nf, q = np.empty(V, np.int32), np.empty(V, np.int32), np.empty(V, np.int64)
    lo, hi = np.empty((V, 3), np.int32), np.empty((V, 3), np.int32)
    shim.mcs_stats(_p(v, F32P), V, _p(f, I32P), len(f), _p(lab, I32P), _p(nv, I32P), _p(nf, I32P), _p(q, I64P), _p(lo, I32P), _p(hi, I32P))
    return nv, nf, q, lo, hi


def unkey(k):
    k = np.asarray(k, dtype=np.int32)
    return np.where(k >= 0, k, k ^ np.int32(0x7fffffff)).astype(np.int32).view(np.float32)


def label_cases():
    rng = np.random.default_rng(7)
    out = {}
    v, f = K.strip(600)
    out["strip-ascending"] = (len(v), f)
    out["strip-descending"] = (len(v), (len(v) - 1 - f).astype(np.int32))
    out["strip-permuted"] = (len(v), K.renumbered(v, f, rng.permutation(len(v)))[1])
    v, f = K.join([K.grid(9, 7), K.cube(), K.cube(), K.tetrahedron((1, 1, 1)), K.strip(5)])
    v, f = K.renumbered(v, f, rng.permutation(len(v)))
    out["several"] = (len(v) + 3, f)                                    # (three vertices no face names)
    bow = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    out["bow-tie"] = (5, bow)
    out["degenerate"] = (8, np.array([[5, 5, 5], [1, 1, 2], [3, 4, 9], [-1, 0, 1], [4, 3, 3], [7, 2, 2]], dtype=np.int32))
    out["random-graph"] = (400, rng.integers(0, 400, size=(150, 3)).astype(np.int32))
    out["no-faces"] = (6, np.zeros((0, 3), dtype=np.int32))
    return out


LABEL_CASES = label_cases()


# ---------------------------------------------------------------------------------------------------------------- 1. labels
@pytest.mark.parametrize("name", list(LABEL_CASES))
def test_labels_equal_the_restatement_for_every_face_order(shim, name):
    V, f = LABEL_CASES[name]
    want, rounds = K.labels(V, f)
    assert np.array_equal(want[want], want) and (want <= np.arange(V)).all()
    orders = {"given": f, "reversed": f[::-1], "shuffled": f[np.random.default_rng(3).permutation(len(f))]}
    for order, faces in orders.items():
        got, forest = shim_labels(shim, V, faces)
        depth = 0
        if V:
            walk = forest.copy()
            while not np.array_equal(walk[walk], walk):
                walk, depth = walk[walk], depth + 1
        print(f"{name}/{order}: {len(np.unique(want))} components, restatement {rounds} rounds, forest depth <= 2^{depth}")
        assert np.array_equal(got, want), (name, order)
    if name == "bow-tie":
        assert (want == 0).all()
    if name == "degenerate":
        assert want.tolist() == [0, 1, 1, 3, 3, 5, 6, 1]


def test_links_from_stale_candidates_keep_the_invariant_and_the_labels(shim):
    """A lane whose finds returned indices that are no longer roots hands them to ``mc_link_roots``: the compare-and-swap fails and names
    the current parent, from which the walk goes on.  Every such call keeps ``parent[v] <= v`` and never splits or wrongly joins."""
    rng = np.random.default_rng(11)
    V, f = LABEL_CASES["several"]
    want = K.labels(V, f)[0]
    parent = np.empty(V, dtype=np.int32)
    assert shim.mcs_link(_p(np.ascontiguousarray(f), I32P), len(f), V, _p(parent, I32P), 0) == 0
    members = [np.flatnonzero(want == r) for r in np.unique(want) if (want == r).sum() > 3]
    for _ in range(300):
        m = members[rng.integers(len(members))]
        a, b = (int(x) for x in rng.choice(m, size=2))                  # any two vertices of one component, roots or not
        shim.mcs_link_roots(_p(parent, I32P), a, b)
        assert shim.mcs_invariant(_p(parent, I32P), V) == 0
    for v in range(V):
        assert shim.mcs_find(_p(parent, I32P), v) == want[v]
    # ... and joining two components through non-roots gives the smaller of the two labels to both
    r0, r1 = (int(m[0]) for m in members[:2])
    shim.mcs_link_roots(_p(parent, I32P), int(members[0][-1]), int(members[1][-1]))
    shim.mcs_flatten(_p(parent, I32P), V)
    joined = np.where((want == r0) | (want == r1), min(r0, r1), want)
    assert np.array_equal(parent, joined) and shim.mcs_invariant(_p(parent, I32P), V) == 0


def test_the_restatement_against_scipy():
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name, (V, f) in LABEL_CASES.items():
        ok = f[K.valid_faces(V, f)].astype(np.int64)
        rows, cols = np.concatenate((ok[:, 0], ok[:, 1])), np.concatenate((ok[:, 1], ok[:, 2]))
        n, comp = connected_components(sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
        want = K.labels(V, f)[0]
        assert len(np.unique(want)) == n, name
        pairs = np.unique(np.stack((comp, want), axis=1), axis=0)       # one label per scipy component and the reverse
        assert len(pairs) == n, name
        assert np.array_equal(K.labels_any(V, f), want), name


# ---------------------------------------------------------------------------------------------------------------- 2. statistics
def test_statistics_equal_the_restatement(shim):
    v, f = K.mix()
    v[5] = (-0.0, -1e-40, 1e-41)                                        # a -0 and two denormals take part in the boxes
    lab = K.labels(len(v), f)[0]
    want = K.stats(v, f, lab)
    nv, nf, q, lo, hi = shim_stats(shim, v, f, lab)
    assert np.array_equal(nv, want["num_vertices"]) and np.array_equal(nf, want["num_faces"]) and np.array_equal(q, want["area_quanta"])
    roots = want["is_root"]
    assert roots.sum() == 3000 + 50 + 1 and sorted(set(nv[roots])) == [3, 4, 1600] and sorted(set(nf[roots])) == [1, 4, 2 * 39 * 39]
    assert np.array_equal(unkey(lo)[roots], want["lo"][roots]) and np.array_equal(unkey(hi)[roots], want["hi"][roots])
    assert (lo[~roots] == 2 ** 31 - 1).all() and (hi[~roots] == -2 ** 31).all() and (nv[~roots] == 0).all() and (q[~roots] == 0).all()
    # the quantised sum against the double sum: half a quantum per face
    a = R.areas(v, f)
    double = np.zeros(len(v))
    np.add.at(double, lab[f[:, 0]], a)
    err = np.abs(q * 2.0 ** -40 - double)
    print(f"largest |quantised - double| area {err.max():.3e} m^2 over components of up to {nf.max()} faces (bound {nf.max() * 2.0 ** -41:.3e})")
    assert (err[roots] <= nf[roots] * 2.0 ** -41 + 1e-15 * double[roots]).all()          # (+ the double sum's own rounding)
    assert shim.mcs_area_quanta(float("inf")) == shim.mcs_area_bad() == 1 << 62 and shim.mcs_area_quanta(2.0 ** 22) == 1 << 62
    assert shim.mcs_area_quanta(1.5 * 2.0 ** -40) == 2 and shim.mcs_area_quanta(2.5 * 2.0 ** -40) == 2          # rint: ties to even
    assert shim.mcs_area_quanta(5000.0 + 2.0 ** -40) == 5000 * 2 ** 40 + 1


def test_the_float_key_is_monotone_and_its_own_inverse(shim):
    tiny = np.float32(1e-45)
    values = np.array([-np.inf, -3.4028235e38, -1e20, -1.0, -1.1754944e-38, -1e-40, -tiny, 0.0, tiny, 1e-40, 1.1754944e-38, 1e-3, 1.0, 1.0000001,
                       1e20, 3.4028235e38, np.inf], dtype=np.float32)
    assert (np.diff(values) > 0).all() and values[6] < 0 < values[8]    # (the denormals are not flushed)
    keys = np.array([shim.mcs_float_key(float(x)) for x in values], dtype=np.int64)
    assert (np.diff(keys) > 0).all()
    for x, k in zip(values, keys):
        assert np.float32(shim.mcs_key_float(int(k))).tobytes() == np.float32(x).tobytes()
    assert shim.mcs_float_key(-0.0) == shim.mcs_float_key(0.0) == 0
    rng = np.random.default_rng(5)
    bits = rng.integers(-2 ** 31, 2 ** 31, size=4000).astype(np.int32)
    x = bits.view(np.float32)
    x = x[np.isfinite(x)]
    k = np.array([shim.mcs_float_key(float(t)) for t in x], dtype=np.int64)
    order = np.argsort(x, kind="stable")
    assert (np.diff(k[order]) >= 0).all() and np.array_equal(unkey(k.astype(np.int32)), np.where(x == 0, np.float32(0), x))
    assert -2 ** 31 < keys.min() and keys.max() < 2 ** 31 - 1           # (the starting values of hi / lo lie outside every finite key)


# ---------------------------------------------------------------------------------------------------------------- 3. sanitizers
def test_header_under_address_and_ub_sanitizers(tmp_path):
    """The shim's host functions as a stand-alone program (its own main) built with -fsanitize=address,undefined: F = 0 and V = 0,
    repeated and out-of-range indices (INT32_MIN / INT32_MAX among them), labels that are not the call's own, vertices that are NaN,
    infinite, -0 and denormal, areas that are infinite or not numbers, one giant fan and links from stale candidates along one chain
    of 20 000.  Any sanitizer report or wrong answer is a non-zero exit.  The runtimes are linked statically; nothing loaded into
    python is involved."""
    exe = str(tmp_path / "meshclean_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DMESHCLEAN_SHIM_MAIN", "-o", exe,
                           os.path.join(os.path.dirname(__file__), "meshclean_math_shim.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout


# ---------------------------------------------------------------------------------------------------------------- 4. plumbing
def test_binding_and_header_name_the_entry_points():
    from splatam_amd import _capi
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "splat_hip.h")).read()
    L = _capi.lib()
    for name in ("splat_mesh_components", "splat_mesh_component_stats"):
        assert hasattr(L, name) and name in _capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert _capi.SPLAT_MESH_AREA_BITS == int(re.search(r"#define SPLAT_MESH_AREA_BITS (\d+)", header).group(1)) == 40
    assert _capi.SPLAT_MESH_AREA_BAD == load_shim().mcs_area_bad() and "#define SPLAT_MESH_AREA_BAD (1LL << 62)" in header
    assert L.splat_abi_version() == 17 and _capi.ABI_VERSION == 17 and "#define SPLAT_ABI_VERSION 17 " in header
    # refusals need no device: nothing is launched
    p = 1 << 12
    assert L.splat_mesh_components(p, -1, 4, p, None) == 1 and L.splat_mesh_components(p, 4, -1, p, None) == 1
    assert L.splat_mesh_components(None, 4, 4, p, None) == 1 and L.splat_mesh_components(p, 4, 4, None, None) == 1
    ok = [p, 4, p, 4, p, p, p, p, p, p, None]
    for k in (0, 2, 4, 5, 6, 7, 8, 9):
        args = list(ok)
        args[k] = None
        assert L.splat_mesh_component_stats(*args) == 1, k
    for k in (1, 3):
        args = list(ok)
        args[k] = -1
        assert L.splat_mesh_component_stats(*args) == 1, k
    # empty inputs succeed without a launch (there is no device here to launch on)
    assert L.splat_mesh_components(None, 0, 0, None, None) == 0
    assert L.splat_mesh_component_stats(None, 0, None, 0, None, None, None, None, None, None, None) == 0


def test_there_is_no_cpu_path():
    import torch
    from splatam_amd import mesh_clean as MC
    from splatam_amd import mesh_score as S
    v, f = K.cube()
    with pytest.raises(RuntimeError, match="no CPU path"):
        MC.clean_mesh((v, f, None), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        MC.label_components(8, torch.from_numpy(f))
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.score_with_views((v, f, None), (v, f, None), samples=100, clean=True, device="cpu")


def test_clean_off_leaves_signatures_and_keys():
    from splatam_amd import mesh as M
    from splatam_amd import mesh_clean as MC
    from splatam_amd import mesh_render as MR
    from splatam_amd import mesh_score as S
    from splatam_amd import run
    sig = inspect.signature(S.score_mesh).parameters
    assert [(k, p.default) for k, p in sig.items()][2:] == [("samples", 200_000), ("threshold", 0.05), ("seed", 0), ("transform", None),
                                                            ("device", "cuda:0"), ("cell", None), ("align", False)]
    views = inspect.signature(S.score_with_views).parameters
    assert views["clean"].default is None and views["align"].default is False and views["depth_l1_views"].default == 0
    ex = inspect.signature(M.extract_mesh).parameters
    assert ex["clean"].default is None and list(ex)[-1] == "clean" and ex["sparse"].default is False and ex["voxel_size"].default == 0.01
    assert [(k, p.default) for k, p in inspect.signature(MR.cull_mesh).parameters.items()][4:] == [
        ("occlusion", None), ("eps", 0.03), ("edge", 0), ("rule", "all"), ("chunk", 16), ("transform", None), ("near", MR.NEAR), ("device", "cuda:0")]
    assert inspect.signature(M.mesh_from_params).parameters["clean"].default is None
    assert [(k, p.default) for k, p in inspect.signature(MC.clean_mesh).parameters.items()][1:] == [
        ("min_vertices", 200), ("min_faces", 0), ("min_area", 0.0), ("min_extent", 0.0), ("keep_largest", None), ("transform", None),
        ("device", "cuda:0"), ("report", False)]
    assert "cleaning" not in S.KEYS and "alignment" not in S.KEYS
    score = dict.fromkeys(S.KEYS, 0.0)
    score["samples"] = 10
    assert S.format_score(score).startswith("Accuracy: ")
    found = dict(fitness=1.0, inlier_rmse=0.01, iterations=7, status=1, translation_cm=2.5, rotation_deg=3.0)
    report = dict(components=12, components_kept=1, faces=1000, faces_removed=40, area_m2=2.0, area_removed_m2=0.5)
    text = S.format_score(dict(score, alignment=found, cleaning=report))
    lines = text.split("\n")
    assert lines[0] == "Cleaning: kept 1 of 12 components, removed 40 of 1000 faces, 0.500000 m^2 (25.0000 % of the area)"
    assert lines[1].startswith("Alignment: ") and "\n".join(lines[2:]) == S.format_score(score)
    for off in (None, False):
        assert MC.clean_options(off) is None
    assert MC.clean_options(True) == {} and MC.clean_options(dict(min_vertices=5)) == {"min_vertices": 5}
    with pytest.raises(ValueError):
        MC.clean_options(dict(min_vertex=5))
    with pytest.raises(ValueError):
        MC.clean_options(3)
    assert inspect.signature(run.run).parameters["mesh"].default is False


def test_the_commands_refuse_cleaning_options_without_what_they_need(capsys):
    from splatam_amd import mesh, mesh_score, run
    with pytest.raises(SystemExit):
        run.main(["experiment.py", "--clean-mesh"])
    assert "--clean-mesh needs --mesh" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh_score.main(["rec.ply", "gt.ply", "--min-vertices", "5"])
    assert "--min-vertices needs --clean" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(["params.npz", "--out", "mesh.ply", "--keep-largest", "1"])
    assert "need --clean" in capsys.readouterr().err


def test_the_restatements_filter_on_a_small_mesh():
    """The tie rules of the filter itself, on the host: two components of equal face count, ``keep_largest=1`` keeps the lower label."""
    v, f = K.join([K.cube(), K.cube((3, 0, 0)), K.tetrahedron((6, 0, 0))])
    c = np.arange(len(v) * 3, dtype=np.float32).reshape(-1, 3)
    nv, nf, nc, rep = K.clean(v, f, c, min_vertices=5)
    assert len(nv) == 16 and len(nf) == 24 and rep["components"] == 3 and rep["components_kept"] == 2 and rep["faces_removed"] == 4
    assert np.array_equal(nc, c[:16])
    nv, nf, nc, rep = K.clean(v, f, c, min_vertices=0, keep_largest=1)
    assert len(nv) == 8 and np.array_equal(nv, v[:8]) and np.array_equal(nf, f[:12]) and rep["components_kept"] == 1
    nv, nf, nc, rep = K.clean(v, f, c, min_vertices=9)
    assert len(nv) == 0 and len(nf) == 0 and rep["faces_removed"] == 28 and rep["area_removed_m2"] == rep["area_m2"] > 12.0
