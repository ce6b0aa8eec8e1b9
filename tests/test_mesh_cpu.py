"""Plumbing of the mesh layer that needs no GPU: the PLY writer against a parser of its own, the default bounds and the ``max_bytes``
refusal of ``splatam_amd.mesh``, vertex keys at the last grid point of a volume at the size limit, the C ABI's new entry points and
struct mirrors (ABI 17 kept)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import tsdf_ref as R
from tests.util import host_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mesh_ply_round_trip(tmp_path):
    from splatam_amd.export import save_mesh_ply
    rng = np.random.default_rng(0)
    pos = rng.normal(size=(7, 3)).astype(np.float32)
    col = rng.uniform(size=(7, 3)).astype(np.float32)
    col[0], col[1] = (0.0, 1.0, 0.5), (-0.2, 1.3, np.nan)                # clamped; NaN -> 0
    faces = np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 0, 3]], dtype=np.int32)
    path = save_mesh_ply(str(tmp_path / "m.ply"), pos, faces, col)
    got_pos, got_col, got_faces = R.read_mesh_ply(path)
    assert got_pos.tobytes() == pos.tobytes() and np.array_equal(got_faces, faces)
    want = np.rint(np.clip(np.nan_to_num(col.astype(np.float64)), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(got_col, want) and got_col[0].tolist() == [0, 255, 128] and got_col[1].tolist() == [0, 255, 0]
    assert os.path.getsize(path) == open(path, "rb").read().index(b"end_header\n") + 11 + 7 * 15 + 4 * 13
    # no colours, no faces
    path = save_mesh_ply(str(tmp_path / "e.ply"), pos, np.zeros((0, 3), np.int32))
    got_pos, got_col, got_faces = R.read_mesh_ply(path)
    assert got_col is None and got_faces.shape == (0, 3) and got_pos.tobytes() == pos.tobytes()
    with pytest.raises(ValueError, match="do not exist"):
        save_mesh_ply(str(tmp_path / "bad.ply"), pos, np.array([[0, 1, 7]]))


def test_default_bounds_are_the_opaque_gaussians_box_padded():
    from splatam_amd import mesh
    means = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [-1.0, 0.5, 0.25], [50.0, 50.0, 50.0], [-40.0, 0.0, 0.0]])
    logits = torch.tensor([[2.0], [0.1], [5.0], [-0.1], [0.0]])         # the last two are not above 0.5
    lo, hi = mesh.default_bounds(means, logits, pad=0.05)
    assert lo == pytest.approx((-1.05, -0.05, -0.05)) and hi == pytest.approx((1.05, 2.05, 3.05))
    with pytest.raises(ValueError, match="no Gaussian"):
        mesh.default_bounds(means, torch.full((5, 1), -1.0), pad=0.05)
    origin, dims = mesh.plan_volume((lo, hi), 0.01)
    assert origin == lo and dims == (211, 211, 311)
    assert mesh.volume_bytes(dims) == 20 * 211 * 211 * 311
    # every point of the box is inside the grid: the last grid point is at or beyond the upper corner
    assert all(o + 0.01 * (d - 1) >= h - 1e-9 for o, d, h in zip(origin, dims, hi))


def test_a_volume_beyond_max_bytes_is_refused_with_its_size():
    from splatam_amd import mesh
    bounds = ((0.0, 0.0, 0.0), (10.0, 10.0, 3.0))
    need = 20 * 1001 * 1001 * 301                                        # 6.0 GB: inside the default 8 GiB
    assert need < mesh.DEFAULT_MAX_BYTES == 8 << 30 and mesh.plan_volume(bounds, 0.01)[1] == (1001, 1001, 301)
    with pytest.raises(ValueError) as e:
        mesh.plan_volume(bounds, 0.01, max_bytes=1 << 30)
    assert str(need) in str(e.value) and "1001 x 1001 x 301" in str(e.value) and "max_bytes" in str(e.value)
    assert mesh.plan_volume(bounds, 0.05, max_bytes=1 << 30)[1] == (201, 201, 61)
    with pytest.raises(ValueError):
        mesh.plan_volume(((0, 0, 0), (0, 1, 1)), 0.01)
    with pytest.raises(ValueError):
        mesh.plan_volume(bounds, 0.0)


def test_keys_at_the_last_grid_point_of_the_largest_volume():
    shim = host_shim("tsdf_math_shim", "tsdf_math.h")
    shim.tm_edge_key.restype = C.c_int64
    shim.tm_edge_key.argtypes = [C.c_int] * 8
    shim.tm_unlinear.argtypes = [C.c_int] * 3 + [C.c_int64, C.POINTER(C.c_int)]
    shim.tm_max_points.restype = C.c_int64
    from splatam_amd import mesh
    assert shim.tm_max_points() == mesh.MAX_POINTS == 1 << 40
    dims = (16384, 8192, 8191)                                           # 2^40 - 2^27 grid points: far past 2^31, inside the limit
    assert dims[0] * dims[1] * dims[2] < mesh.MAX_POINTS
    cell = (dims[0] - 2, dims[1] - 2, dims[2] - 2)
    for ca, cb in ((0, 7), (6, 7), (3, 7), (0, 1), (5, 7)):
        key = shim.tm_edge_key(*dims, *cell, ca, cb)
        assert key == R.edge_key(dims, cell, ca, cb) and key > 0
        a, b = R.decode_key(dims, key)
        ijk = (C.c_int * 3)()
        shim.tm_unlinear(*dims, key >> 3, ijk)
        assert list(ijk) == a.tolist() == [c + o for c, o in zip(cell, R.corner_offset(ca))]
        assert b.tolist() == [c + o for c, o in zip(cell, R.corner_offset(cb))]
    last = shim.tm_edge_key(*dims, *cell, 6, 7)                          # from (nx-2, ny-1, nz-1) along x to the last grid point
    assert last >> 3 == dims[0] * dims[1] * dims[2] - 2 and last & 7 == 1 and last < 1 << 43


def test_the_c_abi_has_the_mesh_layer_within_abi_17():
    from splatam_amd import _capi
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert L.splat_abi_version() == 17 == _capi.ABI_VERSION
    for name in ("splat_tsdf_bytes", "splat_tsdf_reset", "splat_tsdf_integrate", "splat_tsdf_triangles", "splat_tsdf_vertices"):
        assert hasattr(L, name) and name in _capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    for cls in (_capi.SplatTsdfVolume, _capi.SplatTsdfView):
        assert cls in _capi.MIRRORED_STRUCTS and L.splat_sizeof(cls.__name__.encode()) == C.sizeof(cls) > 0
        m = re.search(r"typedef struct " + cls.__name__ + r" \{(.*?)\} " + cls.__name__ + ";", header, flags=re.S)
        names = []
        for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
            decl = re.sub(r"\[[^\]]*\]", "", decl)
            if decl.strip():
                names += [re.findall(r"[A-Za-z_0-9]+", part)[-1] for part in decl.split(",")]
        assert [f[0] for f in cls._fields_] == names


def test_invalid_volumes_are_refused_without_a_launch():
    from splatam_amd import _capi
    L = _capi.lib()
    v = _capi.SplatTsdfVolume()
    assert L.splat_tsdf_bytes(None) == 0 and L.splat_tsdf_bytes(C.byref(v)) == 0
    v.nx, v.ny, v.nz, v.voxel, v.trunc = 8, 4, 2, 0.01, 0.04
    assert L.splat_tsdf_bytes(C.byref(v)) == 20 * 64
    assert L.splat_tsdf_reset(C.byref(v), None) == 1                     # NULL arrays
    v.tsdf = v.weight = v.r = v.g = v.b = 1 << 12
    count = C.c_int64(0)
    assert L.splat_tsdf_triangles(C.byref(v), 1.0, None, 4, None, None) == 1
    assert L.splat_tsdf_triangles(C.byref(v), 1.0, None, 4, C.addressof(count), None) == 1        # capacity without keys
    assert L.splat_tsdf_vertices(C.byref(v), None, 4, None, None, None) == 1
    w = _capi.SplatTsdfView()
    assert L.splat_tsdf_integrate(C.byref(v), C.byref(w), None) == 1 and L.splat_tsdf_integrate(C.byref(v), None, None) == 1
    w.width, w.height, w.out6, w.w2c, w.skip = 8, 8, 1 << 12, 1 << 12, 1 << 12
    assert L.splat_tsdf_integrate(C.byref(v), C.byref(w), None) == 1     # a skip flag without its counter
    for field, bad in (("nx", 0), ("nz", -3), ("voxel", 0.0), ("trunc", -1.0), ("voxel", float("nan"))):
        keep = getattr(v, field)
        setattr(v, field, bad)
        assert L.splat_tsdf_bytes(C.byref(v)) == 0 and L.splat_tsdf_reset(C.byref(v), None) == 1, field
        setattr(v, field, keep)
    v.nx, v.ny, v.nz = 1 << 14, 1 << 13, 1 << 13                         # 2^40 grid points
    assert L.splat_tsdf_bytes(C.byref(v)) == 0 and L.splat_tsdf_reset(C.byref(v), None) == 1
    v.nz = (1 << 13) - 1
    assert L.splat_tsdf_bytes(C.byref(v)) == 20 * (1 << 27) * ((1 << 13) - 1)


def test_mesh_module_refuses_the_cpu():
    from splatam_amd import mesh
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.TsdfVolume((0, 0, 0), (4, 4, 4), 0.1, device="cpu")
