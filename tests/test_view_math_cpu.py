"""The view layer without a GPU: splatam_amd/csrc/view_math.h compiled for the host (tests/view_math_shim.cpp: the camera arithmetic of
splat_view_camera and the loop body of splat_view_finish over every pixel) against the float64 numpy restatement tests/view_ref.py.

V1 (camera): every entry of w2c / viewmatrix / projmatrix / campos within ``view_ref.camera_bound`` = 4 * 2^-24 * (1 + |t|) of the
float64 ``setup_camera`` -- the header evaluates in double and rounds once, so it sits at half an ulp; torch's float32
``slam.setup_camera`` is held to the same bound on the same poses.
V2 (bytes): equal to the restatement wherever the float64 value before the rounding (c * 255) or truncation (n * 255) is farther than
1e-4 from a boundary, off by at most one nearer than that, at most 0.1 % of the elements that near (``view_ref.check_bytes``)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import view_ref
from tests.util import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 72, 40
FX, FY, CX, CY = 60.0, 58.0, 35.5, 19.25
NEAR_Z, FAR_Z = 0.01, 100.0

POSES = {
    "identity": view_ref.rigid((0, 1, 0), 0.0, (0.0, 0.0, 0.0)),
    "general": view_ref.rigid((0.3, 1.0, -0.2), 37.0, (0.4, -0.25, 1.5)),
    "far": view_ref.rigid((1.0, 0.2, 0.5), -112.0, (6.1, -5.3, 5.9)),            # |t| ~ 10
}
OFFSET = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.5], [0, 0, 0, 1]], dtype=np.float64)


@pytest.fixture(scope="module")
def shim():
    return host_shim("view_math_shim", "view_math.h")


def _p(a, t=C.c_float):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _camera_outputs():
    return {'w2c': np.full(16, np.nan, np.float32), 'viewmatrix': np.full(16, np.nan, np.float32),
            'projmatrix': np.full(16, np.nan, np.float32), 'campos': np.full(3, np.nan, np.float32)}


def _intr():
    return [C.c_double(v) for v in (FX, FY, CX, CY, NEAR_Z, FAR_Z)]


def shim_camera(shim, w2c, offset=None):
    o = _camera_outputs()
    shim.vm_camera_matrix(_p(np.ascontiguousarray(w2c, np.float32)), _p(offset, C.c_double), W, H, *_intr(),
                          _p(o['w2c']), _p(o['viewmatrix']), _p(o['projmatrix']), _p(o['campos']))
    return o


def torch_camera(_shim, w2c, offset=None):
    from splatam_amd import slam
    m = torch.from_numpy(np.ascontiguousarray(w2c, np.float32))
    if offset is not None:
        m = torch.from_numpy(offset.astype(np.float32)) @ m
    k = [[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]]
    cam = slam.setup_camera(W, H, k, m, near=NEAR_Z, far=FAR_Z, device="cpu")
    return {'w2c': m.reshape(-1).numpy(), 'viewmatrix': cam.viewmatrix.contiguous().reshape(-1).numpy(),
            'projmatrix': cam.projmatrix.contiguous().reshape(-1).numpy(), 'campos': cam.campos.numpy()}


def _assert_camera(got, want, bound, what):
    for k in ('w2c', 'viewmatrix', 'projmatrix', 'campos'):
        err = np.abs(got[k].astype(np.float64) - want[k]).max()
        print(f"{what} {k}: max |entry - float64| {err:.3e} (bound {bound:.3e})")
        assert np.isfinite(got[k]).all() and err <= bound, (what, k, err, bound)


@pytest.mark.parametrize("impl", ["view_math.h", "slam.setup_camera"])
@pytest.mark.parametrize("pose", sorted(POSES))
def test_camera_against_the_float64_setup_camera(shim, impl, pose):
    w2c = POSES[pose]
    want = view_ref.camera64(w2c, W, H, FX, FY, CX, CY, NEAR_Z, FAR_Z)
    got = (shim_camera if impl == "view_math.h" else torch_camera)(shim, w2c)
    _assert_camera(got, want, view_ref.camera_bound(np.linalg.norm(w2c[:3, 3].astype(np.float64))), f"{impl} {pose}")
    if impl == "view_math.h":
        assert np.array_equal(got['w2c'], w2c.reshape(-1)) and np.array_equal(got['viewmatrix'], w2c.T.reshape(-1))   # copies, bit for bit


@pytest.mark.parametrize("pose", sorted(POSES))
def test_camera_with_the_follow_offset(shim, pose):
    w2c = POSES[pose]
    want = view_ref.camera64(w2c, W, H, FX, FY, CX, CY, NEAR_Z, FAR_Z, offset=OFFSET)
    t_norm = np.linalg.norm(want['w2c'].reshape(4, 4)[:3, 3])
    _assert_camera(shim_camera(shim, w2c, OFFSET), want, view_ref.camera_bound(t_norm), f"offset {pose}")


def test_camera_from_a_pose_of_the_map(shim):
    """first_w2c . rel_w2c[t] from un-normalised quaternions: equal to the matrix form on the float64 product, to the bound."""
    rng = np.random.default_rng(5)
    n = 4
    rots = rng.normal(size=(1, 4, n)).astype(np.float32) * 1.7          # (not unit length: the arithmetic normalises)
    trans = rng.uniform(-2, 2, size=(1, 3, n)).astype(np.float32)
    first = POSES["general"]
    for t in range(n):
        M = first.astype(np.float64) @ view_ref.rel_w2c64(rots[0, :, t], trans[0, :, t])
        want = view_ref.camera64(M, W, H, FX, FY, CX, CY, NEAR_Z, FAR_Z, offset=OFFSET)
        o = _camera_outputs()
        shim.vm_camera_pose(_p(rots), _p(trans), n, t, _p(np.ascontiguousarray(first)), _p(OFFSET, C.c_double), W, H, *_intr(),
                            _p(o['w2c']), _p(o['viewmatrix']), _p(o['projmatrix']), _p(o['campos']))
        _assert_camera(o, want, view_ref.camera_bound(np.linalg.norm(want['w2c'].reshape(4, 4)[:3, 3])), f"map pose {t}")


# ---------------------------------------------------------------------------------------------------------------- V2
def shim_finish(shim, out6, mode, bg=(0.0, 0.0, 0.0), vmin=0.0, vmax=6.0, lut=None, w2c=None, cloud=False):
    h, w = out6.shape[1:]
    rgb8 = np.full((h, w, 3), 77, np.uint8)
    pts = np.full((h * w, 3), np.nan, np.float32) if cloud else None
    col = np.full((h * w, 3), np.nan, np.float32) if cloud else None
    shim.vm_finish(w, h, _p(np.ascontiguousarray(out6)), view_ref.MODES[mode], _p(np.asarray(bg, np.float32)), C.c_float(vmin), C.c_float(vmax),
                   _p(lut, C.c_uint8), C.c_float(FX), C.c_float(FY), C.c_float(CX), C.c_float(CY),
                   _p(None if w2c is None else np.ascontiguousarray(w2c, np.float32)), _p(rgb8, C.c_uint8), _p(pts), _p(col))
    return rgb8, pts, col


def _jet():
    from splatam_amd.view import jet_lut
    return np.ascontiguousarray(jet_lut())


@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.2, 0.5, 0.9)], ids=["black", "white", "tinted"])
@pytest.mark.parametrize("mode", ["color", "depth", "sil"])
def test_bytes_against_the_float64_restatement(shim, mode, bg):
    out6 = view_ref.seeded_planes(W, H, seed=11)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)           # row i = (i, i, i): the table row itself is visible
    for lut in ((grey, _jet()) if mode == "depth" else (None,)):
        rgb8, _, _ = shim_finish(shim, out6, mode, bg=bg, lut=lut)
        view_ref.check_bytes(rgb8, out6, mode, bg=bg, lut=lut, what="view_math.h")


def test_white_background_behind_an_empty_silhouette(shim):
    out6 = np.zeros((6, 3, 5), np.float32)
    rgb8, _, col = shim_finish(shim, out6, "color", bg=(1.0, 1.0, 1.0), w2c=np.eye(4), cloud=True)
    assert (rgb8 == 255).all() and (col == 1.0).all()
    rgb8, _, _ = shim_finish(shim, out6, "sil")
    assert (rgb8 == 255).all()


def test_nan_and_infinities_in_a_plane(shim):
    out6 = np.full((6, 2, 4), 0.4, np.float32)
    out6[3] = 0.5
    bad = [np.nan, np.inf, -np.inf, 0.25]
    for plane in (0, 3, 4):
        o = out6.copy()
        o[plane, 0, :] = bad
        for mode in ("color", "depth", "sil"):
            for bg in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
                rgb8, _, _ = shim_finish(shim, o, mode, bg=bg, lut=_jet())
                view_ref.check_bytes(rgb8, o, mode, bg=bg, lut=_jet(), what=f"plane {plane}")
    o = out6.copy()
    o[0, 0, :] = bad
    rgb8, _, _ = shim_finish(shim, o, "color")
    assert rgb8[0, :, 0].tolist() == [0, 255, 0, 64] and (rgb8[1] == 102).all()      # NaN -> 0; 0.25 * 255 = 63.75, 0.4 * 255 = 102
    o = out6.copy()
    o[3, 0, :] = bad
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    rgb8, _, _ = shim_finish(shim, o, "depth", lut=grey)
    assert rgb8[0, :, 0].tolist() == [0, 255, 0, 10]                                   # trunc(0.25 / 6 * 255) = 10


def test_equal_depth_bounds(shim):
    """vmin == vmax: the table's last row above it, its first row at or below it (0 / 0 is NaN, which the clip sends to 0)."""
    out6 = np.zeros((6, 1, 4), np.float32)
    out6[3, 0] = [1.0, 2.0, 3.0, np.nan]
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    rgb8, _, _ = shim_finish(shim, out6, "depth", vmin=2.0, vmax=2.0, lut=grey)
    assert rgb8[0, :, 0].tolist() == [0, 0, 255, 0]
    view_ref.check_bytes(rgb8, out6, "depth", vmin=2.0, vmax=2.0, lut=grey)


def test_cloud_against_the_float64_restatement(shim):
    """The host model of the cloud: within twice the deviation of the torch float32 form of rgbd2pcd on the same planes."""
    out6 = view_ref.seeded_planes(W, H, seed=3, depth_lo=0.2, depth_hi=6.0)
    for name in ("general", "far"):
        w2c = POSES[name]
        _, pts, col = shim_finish(shim, out6, "color", bg=(1.0, 1.0, 1.0), w2c=w2c, cloud=True)
        want_p, want_c = view_ref.cloud64(out6, w2c, FX, FY, CX, CY, bg=(1.0, 1.0, 1.0))
        torch_err = np.abs(view_ref.cloud_torch32(torch.from_numpy(out6), torch.from_numpy(w2c), FX, FY, CX, CY).numpy().astype(np.float64) - want_p).max()
        err = np.abs(pts.astype(np.float64) - want_p).max()
        print(f"cloud {name}: max |point - float64| {err:.3e}, torch float32 form {torch_err:.3e}")
        assert err <= 2.0 * torch_err
        assert np.abs(col.astype(np.float64) - want_c).max() <= 2.0 ** -23       # one fma and one subtraction at magnitude <= 2


def test_jet_table():
    lut = _jet()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert np.array_equal(lut, np.load(os.path.join(HERE, "golden", "jet_lut.npy")))
    try:
        import matplotlib
    except ImportError:
        return
    assert np.array_equal(lut, matplotlib.colormaps['jet'](np.arange(256), bytes=True)[:, :3])
