"""Frame ingest without a GPU: splatam_amd/csrc/frame_math.h compiled for the host (tests/frame_math_shim.cpp) against the float64
restatement tests/frame_ref.py and against ``datasets.ingest_frame_cpu``, the torch form the loaders use on the CPU.

The reference's loaders cannot be executed here (cv2, imageio and natsort are absent), so the expected values are restated: depth is
what datasets/gradslam_datasets/basedataset.py:249-257, :336 compute, ``float32(float64(raw) / png_depth_scale)``, and must be equal
bit for bit for every uint16; colour is tests/frame_ref.py's float64 bilinear form on the byte values, within 255 * 1e-6 (at most 12
float32 roundings at magnitude <= 255, the bound of tests/test_frame_math_cpu.py on the 0..255 scale) and equal to the bytes at
equal size."""
import ctypes as C

import numpy as np
import pytest

import frame_ref
from tests.util import host_shim

SCALES = (6553.5, 5000.0, 1000.0, 1234.567)
COLOUR_ATOL = 255 * 1e-6
SIZES = frame_ref.SIZES + ((((26, 20), (16, 12)), (13, 9)),)         # ... and a depth image of a size of its own


@pytest.fixture(scope="module")
def shim():
    lib = host_shim("frame_math_shim", "frame_math.h")
    lib.im_depth_metres.argtypes = [C.c_int, C.c_void_p, C.c_double, C.c_void_p]
    lib.im_ingest.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("scale", SCALES)
def test_depth_conversion_is_bit_equal_for_every_uint16(shim, scale):
    raw = np.arange(65536, dtype=np.uint16)
    out = np.full(65536, np.nan, np.float32)
    shim.im_depth_metres(65536, raw.ctypes.data, scale, out.ctypes.data)
    want = (raw.astype(np.float64) / np.float64(scale)).astype(np.float32)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert out[0] == 0.0 and out[65535] == np.float32(65535.0 / scale)


def _sizes(case):
    src, dst = case
    return (src, src, dst) if isinstance(src[0], int) else (src[0], src[1], dst)


@pytest.mark.parametrize("impl", ("frame_math.h", "datasets.ingest_frame_cpu"))
@pytest.mark.parametrize("case", SIZES, ids=str)
def test_ingest_against_the_float64_restatement(shim, impl, case):
    (cw, ch), (zw, zh), (dw, dh) = _sizes(case)
    rgb, raw = frame_ref.seeded_raw(cw, ch, zw, zh, seed=cw * 100 + dw)
    scale = 6553.5
    if impl == "frame_math.h":
        color, depth = np.full((dh, dw, 3), np.nan, np.float32), np.full((dh, dw, 1), np.nan, np.float32)
        shim.im_ingest(cw, ch, rgb.ctypes.data, zw, zh, raw.ctypes.data, scale, dw, dh, color.ctypes.data, depth.ctypes.data)
    else:
        from splatam_amd import datasets
        color, depth = (t.numpy() for t in datasets.ingest_frame_cpu(rgb, raw, scale, size=(dh, dw)))
        assert color.dtype == np.float32 and depth.dtype == np.float32 and color.shape == (dh, dw, 3) and depth.shape == (dh, dw, 1)
    want_d = (frame_ref.resize_nearest(raw, dh, dw).astype(np.float64) / scale).astype(np.float32)
    assert np.array_equal(depth[..., 0], want_d)
    want_c = frame_ref.resize_linear(rgb, dh, dw)
    err = np.abs(color.astype(np.float64) - want_c).max()
    print(f"{impl} {case}: max |colour - float64| {err:.2e}")
    assert err <= COLOUR_ATOL
    if (cw, ch) == (dw, dh):
        assert np.array_equal(color, rgb.astype(np.float32))
