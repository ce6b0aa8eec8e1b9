"""Frame preparation without a GPU: splatam_amd/csrc/frame_math.h compiled for the host (tests/frame_math_shim.cpp: the kernel's loop
body over every pixel) and the torch mirror ``slam.prepare_frame``, both against the float64 numpy restatement tests/frame_ref.py.

Depth is a copy: equal everywhere.  Colour: with integer-valued inputs at 2:1 and at identity every blend is exact in float32 (weights
0.5 / 0, sums of at most four integers over 4), so the result is bit-equal to float32(ref) / float32(255); elsewhere at most 12 float32
roundings at magnitude <= 255 lie between the float32 and the float64 evaluation, 12 * 2^-24 * 255 / 255 ~ 7e-7 on the [0, 1] image:
1e-6 absolute."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_ref
from tests.util import host_shim

COLOUR_ATOL = 1e-6


@pytest.fixture(scope="module")
def shim():
    return host_shim("frame_math_shim", "frame_math.h")


def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def shim_prepare(shim, color, depth, h, w):
    sh, sw = color.shape[:2]
    im, d = np.full((3, h, w), np.nan, np.float32), np.full((1, h, w), np.nan, np.float32)
    shim.fm_prepare(sw, sh, _p(np.ascontiguousarray(color)), _p(np.ascontiguousarray(depth)), w, h, _p(im), _p(d))
    return im, d


def mirror_prepare(_shim, color, depth, h, w):
    from splatam_amd import slam
    im, d = slam.prepare_frame(torch.from_numpy(color), torch.from_numpy(depth), size=(h, w))
    assert im.dtype == torch.float32 and im.is_contiguous() and tuple(im.shape) == (3, h, w) and tuple(d.shape) == (1, h, w)
    return im.numpy(), d.numpy()


IMPLEMENTATIONS = {"frame_math.h": shim_prepare, "slam.prepare_frame": mirror_prepare}


@pytest.mark.parametrize("impl", sorted(IMPLEMENTATIONS))
@pytest.mark.parametrize("src,dst", frame_ref.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_prepare_against_the_float64_restatement(shim, impl, src, dst):
    (sw, sh), (dw, dh) = src, dst
    color, depth = frame_ref.seeded_frame(sw, sh, seed=sw * 100 + dw, integer=False)
    want_im, want_d = frame_ref.prepare(color, depth, dh, dw)
    im, d = IMPLEMENTATIONS[impl](shim, color, depth, dh, dw)
    assert np.array_equal(d, want_d)
    err = np.abs(im.astype(np.float64) - want_im).max()
    print(f"{impl} {src} -> {dst}: max |colour - float64| {err:.2e}")
    assert err <= COLOUR_ATOL


@pytest.mark.parametrize("impl", sorted(IMPLEMENTATIONS))
@pytest.mark.parametrize("src,dst", frame_ref.EXACT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_colours_are_bit_equal_at_2_to_1_and_identity(shim, impl, src, dst):
    (sw, sh), (dw, dh) = src, dst
    color, depth = frame_ref.seeded_frame(sw, sh, seed=7 + sw, integer=True)
    ref = frame_ref.resize_linear(color, dh, dw).transpose(2, 0, 1)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)               # (the sums are exact in float32)
    want = ref.astype(np.float32) / np.float32(255)
    im, d = IMPLEMENTATIONS[impl](shim, color, depth, dh, dw)
    assert np.array_equal(im, want)
    assert np.array_equal(d, frame_ref.prepare(color, depth, dh, dw)[1])
    if src == dst:
        t = torch.from_numpy(color)
        assert np.array_equal(im, (t.permute(2, 0, 1) / 255).numpy())                    # the loop's own statement


@pytest.mark.parametrize("src,dst", [(s[0], d[0]) for s, d in frame_ref.SIZES] + [(s[1], d[1]) for s, d in frame_ref.SIZES])
def test_index_rules(shim, src, dst):
    s0w, s1w, ww = frame_ref.linear_taps(dst, src)
    nn = frame_ref.nearest_index(dst, src)
    for d in range(dst):
        s0, s1, w = C.c_int(), C.c_int(), C.c_float()
        shim.fm_linear_tap(d, src, dst, C.byref(s0), C.byref(s1), C.byref(w))
        assert (s0.value, s1.value) == (int(s0w[d]), int(s1w[d])) and 0 <= s0.value <= s1.value <= src - 1
        assert w.value == np.float32(ww[d])
        assert shim.fm_nearest_index(d, src, dst) == int(nn[d]) and 0 <= int(nn[d]) <= src - 1
    if src == 8 and dst == 13:                                                           # the upscale reaches both clamp branches
        assert ww[0] == 0.0 and s0w[0] == 0 and ww[-1] == 0.0 and s0w[-1] == src - 1
    if src == 39 and dst == 13:                                                          # 3:1: 1 / (13 / 39) is not 3.0 in double
        assert nn.tolist() == np.minimum(np.floor(np.arange(13) * (1.0 / (13.0 / 39.0))), 38).astype(int).tolist()


def test_scale_intrinsics_is_the_formula():
    from splatam_amd import slam
    k = torch.tensor([[600.0, 0, 599.5, 0], [0, 610.0, 339.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    for hr, wr in ((0.5, 0.5), (48 / 64, 72 / 96), (11 / 23, 18 / 37)):
        for m in (k, k[:3, :3]):
            got = slam.scale_intrinsics(m, hr, wr)
            want = m.clone()
            want[0, 0] *= wr
            want[0, 2] *= wr
            want[1, 1] *= hr
            want[1, 2] *= hr
            assert torch.equal(got, want) and got.dtype == torch.float32 and got is not m
            assert np.array_equal(got.numpy(), frame_ref.scale_intrinsics(m.numpy(), hr, wr))
    assert torch.equal(k, torch.tensor([[600.0, 0, 599.5, 0], [0, 610.0, 339.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))      # untouched
    with pytest.raises(ValueError):
        slam.scale_intrinsics(torch.eye(2), 1, 1)
