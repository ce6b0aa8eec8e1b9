"""splat_frame_ingest_planes (csrc/frameprep.hip) through ``fused.ingest_planes``: a sensor's bytes and raw depth to the loop's planes in
one launch.  Held to

  * the float64 restatement tests/frame_ref.py on the bytes: colour within the 0..1 bound of tests/test_gpu_frame_prepare.py, counted
    the same way -- the bytes are exact in float32; three lerps of (subtract, multiply, add) and the three float32 weights are at most
    12 roundings at magnitude <= 255, i.e. 12 * 2^-24 on the 0..1 scale, and the one division adds 2^-24 at magnitude <= 1:
    13 * 2^-24 = 7.7e-7 <= 1e-6; ``float32(byte) / 255`` exactly at identity size;
  * the two kernels it stands for: bit-equal to ``fused.prepare_frame(*fused.ingest_frame(...))`` for uint16 depth in every case;
  * a float32 depth copied bit for bit (zeros, negatives, inf, a NaN with a payload of its own, denormals), a uint16 depth
    ``float32(float64(raw) / scale)`` for all 65 536 values.

Both outputs are views inside ONE guarded flat buffer at lead 64 (on a 16-byte boundary) and lead 61 (off it), as
tests/test_gpu_frame_ingest.py does it, so a width divisible by 4 takes the 16-byte and the scalar stores."""
import numpy as np
import pytest
import torch

import frame_ref

pytestmark = pytest.mark.gpu
COLOUR_ATOL = 1e-6
SCALES = (6553.5, 5000.0, 1000.0, 1234.567)
CASES = frame_ref.RAW_CASES     # ((colour w, h), (depth w, h), (destination w, h))


def run_kernel(rgb, raw, scale, h, w, lead):
    """``fused.ingest_planes`` into guarded views (frame_ref.run_guarded): (im [3, h, w], depth [h, w]) on the host."""
    from splatam_amd import fused
    im, depth = frame_ref.run_guarded(lambda c, z, out: fused.ingest_planes(c, z, scale, size=(h, w), out=out), (rgb, raw),
                                      ((3, h, w), (1, h, w)), lead)
    return im, depth[0]


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_kernel_against_the_float64_restatement_and_the_two_kernels_it_replaces(case, lead):
    from splatam_amd import fused
    (cw, ch), (zw, zh), (dw, dh) = case
    rgb, raw = frame_ref.seeded_raw(cw, ch, zw, zh, seed=cw * 100 + dw)
    im, depth = run_kernel(rgb, raw, 6553.5, dh, dw, lead)
    want_im, _ = frame_ref.prepare(rgb, raw, dh, dw) if (zw, zh) == (cw, ch) else frame_ref.prepare(rgb, np.zeros((ch, cw), np.uint16), dh, dw)
    err = np.abs(im.astype(np.float64) - want_im).max()
    path = "16-byte stores" if (dw % 4 == 0 and lead % 4 == 0) else "scalar stores"
    print(f"{case} ({path}): max |colour - float64| {err:.2e}")
    assert err <= COLOUR_ATOL
    assert np.array_equal(depth, (frame_ref.resize_nearest(raw, dh, dw).astype(np.float64) / 6553.5).astype(np.float32))
    if (cw, ch) == (dw, dh):
        assert np.array_equal(im, rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    # the pair of launches it stands for, bit for bit
    c, z = torch.from_numpy(rgb).cuda(), torch.from_numpy(raw).cuda()
    pair_im, pair_depth = fused.prepare_frame(*fused.ingest_frame(c, z, 6553.5, size=(dh, dw)))
    assert np.array_equal(im.view(np.uint32), pair_im.cpu().numpy().view(np.uint32))
    assert np.array_equal(depth.view(np.uint32), pair_depth.cpu().numpy().reshape(dh, dw).view(np.uint32))


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_float_depth_travels_bit_for_bit(case, lead):
    (cw, ch), (zw, zh), (dw, dh) = case
    rgb, _ = frame_ref.seeded_raw(cw, ch, zw, zh, seed=cw * 100 + dw)
    src = frame_ref.special_floats(zw, zh, seed=zw * 10 + dw)
    im, depth = run_kernel(rgb, src, None, dh, dw, lead)
    assert np.array_equal(depth.view(np.uint32), frame_ref.resize_nearest(src.view(np.uint32), dh, dw))
    err = np.abs(im.astype(np.float64) - frame_ref.prepare(rgb, np.zeros((ch, cw), np.uint16), dh, dw)[0]).max()
    print(f"{case} float32 depth: max |colour - float64| {err:.2e}")
    assert err <= COLOUR_ATOL


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
def test_every_special_float_survives_at_identity(lead):
    src = frame_ref.special_floats(8, 5, seed=1)
    want = src.view(np.uint32)
    assert {0x7FA12345, 0xFFC00001, 0x00000001, 0x7F800000, 0xBF800000} <= set(want.reshape(-1).tolist())
    _, depth = run_kernel(np.zeros((5, 8, 3), np.uint8), src, 1.0, 5, 8, lead)
    assert np.array_equal(depth.view(np.uint32), want)


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("scale", SCALES)
def test_depth_is_bit_equal_for_every_uint16(scale, lead):
    raw = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    assert raw[0, 0] == 0 and raw[-1, -1] == 65535
    rgb = np.zeros((256, 256, 3), np.uint8)
    for h, w in ((256, 256), (128, 128)):                               # identity, and 2:1 (every other value of every other row)
        _, depth = run_kernel(rgb, raw, scale, h, w, lead)
        want = (frame_ref.resize_nearest(raw, h, w).astype(np.float64) / np.float64(scale)).astype(np.float32)
        assert np.array_equal(depth.view(np.uint32), want.view(np.uint32))
        if (h, w) == (256, 256):
            assert depth[0, 0] == 0.0 and depth[-1, -1] == np.float32(65535.0 / scale)


def test_default_size_new_tensors_and_the_host_form_agree():
    from splatam_amd import datasets, fused
    rgb, raw = frame_ref.seeded_raw(37, 23, 16, 12, seed=3)
    src = frame_ref.special_floats(16, 12, seed=4)
    c = torch.from_numpy(rgb).cuda()
    im, depth = fused.ingest_planes(c, torch.from_numpy(src).cuda())
    assert tuple(im.shape) == (3, 23, 37) and tuple(depth.shape) == (1, 23, 37) and im.dtype == depth.dtype == torch.float32
    assert np.array_equal(im.cpu().numpy(), rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    for z, scale in ((raw, 5000.0), (raw.reshape(12, 16, 1), 5000.0), (src, None), (src, 1.0)):
        im, depth = fused.ingest_planes(c, torch.from_numpy(z).cuda(), scale, size=(11, 18))
        mim, md = datasets.ingest_planes_cpu(rgb, z, scale, size=(11, 18))
        assert tuple(mim.shape) == (3, 11, 18) and tuple(md.shape) == (1, 11, 18)
        assert np.array_equal(depth.cpu().numpy().view(np.uint32), md.numpy().view(np.uint32))
        assert float((im.cpu() - mim).abs().max()) <= 2 * COLOUR_ATOL      # (each within 1e-6 of the float64 form)


def test_bad_arguments_raise_before_any_launch():
    from splatam_amd import _capi, fused
    c = torch.zeros(6, 8, 3, dtype=torch.uint8, device="cuda")
    z = torch.from_numpy(np.zeros((6, 8), np.uint16)).cuda()
    f = torch.zeros(6, 8, device="cuda")
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c.cpu(), z.cpu(), 1000.0)                      # a CPU tensor
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, f.cpu())
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c.to(torch.float32), z, 1000.0)               # a float colour
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, torch.zeros(6, 8, dtype=torch.int32, device="cuda"), 1000.0)     # an int32 depth
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, f, 2)                                      # float32 depth is metres already
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, z)                                         # uint16 depth without its divisor
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, z, 0.0)
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, f, size=(0, 4))
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, f, size=(3, 4), out=(torch.zeros(3, 3, 5, device="cuda"), torch.zeros(1, 3, 4, device="cuda")))
    with pytest.raises(RuntimeError):
        fused.ingest_planes(c, f, size=(3, 4), out=(torch.zeros(3, 3, 4, device="cuda"), torch.zeros(3, 4, 1, device="cuda")))
    # ... and the C entry itself answers SPLAT_E_INVALID without launching
    L, p = _capi.lib(), c.data_ptr()
    o = torch.zeros(4 * 6 * 8, device="cuda").data_ptr()
    ok = (8, 6, p, 8, 6, f.data_ptr(), _capi.SPLAT_DEPTH_F32, 1.0, 8, 6, o, o, None)
    for at, value in ((6, 2), (7, 2.0), (7, 0.0), (0, 0), (8, 0), (2, None), (5, None), (10, None), (11, None)):
        args = list(ok)
        args[at] = value
        assert L.splat_frame_ingest_planes(*args) == 1, (at, value)          # SPLAT_E_INVALID
