"""splat_frame_ingest (csrc/frameprep.hip) through ``fused.ingest_frame`` against the float64 restatement tests/frame_ref.py on the
raw integers.  The reference's loaders cannot be executed here (cv2, imageio and natsort are absent), so the expected values are
restated: colour is frame_ref.resize_linear of the bytes (within 255 * 1e-6: at most 12 float32 roundings at magnitude <= 255, the
bound of tests/test_gpu_frame_prepare.py on the 0..255 scale; the bytes themselves at identity size), depth is
``float32(float64(raw) / png_depth_scale)`` of frame_ref.resize_nearest, bit for bit (datasets/gradslam_datasets/basedataset.py
:249-257, :336).  Outputs are views into a larger buffer whose guard elements must stay as they were; the guard lengths put the
views on a 16-byte boundary in one run and off it in the other, so a width that is a multiple of 4 takes the 16-byte stores when
aligned and the scalar stores when not, and an odd width takes the scalar stores either way."""
import numpy as np
import pytest
import torch

import frame_ref

pytestmark = pytest.mark.gpu
COLOUR_ATOL = 255 * 1e-6
SCALES = (6553.5, 5000.0, 1000.0, 1234.567)
# ((colour w, h), (depth w, h), (destination w, h)): every frame_ref.SIZES pair, and a depth image of a size of its own
CASES = tuple((s, s, d) for s, d in frame_ref.SIZES) + (((26, 20), (16, 12), (13, 9)),)


def run_kernel(rgb, raw, scale, h, w, lead):
    """``fused.ingest_frame`` into guarded views (frame_ref.run_guarded): (colour [h, w, 3], depth [h, w]) on the host."""
    from splatam_amd import fused
    color, depth = frame_ref.run_guarded(lambda c, z, out: fused.ingest_frame(c, z, scale, size=(h, w), out=out), (rgb, raw),
                                         ((h, w, 3), (h, w, 1)), lead)
    return color, depth[..., 0]


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_kernel_against_the_float64_restatement(case, lead):
    (cw, ch), (zw, zh), (dw, dh) = case
    rgb, raw = frame_ref.seeded_raw(cw, ch, zw, zh, seed=cw * 100 + dw)
    color, depth = run_kernel(rgb, raw, 6553.5, dh, dw, lead)
    assert np.array_equal(depth, (frame_ref.resize_nearest(raw, dh, dw).astype(np.float64) / 6553.5).astype(np.float32))
    err = np.abs(color.astype(np.float64) - frame_ref.resize_linear(rgb, dh, dw)).max()
    path = "16-byte stores" if (dw % 4 == 0 and lead % 4 == 0) else "scalar stores"
    print(f"{case} ({path}): max |colour - float64| {err:.2e}")
    assert err <= COLOUR_ATOL
    if (cw, ch) == (dw, dh):
        assert np.array_equal(color, rgb.astype(np.float32))


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
    rgb, raw = frame_ref.seeded_raw(37, 23, 37, 23, seed=3)
    c, z = torch.from_numpy(rgb).cuda(), torch.from_numpy(raw).cuda()
    color, depth = fused.ingest_frame(c, z, 5000.0)
    assert tuple(color.shape) == (23, 37, 3) and tuple(depth.shape) == (23, 37, 1) and color.dtype == depth.dtype == torch.float32
    assert torch.equal(color, c.to(torch.float32))
    color, depth = fused.ingest_frame(c, z.view(23, 37, 1), 5000.0, size=(11, 18))
    mc, md = datasets.ingest_frame_cpu(rgb, raw, 5000.0, size=(11, 18))
    assert torch.equal(depth.cpu(), md)
    assert float((color.cpu() - mc).abs().max()) <= 2 * COLOUR_ATOL      # (each within 255e-6 of the float64 form)


def test_bad_arguments_raise_before_any_launch():
    from splatam_amd import fused
    c, z = torch.zeros(6, 8, 3, dtype=torch.uint8, device="cuda"), torch.from_numpy(np.zeros((6, 8), np.uint16)).cuda()
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c.cpu(), z.cpu(), 1000.0)
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c.to(torch.float32), z, 1000.0)                # wrong colour dtype
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c, torch.zeros(6, 8, dtype=torch.int32, device="cuda"), 1000.0)     # wrong depth dtype
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c, z.cpu(), 1000.0)
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c, z, 0.0)
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c, z, 1000.0, size=(0, 4))
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c, z, 1000.0, size=(3, 4), out=(torch.zeros(3, 5, 3, device="cuda"), torch.zeros(3, 4, 1, device="cuda")))
    with pytest.raises(RuntimeError):
        fused.ingest_frame(c, z, 1000.0, size=(3, 4), out=(torch.zeros(3, 4, 3, device="cuda"), torch.zeros(1, 3, 4, device="cuda")))
