"""splat_frame_prepare (csrc/frameprep.hip) through ``fused.prepare_frame`` against the float64 restatement tests/frame_ref.py: the
sizes and the three assertions of tests/test_frame_math_cpu.py, on a non-default stream, with outputs that are views into a larger
buffer whose guard elements on either side must stay as they were.  The guard lengths put the outputs on a 16-byte boundary in one
run and off it in the other, so every width meets the vector and the scalar store path where it can take both."""
import numpy as np
import pytest
import torch

import frame_ref

pytestmark = pytest.mark.gpu
COLOUR_ATOL = 1e-6          # 12 float32 roundings at magnitude <= 255: 12 * 2^-24 ~ 7e-7 on the [0, 1] image


def run_kernel(color, depth, h, w, lead):
    """``fused.prepare_frame`` into guarded views (frame_ref.run_guarded): (im [3, h, w], depth [1, h, w]) on the host."""
    from splatam_amd import fused
    return frame_ref.run_guarded(lambda c, z, out: fused.prepare_frame(c, z, size=(h, w), out=out), (color, depth), ((3, h, w), (1, h, w)), lead)


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("src,dst", frame_ref.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_against_the_float64_restatement(src, dst, lead):
    (sw, sh), (dw, dh) = src, dst
    color, depth = frame_ref.seeded_frame(sw, sh, seed=sw * 100 + dw, integer=False)
    want_im, want_d = frame_ref.prepare(color, depth, dh, dw)
    im, d = run_kernel(color, depth, dh, dw, lead)
    assert np.array_equal(d, want_d)
    err = np.abs(im.astype(np.float64) - want_im).max()
    print(f"{src} -> {dst} ({'aligned' if lead % 4 == 0 else 'unaligned'}): max |colour - float64| {err:.2e}")
    assert err <= COLOUR_ATOL


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("src,dst", frame_ref.EXACT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_colours_are_bit_equal_at_2_to_1_and_identity(src, dst, lead):
    (sw, sh), (dw, dh) = src, dst
    color, depth = frame_ref.seeded_frame(sw, sh, seed=7 + sw, integer=True)
    want = frame_ref.resize_linear(color, dh, dw).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    im, d = run_kernel(color, depth, dh, dw, lead)
    assert np.array_equal(im, want)
    assert np.array_equal(d, frame_ref.prepare(color, depth, dh, dw)[1])


def test_default_size_is_the_loops_layout_change_and_the_mirror_agrees():
    from splatam_amd import fused, slam
    color, depth = frame_ref.seeded_frame(37, 23, seed=3, integer=False)
    c, z = torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda()
    im, d = fused.prepare_frame(c, z)
    assert torch.equal(d, z.permute(2, 0, 1).contiguous())
    assert np.array_equal(im.cpu().numpy(), color.transpose(2, 0, 1) / np.float32(255))       # ONE correctly rounded float32 division
    # (torch's own `x / 255` on the device multiplies by the rounded reciprocal: it may differ from the division in the last bit)
    assert float((im - c.permute(2, 0, 1) / 255).abs().max()) <= 2.0 ** -23
    im, d = fused.prepare_frame(c, z, size=(11, 18))
    mim, md = slam.prepare_frame(c, z, size=(11, 18))
    assert torch.equal(d, md) and float((im - mim).abs().max()) <= 2 * COLOUR_ATOL        # (each within 1e-6 of the float64 form)


def test_bad_arguments_raise_before_any_launch():
    from splatam_amd import fused
    c, z = torch.zeros(6, 8, 3, device="cuda"), torch.zeros(6, 8, 1, device="cuda")
    with pytest.raises(RuntimeError):
        fused.prepare_frame(c.cpu(), z.cpu())
    with pytest.raises(RuntimeError):
        fused.prepare_frame(c, z[:5])
    with pytest.raises(RuntimeError):
        fused.prepare_frame(c, z, size=(0, 4))
    with pytest.raises(RuntimeError):
        fused.prepare_frame(c, z, size=(3, 4), out=(torch.zeros(3, 3, 5, device="cuda"), torch.zeros(1, 3, 4, device="cuda")))
