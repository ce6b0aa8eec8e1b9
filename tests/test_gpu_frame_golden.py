"""The three frame entry points (csrc/frameprep.hip) against the bits the kernels computed before they became one template:
tests/golden/frame_kernels_reference.npz, recorded on the device by tests/golden/make_golden_frame_kernels.py at the commit it names.
The kernels have no atomics and IEEE divisions, so every output is equal in every bit, with the outputs on a 16-byte boundary and off
it; one differing bit means that the order of operations changed."""
import os

import numpy as np
import pytest

import frame_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_kernels_reference.npz")


@pytest.mark.parametrize("lead", (64, 61), ids=("aligned", "unaligned"))
def test_every_output_bit_is_the_recorded_one(lead):
    from splatam_amd import fused
    want = np.load(GOLDEN)
    assert np.array_equal(want["sizes"], np.array(frame_ref.SIZES)) and np.array_equal(want["raw_cases"], np.array(frame_ref.RAW_CASES))
    assert float(want["scale"]) == frame_ref.GOLDEN_SCALE
    seen = set()
    for key, colour, depth in frame_ref.golden_frame_kernel_runs(fused, lead):
        assert np.array_equal(colour.view(np.uint32), want[key + "/colour"]), key
        assert np.array_equal(depth.view(np.uint32), want[key + "/depth"]), key
        seen |= {key + "/colour", key + "/depth"}
    assert seen == set(want.files) - {"commit", "scale", "seed_rule", "sizes", "raw_cases"} and len(seen) == 2 * (2 * 6 + 3 * 16)
