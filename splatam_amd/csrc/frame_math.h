// frame_math.h -- index and blend arithmetic of frame preparation (a dataset frame color[H][W][3] in 0..255, depth[H][W][1] -> the
// loop's im[3][h][w] in 0..1, depth[1][h][w], at the same or at another size) and of frame ingest (a decoded image's bytes and a depth
// PNG's integers -> such a dataset frame), written once as host/device inline functions:
// frameprep.hip calls them per lane, tests/test_frame_math_cpu.py and tests/test_ingest_math_cpu.py compile the very same header with
// g++ (tests/frame_math_shim.cpp) and check it against the float64 numpy form of the same definitions
// (tests/frame_ref.py).
//
// Restates (in this project's words; nothing is copied) what the reference's datasets do to a frame on the host
// (/root/reference/datasets/gradslam_datasets/basedataset.py:210-257): colour through cv2.resize(INTER_LINEAR) on the 0..255 values,
// depth through cv2.resize(INTER_NEAREST), then the loop's permute(2, 0, 1) / 255.  The two index rules below are OpenCV's DOCUMENTED
// ones (pixel centres at half-integers for the linear taps; floor(d * (1 / (dst / src))) in double for the nearest source).  OpenCV is
// installed neither where this is developed nor where it is tested: the rules are a restatement and are NOT pinned against cv2 itself.
#pragma once

#include <math.h>
#include <stdint.h>

#include "splat_math.h"

namespace splat {

// The two source pixels and the weight of the second for destination index d along one axis:
// f = (d + 0.5) * (src / dst) - 0.5, s = floor(f), w = f - s; s < 0 -> s = 0, w = 0; s >= src - 1 -> s = src - 1, w = 0.
// (f in double: at f ~ 40 a float32 f would carry 2.4e-6 into the weight.)  s1 never leaves the row: with w = 0 it equals s0.
struct FrameTap {
    int s0, s1;
    float w;
};
SPLAT_HD FrameTap frame_linear_tap(int d, int src, int dst) {
    const double f = ((double)d + 0.5) * ((double)src / (double)dst) - 0.5;
    const double fl = floor(f);
    FrameTap t;
    int s = (int)fl;
    float w = (float)(f - fl);
    if (s < 0) { s = 0; w = 0.f; }
    if (s >= src - 1) { s = src - 1; w = 0.f; }
    t.s0 = s;
    t.s1 = s + 1 < src ? s + 1 : src - 1;
    t.w = w;
    return t;
}

// nearest source index: min(floor(d * (1 / (dst / src))), src - 1), every step in double (3:1 then rounds as OpenCV's does)
SPLAT_HD int frame_nearest_index(int d, int src, int dst) {
    const double inv = 1.0 / ((double)dst / (double)src);
    const int s = (int)floor((double)d * inv);
    return s < src - 1 ? s : src - 1;
}

SPLAT_HD float frame_lerp(float a, float b, float w) { return a + w * (b - a); }

// one channel of one destination pixel from its four source values (0..255), still in 0..255: along x on both rows, then along y.
// With both weights 0 (equal sizes) this is v00 itself.
SPLAT_HD float frame_blend(float v00, float v01, float v10, float v11, float wx, float wy) {
    const float top = frame_lerp(v00, v01, wx), bottom = frame_lerp(v10, v11, wx);
    return frame_lerp(top, bottom, wy);
}

// ... and as the loop's image in 0..1: the blend, then ONE division
SPLAT_HD float frame_colour(float v00, float v01, float v10, float v11, float wx, float wy) {
    return frame_blend(v00, v01, v10, v11, wx, wy) / 255.0f;
}

// Frame ingest (splat_frame_ingest): a depth PNG's integer as metres.  The reference's datasets divide the float64 image by
// png_depth_scale and narrow the quotient to float32 afterwards (basedataset.py:249-257, :336), so the division here is ONE division in
// double and ONE narrowing: bit-equal to that for every uint16 and every scale.  (A float32 division rounds once where this rounds
// twice; the two agree for many scales, 6553.5 / 5000 / 1000 among them, but not provably for all.)
SPLAT_HD float frame_depth_metres(uint16_t raw, double png_depth_scale) { return (float)((double)raw / png_depth_scale); }

}  // namespace splat
