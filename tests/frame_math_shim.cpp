// Host build of splatam_amd/csrc/frame_math.h for tests/test_frame_math_cpu.py and tests/test_ingest_math_cpu.py: the index rules one
// by one, the depth conversion over a whole array of raw values, and a plain-loop model of the resampling pass (frame_pass) that calls
// nothing but the header's functions, so that frame preparation and frame ingest are checked against the float64 restatement
// (tests/frame_ref.py) without a GPU.
#include "../splatam_amd/csrc/frame_math.h"

using namespace splat;

namespace {

float depth_value(uint16_t raw, double scale) { return frame_depth_metres(raw, scale); }
float depth_value(float metres, double) { return metres; }

// colour [ch][cw][3], depth_in [zh][zw] -> colour_out (PLANES: [3][dh][dw] in 0..1, else [dh][dw][3] in 0..255), depth_out [dh][dw]:
// the kernel's loop body over every destination pixel
template <bool PLANES, typename Colour, typename Z>
void frame_pass(int cw, int ch, const Colour *colour, int zw, int zh, const Z *depth_in, double scale, int dw, int dh, float *colour_out,
                float *depth_out) {
    for (int y = 0; y < dh; ++y) {
        const FrameTap ty = frame_linear_tap(y, ch, dh);
        const Colour *row0 = colour + (size_t)ty.s0 * cw * 3, *row1 = colour + (size_t)ty.s1 * cw * 3;
        const Z *drow = depth_in + (size_t)frame_nearest_index(y, zh, dh) * zw;
        for (int x = 0; x < dw; ++x) {
            const FrameTap tx = frame_linear_tap(x, cw, dw);
            for (int k = 0; k < 3; ++k) {
                const float v00 = (float)row0[3 * tx.s0 + k], v01 = (float)row0[3 * tx.s1 + k];
                const float v10 = (float)row1[3 * tx.s0 + k], v11 = (float)row1[3 * tx.s1 + k];
                if (PLANES) colour_out[((size_t)k * dh + y) * dw + x] = frame_colour(v00, v01, v10, v11, tx.w, ty.w);
                else colour_out[((size_t)y * dw + x) * 3 + k] = frame_blend(v00, v01, v10, v11, tx.w, ty.w);
            }
            depth_out[(size_t)y * dw + x] = depth_value(drow[frame_nearest_index(x, zw, dw)], scale);
        }
    }
}

}  // namespace

extern "C" {

void fm_linear_tap(int d, int src, int dst, int *s0, int *s1, float *w) {
    const FrameTap t = frame_linear_tap(d, src, dst);
    *s0 = t.s0; *s1 = t.s1; *w = t.w;
}
int fm_nearest_index(int d, int src, int dst) { return frame_nearest_index(d, src, dst); }

void im_depth_metres(int n, const uint16_t *raw, double scale, float *out) {
    for (int i = 0; i < n; ++i) out[i] = frame_depth_metres(raw[i], scale);
}

// splat_frame_prepare: color [sh][sw][3], depth [sh][sw] -> im [3][dh][dw], depth_out [dh][dw]
void fm_prepare(int sw, int sh, const float *color, const float *depth, int dw, int dh, float *im, float *depth_out) {
    frame_pass<true>(sw, sh, color, sw, sh, depth, 1.0, dw, dh, im, depth_out);
}

// splat_frame_ingest: rgb [ch][cw][3] bytes, depth_raw [zh][zw] -> color [dh][dw][3] in 0..255, depth [dh][dw]
void im_ingest(int cw, int ch, const uint8_t *rgb, int zw, int zh, const uint16_t *depth_raw, double scale, int dw, int dh, float *color,
               float *depth) {
    frame_pass<false>(cw, ch, rgb, zw, zh, depth_raw, scale, dw, dh, color, depth);
}

}
