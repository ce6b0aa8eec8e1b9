// Host build of splatam_amd/csrc/frame_math.h for tests/test_frame_math_cpu.py: the index rules one by one, and a plain-loop model of
// the whole kernel (fm_prepare) that calls nothing but them, so that frame preparation is checked against the float64 restatement
// (tests/frame_ref.py) without a GPU.
#include "../splatam_amd/csrc/frame_math.h"

using namespace splat;

extern "C" {

void fm_linear_tap(int d, int src, int dst, int *s0, int *s1, float *w) {
    const FrameTap t = frame_linear_tap(d, src, dst);
    *s0 = t.s0; *s1 = t.s1; *w = t.w;
}
int fm_nearest_index(int d, int src, int dst) { return frame_nearest_index(d, src, dst); }

// color [sh][sw][3], depth [sh][sw] -> im [3][dh][dw], depth_out [dh][dw]: the kernel's loop body over every destination pixel
void fm_prepare(int sw, int sh, const float *color, const float *depth, int dw, int dh, float *im, float *depth_out) {
    for (int y = 0; y < dh; ++y) {
        const FrameTap ty = frame_linear_tap(y, sh, dh);
        const int ny = frame_nearest_index(y, sh, dh);
        const float *row0 = color + (size_t)ty.s0 * sw * 3, *row1 = color + (size_t)ty.s1 * sw * 3;
        for (int x = 0; x < dw; ++x) {
            const FrameTap tx = frame_linear_tap(x, sw, dw);
            for (int c = 0; c < 3; ++c)
                im[((size_t)c * dh + y) * dw + x] = frame_colour(row0[3 * tx.s0 + c], row0[3 * tx.s1 + c], row1[3 * tx.s0 + c], row1[3 * tx.s1 + c], tx.w, ty.w);
            depth_out[(size_t)y * dw + x] = depth[(size_t)ny * sw + frame_nearest_index(x, sw, dw)];
        }
    }
}

}
