// Host build of splatam_amd/csrc/frame_math.h for tests/test_ingest_math_cpu.py: the depth conversion of frame ingest over a whole
// array of raw values, and a plain-loop model of the ingest kernel (im_ingest) that calls nothing but the header's functions.
#include "../splatam_amd/csrc/frame_math.h"

using namespace splat;

extern "C" {

void im_depth_metres(int n, const uint16_t *raw, double scale, float *out) {
    for (int i = 0; i < n; ++i) out[i] = frame_depth_metres(raw[i], scale);
}

// rgb [ch][cw][3] bytes, depth_raw [zh][zw] -> color [dh][dw][3] in 0..255, depth [dh][dw]: the kernel's loop body over every pixel
void im_ingest(int cw, int ch, const uint8_t *rgb, int zw, int zh, const uint16_t *depth_raw, double scale, int dw, int dh, float *color,
               float *depth) {
    for (int y = 0; y < dh; ++y) {
        const FrameTap ty = frame_linear_tap(y, ch, dh);
        const uint8_t *row0 = rgb + (size_t)ty.s0 * cw * 3, *row1 = rgb + (size_t)ty.s1 * cw * 3;
        const uint16_t *drow = depth_raw + (size_t)frame_nearest_index(y, zh, dh) * zw;
        for (int x = 0; x < dw; ++x) {
            const FrameTap tx = frame_linear_tap(x, cw, dw);
            for (int k = 0; k < 3; ++k)
                color[((size_t)y * dw + x) * 3 + k] = frame_blend((float)row0[3 * tx.s0 + k], (float)row0[3 * tx.s1 + k],
                                                                  (float)row1[3 * tx.s0 + k], (float)row1[3 * tx.s1 + k], tx.w, ty.w);
            depth[(size_t)y * dw + x] = frame_depth_metres(drow[frame_nearest_index(x, zw, dw)], scale);
        }
    }
}

}
