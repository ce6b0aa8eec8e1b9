// frameprep.hip -- ONE streaming resampling pass behind the three frame entries: a colour image colour[ch][cw][3] in 0..255 (float or
// byte) and a depth image depth[zh][zw] of a size of its own (possibly SMALLER than the output) -> colour and depth at dw x dh: what
// the reference's datasets do on the host with two cv2.resize calls and the loop with permute(2, 0, 1) / 255.  The arithmetic is
// frame_math.h's: colour is frame_blend of the four bilinear taps, depth the nearest source pixel.
//
//   frame_kernel<V, Colour, Z, PLANES>   one lane = V consecutive output x of one row (V = 4 when the width and the outputs' alignment
//       allow 16-byte stores, else 1): consecutive lanes take consecutive x, so the stores coalesce; the y taps and the nearest row are
//       the same for a whole wave but for the row breaks.  The sources are read element by element through __restrict__ const pointers:
//       neighbouring lanes read neighbouring or overlapping elements of at most two rows, which the vector cache serves from the lines
//       the first lane brought in (the image is read from memory once; nothing is staged).  No LDS, no atomics, plain stores.
//       Colour  float or uint8_t, read as (float)row[i].
//       Z       how a depth element becomes the 32 bits stored: uint16_t, a PNG's integer -> frame_depth_metres; uint32_t, the bits as
//               they are (a float32 moved as an integer, never through a floating-point operation: NaN payloads survive).
//       PLANES  true: the loop's planes im[3][dh][dw] in 0..1 -- the blend, then ONE division by 255 -- four 16-byte plane stores per
//               lane with V = 4; false: the dataset frame colour[dh][dw][3] in 0..255 -- a lane's V pixels are 3V consecutive floats,
//               with V = 4 three 16-byte stores (a wave writes 3 KiB without a gap).
//
//   P1 splat_frame_prepare         <float, uint32_t, planes>, the depth at the colour's size: a dataset frame -> the loop's planes.
//   P2 splat_frame_ingest          <uint8_t, uint16_t, interleaved>: a decoded image's bytes and a depth PNG's integers -> a dataset frame.
//   P3 splat_frame_ingest_planes   <uint8_t, uint16_t or uint32_t, planes>: P2's reads, P1's stores, the operations of P2 followed by P1
//                                  at equal size, so bit-equal to that pair without the interleaved frame (12 bytes per pixel written
//                                  and read again) in between.
#include "splat_device.h"
#include "frame_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint32_t depth_bits(uint16_t raw, double scale) { return __float_as_uint(frame_depth_metres(raw, scale)); }
__device__ __forceinline__ uint32_t depth_bits(uint32_t bits, double) { return bits; }

template <int V, typename Colour, typename Z, bool PLANES>
__global__ void __launch_bounds__(kBlock) frame_kernel(int cw, int ch, const Colour *__restrict__ colour, int zw, int zh,
                                                       const Z *__restrict__ depth_in, double depth_scale, int dw, int dh,
                                                       float *__restrict__ colour_out, uint32_t *__restrict__ depth_out) {
    const int per_row = dw / V;                                     // (V divides dw: the launcher's choice)
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)per_row * dh) return;
    const int y = (int)(i / per_row), x0 = (int)(i % per_row) * V;
    const FrameTap ty = frame_linear_tap(y, ch, dh);
    const Colour *row0 = colour + (size_t)ty.s0 * cw * 3, *row1 = colour + (size_t)ty.s1 * cw * 3;
    const Z *drow = depth_in + (size_t)frame_nearest_index(y, zh, dh) * zw;
    float c[3 * V];                                                 // pixel v's channel k at 3 * v + k
    uint32_t d[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const FrameTap tx = frame_linear_tap(x0 + v, cw, dw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v00 = (float)row0[3 * tx.s0 + k], v01 = (float)row0[3 * tx.s1 + k];
            const float v10 = (float)row1[3 * tx.s0 + k], v11 = (float)row1[3 * tx.s1 + k];
            c[3 * v + k] = PLANES ? frame_colour(v00, v01, v10, v11, tx.w, ty.w) : frame_blend(v00, v01, v10, v11, tx.w, ty.w);
        }
        d[v] = depth_bits(drow[frame_nearest_index(x0 + v, zw, dw)], depth_scale);
    }
    const size_t plane = (size_t)dw * dh, o = (size_t)y * dw + x0;
    if (V == 4) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (PLANES) *reinterpret_cast<float4 *>(colour_out + q * plane + o) = make_float4(c[q], c[3 + q], c[6 + q], c[9 + q]);
            else *reinterpret_cast<float4 *>(colour_out + 3 * o + 4 * q) = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
        *reinterpret_cast<uint4 *>(depth_out + o) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) colour_out[PLANES ? k * plane + o : 3 * o + k] = c[k];
        depth_out[o] = d[0];
    }
}

template <bool PLANES, typename Colour, typename Z>
hipError_t launch_frame(int cw, int ch, const Colour *colour, int zw, int zh, const Z *depth_in, double depth_scale, int dw, int dh,
                        float *colour_out, float *depth_out, hipStream_t s) {
    // 16-byte stores: a lane's 4 pixels start at float 4 * (...) of a plane or of the depth, or at float 12 * (...) of the interleaved
    // colour, so the width a multiple of 4 and both bases aligned put every store of every row on 16 bytes
    const bool vec = dw % 4 == 0 && (((uintptr_t)colour_out | (uintptr_t)depth_out) & 15) == 0;
    const long long items = (long long)(vec ? dw / 4 : dw) * dh;
    const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));
    hipLaunchKernelGGL((vec ? frame_kernel<4, Colour, Z, PLANES> : frame_kernel<1, Colour, Z, PLANES>), grid, dim3(kBlock), 0, s, cw, ch, colour,
                       zw, zh, depth_in, depth_scale, dw, dh, colour_out, reinterpret_cast<uint32_t *>(depth_out));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_frame_prepare(int sw, int sh, const float *color, const float *depth, int dw, int dh, float *im, float *depth_out,
                                hipStream_t s) {
    return launch_frame<true>(sw, sh, color, sw, sh, reinterpret_cast<const uint32_t *>(depth), 1.0, dw, dh, im, depth_out, s);
}

hipError_t launch_frame_ingest(int cw, int ch, const uint8_t *rgb, int zw, int zh, const uint16_t *depth_raw, double png_depth_scale,
                               int dw, int dh, float *color_out, float *depth_out, hipStream_t s) {
    return launch_frame<false>(cw, ch, rgb, zw, zh, depth_raw, png_depth_scale, dw, dh, color_out, depth_out, s);
}

hipError_t launch_frame_ingest_planes(int cw, int ch, const uint8_t *rgb, int zw, int zh, const void *depth_raw, bool depth_is_float,
                                      double depth_scale, int dw, int dh, float *im, float *depth_out, hipStream_t s) {
    if (depth_is_float) return launch_frame<true>(cw, ch, rgb, zw, zh, static_cast<const uint32_t *>(depth_raw), depth_scale, dw, dh, im, depth_out, s);
    return launch_frame<true>(cw, ch, rgb, zw, zh, static_cast<const uint16_t *>(depth_raw), depth_scale, dw, dh, im, depth_out, s);
}

}  // namespace splat
