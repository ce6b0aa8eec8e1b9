// frameprep.hip -- a frame as a dataset hands it over (color[H][W][3] in 0..255, depth[H][W][1]) -> the planes the loop works on
// (im[3][h][w] in 0..1, depth[1][h][w]) at the same or another size, in one streaming kernel: what the reference's datasets do on
// the host with two cv2.resize calls and the loop with permute(2, 0, 1) / 255.  The arithmetic is frame_math.h's.
//
//   P1 frame_prepare_kernel<V>   one lane = V consecutive output x of one row (V = 4 when the width and the planes' alignment allow
//                                16-byte stores, else 1): consecutive lanes take consecutive x, so the four plane stores coalesce;
//                                the y taps and the nearest row are the same for a whole wave but for the row breaks.
//                                No LDS, no atomics, plain stores.
//   P2 frame_ingest_kernel<V>    the step before P1: a decoded image's bytes rgb[H][W][3] and a depth PNG's integers depth[H'][W'] ->
//                                the dataset frame color[h][w][3] in 0..255, depth[h][w] in metres (splat_frame_ingest).  The same lane
//                                ownership; a lane's V pixels are 3V consecutive floats of the interleaved colour row, so with V = 4
//                                a lane stores 48 contiguous bytes as three 16-byte stores and a wave 3 KiB without a gap.  The source
//                                bytes are read one by one through __restrict__ const pointers: neighbouring lanes read neighbouring
//                                or overlapping bytes of at most two rows, which the vector cache serves from the lines the first
//                                lane brought in (the 2.4 MB image is read from memory once; nothing is staged).
//   P3 frame_ingest_planes_kernel<V, Z>   P2 and P1 in one pass (splat_frame_ingest_planes): the bytes and the raw depth (Z = uint16_t
//                                integers of a PNG, or float metres of a sensor) -> the loop's planes im[3][h][w] in 0..1, depth[h][w].
//                                P2's reads (byte by byte through __restrict__ const pointers, the depth image at a size of its own,
//                                possibly SMALLER than the output), P1's stores (four float4 plane stores per lane with V = 4).  The
//                                operations and their order are P2's followed by P1's at equal size -- frame_blend on the bytes, ONE
//                                division by 255 -- so the planes are bit-equal to that pair's, without the interleaved 0..255 frame
//                                (12 bytes per pixel written and read again) in between.  A float depth is copied as its 32 bits.
#include "splat_device.h"
#include "frame_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;

template <int V>
__global__ void __launch_bounds__(kBlock) frame_prepare_kernel(int sw, int sh, const float *__restrict__ color, const float *__restrict__ depth_in,
                                                               int dw, int dh, float *__restrict__ im, float *__restrict__ depth_out) {
    const int per_row = dw / V;                                     // (V divides dw: the launcher's choice)
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)per_row * dh) return;
    const int y = (int)(i / per_row), x0 = (int)(i % per_row) * V;
    const FrameTap ty = frame_linear_tap(y, sh, dh);
    const int ny = frame_nearest_index(y, sh, dh);
    const float *row0 = color + (size_t)ty.s0 * sw * 3, *row1 = color + (size_t)ty.s1 * sw * 3;
    const float *drow = depth_in + (size_t)ny * sw;
    float out[4][V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const FrameTap tx = frame_linear_tap(x0 + v, sw, dw);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[c][v] = frame_colour(row0[3 * tx.s0 + c], row0[3 * tx.s1 + c], row1[3 * tx.s0 + c], row1[3 * tx.s1 + c], tx.w, ty.w);
        out[3][v] = drow[frame_nearest_index(x0 + v, sw, dw)];
    }
    const size_t plane = (size_t)dw * dh, o = (size_t)y * dw + x0;
    if (V == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(im + c * plane + o) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
        *reinterpret_cast<float4 *>(depth_out + o) = make_float4(out[3][0], out[3][1], out[3][2], out[3][3]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) im[c * plane + o] = out[c][0];
        depth_out[o] = out[3][0];
    }
}

template <int V>
__global__ void __launch_bounds__(kBlock) frame_ingest_kernel(int cw, int ch, const uint8_t *__restrict__ rgb, int zw, int zh,
                                                              const uint16_t *__restrict__ depth_raw, double png_depth_scale,
                                                              int dw, int dh, float *__restrict__ color_out, float *__restrict__ depth_out) {
    const int per_row = dw / V;                                     // (V divides dw: the launcher's choice)
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)per_row * dh) return;
    const int y = (int)(i / per_row), x0 = (int)(i % per_row) * V;
    const FrameTap ty = frame_linear_tap(y, ch, dh);
    const uint8_t *row0 = rgb + (size_t)ty.s0 * cw * 3, *row1 = rgb + (size_t)ty.s1 * cw * 3;
    const uint16_t *drow = depth_raw + (size_t)frame_nearest_index(y, zh, dh) * zw;
    float c[3 * V], d[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const FrameTap tx = frame_linear_tap(x0 + v, cw, dw);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            c[3 * v + k] = frame_blend((float)row0[3 * tx.s0 + k], (float)row0[3 * tx.s1 + k], (float)row1[3 * tx.s0 + k],
                                       (float)row1[3 * tx.s1 + k], tx.w, ty.w);
        d[v] = frame_depth_metres(drow[frame_nearest_index(x0 + v, zw, dw)], png_depth_scale);
    }
    const size_t o = (size_t)y * dw + x0;
    if (V == 4) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            *reinterpret_cast<float4 *>(color_out + 3 * o + 4 * q) = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
        *reinterpret_cast<float4 *>(depth_out + o) = make_float4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) color_out[3 * o + k] = c[k];
        depth_out[o] = d[0];
    }
}

// the depth of one output pixel from its nearest source: a PNG's integer as metres, a float as the very bits it has (NaN payloads too:
// the value is moved as an integer, never through a floating-point operation)
__device__ __forceinline__ uint32_t planes_depth_bits(const uint16_t *__restrict__ row, int x, double scale) {
    return __float_as_uint(frame_depth_metres(row[x], scale));
}
__device__ __forceinline__ uint32_t planes_depth_bits(const uint32_t *__restrict__ row, int x, double) { return row[x]; }

template <int V, typename Z>
__global__ void __launch_bounds__(kBlock) frame_ingest_planes_kernel(int cw, int ch, const uint8_t *__restrict__ rgb, int zw, int zh,
                                                                     const Z *__restrict__ depth_raw, double depth_scale, int dw, int dh,
                                                                     float *__restrict__ im, uint32_t *__restrict__ depth_out) {
    const int per_row = dw / V;                                     // (V divides dw: the launcher's choice)
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)per_row * dh) return;
    const int y = (int)(i / per_row), x0 = (int)(i % per_row) * V;
    const FrameTap ty = frame_linear_tap(y, ch, dh);
    const uint8_t *row0 = rgb + (size_t)ty.s0 * cw * 3, *row1 = rgb + (size_t)ty.s1 * cw * 3;
    const Z *drow = depth_raw + (size_t)frame_nearest_index(y, zh, dh) * zw;
    float out[3][V];
    uint32_t d[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const FrameTap tx = frame_linear_tap(x0 + v, cw, dw);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[c][v] = frame_colour((float)row0[3 * tx.s0 + c], (float)row0[3 * tx.s1 + c], (float)row1[3 * tx.s0 + c],
                                     (float)row1[3 * tx.s1 + c], tx.w, ty.w);
        d[v] = planes_depth_bits(drow, frame_nearest_index(x0 + v, zw, dw), depth_scale);
    }
    const size_t plane = (size_t)dw * dh, o = (size_t)y * dw + x0;
    if (V == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(im + c * plane + o) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
        *reinterpret_cast<uint4 *>(depth_out + o) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) im[c * plane + o] = out[c][0];
        depth_out[o] = d[0];
    }
}

template <typename Z>
hipError_t launch_planes(int cw, int ch, const uint8_t *rgb, int zw, int zh, const Z *depth_raw, double depth_scale, int dw, int dh,
                         float *im, float *depth_out, hipStream_t s) {
    // 16-byte stores as in launch_frame_prepare: every plane's every row start on 16 bytes
    const bool vec = dw % 4 == 0 && (((uintptr_t)im | (uintptr_t)depth_out) & 15) == 0;
    const long long items = (long long)(vec ? dw / 4 : dw) * dh;
    const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));
    uint32_t *bits = reinterpret_cast<uint32_t *>(depth_out);
    if (vec) hipLaunchKernelGGL((frame_ingest_planes_kernel<4, Z>), grid, dim3(kBlock), 0, s, cw, ch, rgb, zw, zh, depth_raw, depth_scale, dw, dh, im, bits);
    else hipLaunchKernelGGL((frame_ingest_planes_kernel<1, Z>), grid, dim3(kBlock), 0, s, cw, ch, rgb, zw, zh, depth_raw, depth_scale, dw, dh, im, bits);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_frame_ingest_planes(int cw, int ch, const uint8_t *rgb, int zw, int zh, const void *depth_raw, bool depth_is_float,
                                      double depth_scale, int dw, int dh, float *im, float *depth_out, hipStream_t s) {
    if (depth_is_float) return launch_planes(cw, ch, rgb, zw, zh, static_cast<const uint32_t *>(depth_raw), depth_scale, dw, dh, im, depth_out, s);
    return launch_planes(cw, ch, rgb, zw, zh, static_cast<const uint16_t *>(depth_raw), depth_scale, dw, dh, im, depth_out, s);
}

hipError_t launch_frame_ingest(int cw, int ch, const uint8_t *rgb, int zw, int zh, const uint16_t *depth_raw, double png_depth_scale,
                               int dw, int dh, float *color_out, float *depth_out, hipStream_t s) {
    // 16-byte stores: a lane's 4 pixels start at float 12 * (...) of the colour and 4 * (...) of the depth, so, as in
    // launch_frame_prepare, the width a multiple of 4 and both bases aligned put every store on 16 bytes
    const bool vec = dw % 4 == 0 && (((uintptr_t)color_out | (uintptr_t)depth_out) & 15) == 0;
    const long long items = (long long)(vec ? dw / 4 : dw) * dh;
    const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));
    if (vec) hipLaunchKernelGGL(frame_ingest_kernel<4>, grid, dim3(kBlock), 0, s, cw, ch, rgb, zw, zh, depth_raw, png_depth_scale, dw, dh, color_out, depth_out);
    else hipLaunchKernelGGL(frame_ingest_kernel<1>, grid, dim3(kBlock), 0, s, cw, ch, rgb, zw, zh, depth_raw, png_depth_scale, dw, dh, color_out, depth_out);
    return hipGetLastError();
}

hipError_t launch_frame_prepare(int sw, int sh, const float *color, const float *depth, int dw, int dh, float *im, float *depth_out,
                                hipStream_t s) {
    // 16-byte stores need every plane's every row start on 16 bytes: the width a multiple of 4 and both bases aligned
    const bool vec = dw % 4 == 0 && (((uintptr_t)im | (uintptr_t)depth_out) & 15) == 0;
    const long long items = (long long)(vec ? dw / 4 : dw) * dh;
    const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));
    if (vec) hipLaunchKernelGGL(frame_prepare_kernel<4>, grid, dim3(kBlock), 0, s, sw, sh, color, depth, dw, dh, im, depth_out);
    else hipLaunchKernelGGL(frame_prepare_kernel<1>, grid, dim3(kBlock), 0, s, sw, sh, color, depth, dw, dh, im, depth_out);
    return hipGetLastError();
}

}  // namespace splat
