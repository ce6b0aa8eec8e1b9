// window_sums.h -- the separable 11-tap window pass of the SSIM kernels (device only): fused.hip F4 (ssim_forward_kernel) and F5
// (map_loss_backward_kernel), evalmetrics.hip Q1 (eval_level_kernel).
//
// VERTICAL pass first and without LDS: a thread owns one column of the window (lanes = consecutive columns: the loads coalesce), holds
// kWinTR + 10 input rows in registers and forms kWinTR output rows of vertical sums; only those go through LDS (24 rows x 42 columns, no
// halo rows), and the horizontal pass reads 14 columns for 4 output pixels of one thread: 10.5 LDS reads and 76 multiply-adds per pixel
// of five statistics, one barrier.  (Rounds 2-4 ran the passes the other way round -- window staged in LDS, horizontal pass over 26 halo
// rows for 16 output rows, 12 rows of five sums read back per two output pixels: 29 LDS reads and 87 multiply-adds per pixel, 26 KB,
// two barriers: F4 31.2 -> 25.0 us, F5 22.2 -> 21.0 us at 1200x680, profiles/r04_experiments.md 10.)  The statistics travel as NP float
// pairs + one float, so that the 11-tap sums are v_pk_fma_f32 (two statistics per instruction).
//
// A kernel keeps what is its own: how a thread obtains its 14 input rows (F4 / F5: the zero-padded window that starts 5 pixels above and
// left of the tile; Q1: the unpadded window that starts AT the tile) and what it does with the four finished outputs.
//
// The window VALUES are the callers' and deliberately differ: ssim_window_host (fused.hip) rounds per tap in float as create_window
// does, eval_window (eval_math.h) forms the window in double and rounds once as pytorch_msssim does -- each restates its own reference.
// So do the per-pixel formulas: ssim_pixel_dev (fused.hip) takes hardware reciprocals, eval_ssim_pixel (eval_math.h) IEEE divisions.
#pragma once

#include "splat_device.h"

namespace splat {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kWinBlock = 256;                          // threads of a workgroup
constexpr int kWinTaps = 11, kWinRadius = 5;
constexpr int kWinTW = 32, kWinTR = 4, kWinTG = 6;      // tile width; output rows per thread of the vertical pass; row groups per workgroup
constexpr int kWinTH = kWinTR * kWinTG;                 // tile height 24
constexpr int kWinCols = kWinTW + kWinTaps - 1;         // 42 window columns
constexpr int kWinRows = kWinTR + kWinTaps - 1;         // 14 input rows per thread
constexpr int kWinStride = 45;                          // LDS row stride in elements: 1 mod 4, the 64-bit reads of the horizontal pass fall on distinct banks
constexpr int kWinItems = kWinTH * (kWinTW / 4);        // horizontal work items: (row, group of 4 columns)
static_assert(kWinCols * kWinTG <= kWinBlock && kWinItems <= kWinBlock, "one trip per pass");

// blockIdx -> (tile column, tile row, channel).  Workgroups are dealt to the 8 XCDs round robin and each XCD has its own L2: with a plain
// 3-d grid the eight neighbours of a tile run on eight OTHER XCDs, and every halo pixel (the window is 1.9x the tile) comes from memory
// again (F5: 167 MB of traffic for 75 MB of planes).  Here XCD x owns a contiguous run of the (channel, row, column) order, so a tile's
// halo was read by the workgroup before it or one tile row earlier, through the SAME L2.
inline dim3 xcd_tile_grid(int W, int H) {
    const int tiles = 3 * ((W + kWinTW - 1) / kWinTW) * ((H + kWinTH - 1) / kWinTH);
    return dim3(8 * ((tiles + 7) / 8));
}

__device__ __forceinline__ bool xcd_tile(int W, int H, int &bx, int &by, int &ch) {
    const int ntx = (W + kWinTW - 1) / kWinTW, nty = (H + kWinTH - 1) / kWinTH, total = 3 * ntx * nty, per = (total + 7) / 8;
    const int b = blockIdx.x, slot = b >> 3, t = (b & 7) * per + slot;
    if (slot >= per || t >= total) return false;
    ch = t / (ntx * nty);
    const int r = t - ch * ntx * nty;
    by = r / ntx;
    bx = r - by * ntx;
    return true;
}

// vertical sums of NP pairs and one single statistic
template <int NP>
struct WindowLds {
    f2 a[NP][kWinTH][kWinStride];
    float c[kWinTH][kWinStride];
};

// Input t of a pass (a row of the vertical pass, a column of the horizontal one) into the 4 outputs it reaches: output j takes it with
// tap t - j, i.e. sums inputs j .. j + 10
template <int NP>
__device__ __forceinline__ void window_taps(const float (&g)[kWinTaps], int t, const f2 (&p)[NP], float c, f2 (&o)[NP][4], float (&oC)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tap = t - j;
        if (tap >= 0 && tap < kWinTaps) {
            const f2 w = (f2)(g[tap]);
#pragma unroll
            for (int n = 0; n < NP; ++n) o[n][j] = __builtin_elementwise_fma(w, p[n], o[n][j]);
            oC[j] = fmaf(g[tap], c, oC[j]);
        }
    }
}

template <int NP>
__device__ __forceinline__ void window_zero(f2 (&o)[NP][4], float (&oC)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int n = 0; n < NP; ++n) o[n][j] = (f2)(0.f);
        oC[j] = 0.f;
    }
}

// Thread (grp, col) of the vertical pass: row(t, p, c) yields the NP pairs and the single of its input row t (0 .. kWinRows - 1; the
// caller has every load in flight before this is entered); the kWinTR rows of sums go to LDS
template <int NP, typename Row>
__device__ __forceinline__ void window_vertical(const float (&g)[kWinTaps], Row row, WindowLds<NP> &S, int grp, int col) {
    static_assert(kWinTR == 4, "window_taps: 4 outputs per thread in either pass");
    f2 vA[NP][4];
    float vC[4];
    window_zero<NP>(vA, vC);
#pragma unroll
    for (int t = 0; t < kWinRows; ++t) {
        f2 p[NP];
        float c;
        row(t, p, c);
        window_taps<NP>(g, t, p, c, vA, vC);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int n = 0; n < NP; ++n) S.a[n][grp * kWinTR + j][col] = vA[n][j];
        S.c[grp * kWinTR + j][col] = vC[j];
    }
}

// Work item (hr, hc) of the horizontal pass, behind the barrier: 14 columns of vertical sums feed the 4 outputs at (hr, hc .. hc + 3)
template <int NP>
__device__ __forceinline__ void window_horizontal(const float (&g)[kWinTaps], const WindowLds<NP> &S, int hr, int hc, f2 (&o)[NP][4], float (&oC)[4]) {
    window_zero<NP>(o, oC);
#pragma unroll
    for (int t = 0; t < kWinRows; ++t) {
        f2 p[NP];
#pragma unroll
        for (int n = 0; n < NP; ++n) p[n] = S.a[n][hr][hc + t];
        const float c = S.c[hr][hc + t];
        window_taps<NP>(g, t, p, c, o, oC);
    }
}

}  // namespace splat
