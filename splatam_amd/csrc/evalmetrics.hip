// evalmetrics.hip -- the metrics a finished run is quoted by (PSNR, depth L1, MS-SSIM), from rendered planes and the frame,
// with nothing read back: per frame at most five level kernels + one finish kernel that writes a row of eight doubles.
//
//   Q1 eval_level_kernel<L0>   one pyramid level: 11x11 "valid" window statistics -> sums of cs and ssim per channel, the
//                              2x2-pooled X and Y of the next level; level 0 forms weighted_im / weighted_gt on the fly from the
//                              rendered planes, the frame and the two masks, and takes the PSNR and depth sums -- and, with
//                              SplatEvalConfig.holes, the count of valid-depth pixels the map does not cover
//   Q2 eval_finish_kernel      totals the copies of the sums, forms the row in double (eval_math.h: eval_finish), zeroes the sums
//
// The level kernel runs the window pass of window_sums.h on an UNPADDED window that starts at the tile's origin (a tile's 32 x 24 outputs
// read the 42 x 34 pixels below and right of it); a tile OWNS the 32 x 24 input pixels at its origin: it alone adds their PSNR / depth
// terms, in the load loop, and writes the 16 x 12 pooled pixels that start at half its origin.
#include "splat_device.h"
#include "eval_math.h"
#include "window_sums.h"

namespace splat {
namespace {

constexpr int kBlock = kWinBlock;
constexpr int kPooled = (kWinTW / 2) * (kWinTH / 2);
static_assert(kEvalTaps == kWinTaps && kPooled <= kBlock, "the window pass' taps; one trip over the pooled pixels");

struct LevelArgs {
    // level 0: the planes of the frame and of the render; levels 1..4: x, y = [3][H][W] of the pyramid
    const float *x, *y;             // rendered r, g, b / ground-truth im (level 0), pooled X / Y otherwise
    const float *depth, *sil, *gt_depth;    // level 0 only: [H][W] each
    float *px, *py;                 // [3][PH][PW] pooled planes of the next level (NULL at the last level)
    double *sums;                   // [SPLAT_ITER_SUM_COPIES][SPLAT_EVAL_SUMS]
    int W, H, PW, PH, level;
    float sil_thres;
    int sil_mask, holes;
    float win[kEvalTaps];
};

// (x, y) of channel `ch` at pixel offset `off` of the level; level 0 weighs the planes (eval_math.h) and returns the masks
template <bool L0>
__device__ __forceinline__ f2 level_pixel(const LevelArgs &a, const float *X, const float *Y, int off, EvalPixel &m) {
    f2 p = {X[off], Y[off]};
    if constexpr (L0) {
        m = eval_masks(a.gt_depth[off], a.sil_mask ? a.sil[off] : 0.f, a.sil_thres, a.sil_mask != 0);
        p.x = eval_weighted(p.x, m, a.sil_mask != 0);
        p.y = eval_weighted(p.y, m, a.sil_mask != 0);
    }
    return p;
}

// SSIM false: PSNR and depth sums alone (ms_ssim off; level 0 only)
template <bool L0, bool SSIM>
__global__ __launch_bounds__(kBlock) void eval_level_kernel(LevelArgs a) {
    __shared__ WindowLds<2> S;                      // vertical sums of (x, y), (x x, y y) and x y
    __shared__ double s_part[6 * (kBlock / 64)];
    float g[kWinTaps];
#pragma unroll
    for (int k = 0; k < kWinTaps; ++k) g[k] = a.win[k];
    int bx, by, ch;
    if (!xcd_tile(a.W, a.H, bx, by, ch)) return;
    const int W = a.W, H = a.H, tid = threadIdx.x;
    const int x0 = bx * kWinTW, y0 = by * kWinTH;
    const size_t HW = (size_t)H * W;
    const float *X = a.x + ch * HW, *Y = a.y + ch * HW;
    const bool sil_mask = a.sil_mask != 0;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // squared error, depth term, valid count (owned pixels); cs, ssim (owned window positions); holes (owned pixels)
    {   // vertical pass: thread = (window column, group of kWinTR output rows); the thread's first kWinTR rows of the tile's first kWinTW
        // columns are pixels the tile owns
        const int grp = tid / kWinCols, col = tid - grp * kWinCols;
        constexpr int rows = SSIM ? kWinRows : kWinTR;
        if (grp < kWinTG && (SSIM || col < kWinTW)) {
            const int xx = x0 + col;
            const bool cin = xx < W;
            const int xc = min(xx, W - 1);
            float vx[rows], vy[rows];
#pragma unroll
            for (int t = 0; t < rows; ++t) {
                const int yy = y0 + grp * kWinTR + t;
                const bool in = cin && yy < H;
                const int off = min(yy, H - 1) * W + xc;    // (a row or column outside the image: any address inside the plane, value discarded)
                EvalPixel m{};
                const f2 p = level_pixel<L0>(a, X, Y, off, m);
                vx[t] = in ? p.x : 0.f;
                vy[t] = in ? p.y : 0.f;
                if (L0 && t < kWinTR && col < kWinTW) {
                    const float d = p.x - p.y;
                    acc[0] += in ? d * d : 0.f;
                    if (ch == 0) {
                        const float term = eval_depth_term(a.depth[off], a.gt_depth[off], m, sil_mask);
                        acc[1] += in ? term : 0.f;
                        acc[2] += in ? m.vf : 0.f;
                        if (a.holes) acc[5] += in && eval_hole(a.gt_depth[off], a.sil[off], a.sil_thres) ? 1.f : 0.f;
                    }
                }
            }
            if constexpr (SSIM)
                window_vertical<2>(g, [&](int t, f2 (&p)[2], float &c) {
                    p[0] = f2{vx[t], vy[t]};
                    p[1] = p[0] * p[0];
                    c = p[0].x * p[0].y;
                }, S, grp, col);
        }
    }
    if constexpr (SSIM) {
        __syncthreads();
        if (tid < kWinItems) {                      // horizontal pass: 4 window positions
            const int hr = tid / (kWinTW / 4), hc = (tid & (kWinTW / 4 - 1)) * 4;
            f2 o[2][4];                             // (mu1, mu2), (E11, E22)
            float oC[4];                            // E12
            window_horizontal<2>(g, S, hr, hc, o, oC);
            const int yy = y0 + hr;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float cs;
                const float ss = eval_ssim_pixel(o[0][j].x, o[0][j].y, o[1][j].x, o[1][j].y, oC[j], &cs);
                const bool ok = yy + kEvalTaps - 1 < H && x0 + hc + j + kEvalTaps - 1 < W;      // the whole window lies inside the level
                acc[3] += ok ? cs : 0.f;
                acc[4] += ok ? ss : 0.f;
            }
        }
        if (a.px && tid < kPooled) {                // the next level's pixels that start at half this tile's origin
            const int px = x0 / 2 + (tid & (kWinTW / 2 - 1)), py = y0 / 2 + tid / (kWinTW / 2);
            if (px < a.PW && py < a.PH) {
                const int ix = eval_pool_first(px, W), iy = eval_pool_first(py, H);
                f2 s = (f2)(0.f);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sx = ix + (k & 1), sy = iy + (k >> 1);
                    const bool in = sx >= 0 && sy >= 0;                 // (-1: the zero pad of an odd dimension; the far side is never reached)
                    EvalPixel m{};
                    const f2 p = level_pixel<L0>(a, X, Y, min(max(sy, 0), H - 1) * W + min(max(sx, 0), W - 1), m);
                    s.x += in ? p.x : 0.f;
                    s.y += in ? p.y : 0.f;
                }
                const size_t o = ((size_t)ch * a.PH + py) * a.PW + px;
                a.px[o] = 0.25f * s.x;
                a.py[o] = 0.25f * s.y;
            }
        }
    }
    // the wave reduction runs in double: the PSNR / depth sums are compared at 1e-6
    double *const copy = sum_copy(a.sums, SPLAT_EVAL_SUMS);
    const int base = eval_level_slot(a.level, ch);
    if constexpr (L0) {
        block_sums_to<6, double>(copy, acc, s_part, [&](int k) { return k == 0 ? kEvalSumSq + ch : k == 1 ? kEvalSumDepth : k == 2 ? kEvalSumValid : k == 5 ? kEvalSumHoles : base + k - 3; });
    } else {
        const float v[2] = {acc[3], acc[4]};
        block_sums_to<2, double>(copy, v, s_part, [&](int k) { return base + k; });
    }
}

// one workgroup of four waves: lane = copy of the sums, wave w totals slots w, w + 4, ... (all of a wave's loads are in flight before
// its first shuffle: one memory round trip, not one per slot); the row's transcendental calls are spread over lanes (eval_math.h:
// eval_psnr_channel, eval_level_factor, eval_row)
constexpr int kFinishWaves = 4, kFinishPer = SPLAT_EVAL_SUMS / kFinishWaves;
__global__ __launch_bounds__(64 * kFinishWaves) void eval_finish_kernel(double *sums, int W, int H, int ms_ssim, const int32_t *status, double *row) {
    static_assert(SPLAT_ITER_SUM_COPIES == 64 && SPLAT_EVAL_SUMS % kFinishWaves == 0, "one copy per lane, whole slots per wave");
    __shared__ double s_tot[SPLAT_EVAL_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v[kFinishPer];
#pragma unroll
    for (int i = 0; i < kFinishPer; ++i) {
        double *p = sums + (size_t)lane * SPLAT_EVAL_SUMS + wave + kFinishWaves * i;
        v[i] = *p;
        *p = 0.0;                                   // consumed
    }
#pragma unroll
    for (int i = 0; i < kFinishPer; ++i) {
        double t = v[i];
        for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
        if (lane == 0) s_tot[wave + kFinishWaves * i] = t;
    }
    __syncthreads();
    // the frame's totals stay readable behind the copies (SplatEvalWorkspace.sums)
    if (threadIdx.x < SPLAT_EVAL_SUMS) sums[(size_t)SPLAT_ITER_SUM_COPIES * SPLAT_EVAL_SUMS + threadIdx.x] = s_tot[threadIdx.x];
    // (a double pow / log10 is a few hundred instructions: eighteen of them on one lane were 15 us of this kernel)
    __shared__ double s_psnr[3], s_factor[3 * kEvalLevels];
    if (wave == 0 && lane < 3 * kEvalLevels && ms_ssim) s_factor[lane] = eval_level_factor(s_tot, W, H, lane % kEvalLevels, lane / kEvalLevels);
    if (wave == 1 && lane < 3) s_psnr[lane] = eval_psnr_channel(s_tot, W, H, lane);
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[SPLAT_EVAL_ROW];
        eval_row(s_tot, s_psnr, s_factor, ms_ssim != 0, r);
        r[5] = status && (status[SPLAT_STATUS_OVERFLOW] != 0 || status[SPLAT_STATUS_STALE_HINT] != 0) ? 1.0 : 0.0;
        r[6] = s_tot[kEvalSumHoles];                // (0 without SplatEvalConfig.holes: nothing was added)
        r[7] = 0.0;
        for (int k = 0; k < SPLAT_EVAL_ROW; ++k) row[k] = r[k];
    }
}

}  // namespace

static_assert(SPLAT_EVAL_SUMS == kEvalSums && SPLAT_EVAL_LEVELS == kEvalLevels, "include/splat_hip.h and eval_math.h agree");

size_t eval_pyramid_bytes(int W, int H) { return sizeof(float) * eval_pyramid_floats(W, H); }

hipError_t launch_eval_metrics(int W, int H, const float *rgb, const float *depth, const float *sil, const float *gt_im,
                               const float *gt_depth, const SplatEvalConfig &cfg, const SplatEvalWorkspace &ews, const int32_t *status,
                               double *out_row, hipStream_t s) {
    LevelArgs a{};
    eval_window(a.win);
    a.x = rgb; a.y = gt_im; a.depth = depth; a.sil = sil; a.gt_depth = gt_depth;
    a.sums = ews.sums;
    a.sil_thres = cfg.sil_thres;
    a.sil_mask = cfg.sil_mask;
    a.holes = cfg.holes;
    a.W = W; a.H = H;
    if (!cfg.ms_ssim) {
        hipLaunchKernelGGL((eval_level_kernel<true, false>), xcd_tile_grid(W, H), dim3(kBlock), 0, s, a);
    } else {
        float *next = ews.pyramid;
        for (int l = 0; l < kEvalLevels; ++l) {
            a.level = l;
            const bool last = l == kEvalLevels - 1;
            a.PW = eval_pool_size(a.W); a.PH = eval_pool_size(a.H);
            const size_t plane3 = 3 * (size_t)a.PW * a.PH;
            a.px = last ? nullptr : next;
            a.py = last ? nullptr : next + plane3;
            if (l == 0) hipLaunchKernelGGL((eval_level_kernel<true, true>), xcd_tile_grid(a.W, a.H), dim3(kBlock), 0, s, a);
            else hipLaunchKernelGGL((eval_level_kernel<false, true>), xcd_tile_grid(a.W, a.H), dim3(kBlock), 0, s, a);
            a.x = a.px; a.y = a.py;
            a.W = a.PW; a.H = a.PH;
            next += 2 * plane3;
        }
    }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(64 * kFinishWaves), 0, s, ews.sums, W, H, cfg.ms_ssim, status, out_row);
    return hipGetLastError();
}

}  // namespace splat
