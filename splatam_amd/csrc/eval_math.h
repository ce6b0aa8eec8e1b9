// eval_math.h -- per-pixel and per-frame arithmetic of the evaluation metrics (PSNR, depth L1, MS-SSIM), written once as
// host/device inline functions: evalmetrics.hip calls them per lane, tests/test_eval_cpu.py compiles the very same header with
// g++ (tests/eval_math_shim.cpp) and checks it against the float64 torch form of the same definitions.
//
// Restates (in this project's words; nothing is copied):
//   the masks and sums of eval()          /root/reference/utils/eval_helpers.py:466-505
//   calc_psnr                             /root/reference/utils/slam_external.py:49-51
//   pytorch_msssim.ms_ssim (data_range 1, 11 taps, sigma 1.5, five levels) as splatam_amd/slam.py `ms_ssim` states it
#pragma once

#include <math.h>
#include <stddef.h>

#include "splat_math.h"

namespace splat {

constexpr int kEvalLevels = 5;
constexpr int kEvalTaps = 11;

// slots of one copy of SplatEvalWorkspace.sums (SPLAT_EVAL_SUMS doubles)
constexpr int kEvalSumSq = 0;        // [0..2] sum over ALL pixels of (weighted_im - weighted_gt)^2, per channel
constexpr int kEvalSumDepth = 3;     // sum of the masked |depth difference|
constexpr int kEvalSumValid = 4;     // number of pixels with ground-truth depth > 0
constexpr int kEvalSumHoles = 5;     // number of holes (eval_hole), with SplatEvalConfig.holes; otherwise 0
constexpr int kEvalSumLevels = 8;    // [8 + 6 level + 2 channel]: sum of cs, + 1: sum of ssim, over the level's (H - 10) x (W - 10) window positions
constexpr int kEvalSums = 40;
SPLAT_HD int eval_level_slot(int level, int ch) { return kEvalSumLevels + 6 * level + 2 * ch; }

// the five level weights of ms_ssim
SPLAT_HD double eval_level_weight(int level) {
    return level == 0 ? 0.0448 : level == 1 ? 0.2856 : level == 2 ? 0.3001 : level == 3 ? 0.2363 : 0.1333;
}

// normalised Gaussian window, exp(-(k - 5)^2 / (2 * 1.5^2)) / sum: formed in double, rounded once
inline void eval_window(float *g) {
    double e[kEvalTaps], s = 0.0;
    for (int k = 0; k < kEvalTaps; ++k) { e[k] = exp(-(double)((k - 5) * (k - 5)) / 4.5); s += e[k]; }
    for (int k = 0; k < kEvalTaps; ++k) g[k] = (float)(e[k] / s);
}

// avg_pool2d(kernel 2, stride 2, padding n % 2, count_include_pad) along one dimension of n pixels: the output has
// eval_pool_size(n) pixels, output p averages inputs eval_pool_first(p, n) and the one after it; index -1 is the zero pad
// (an odd n shifts the windows by one against the even case; the pad on the far side is never reached)
SPLAT_HD int eval_pool_size(int n) { return n / 2 + (n & 1); }
SPLAT_HD int eval_pool_first(int p, int n) { return 2 * p - (n & 1); }

// size of pyramid level `level` (0 = the frame) along a dimension of n pixels
SPLAT_HD int eval_level_size(int n, int level) {
    for (int l = 0; l < level; ++l) n = eval_pool_size(n);
    return n;
}

// floats of the pooled pyramid: X and Y, three channels each, levels 1..4
inline size_t eval_pyramid_floats(int W, int H) {
    size_t n = 0;
    for (int l = 1; l < kEvalLevels; ++l) n += 6 * (size_t)eval_level_size(W, l) * (size_t)eval_level_size(H, l);
    return n;
}

// One pixel of one channel as eval() weighs it.  valid = gt_depth > 0, presence = silhouette > sil_thres (both as 0 / 1 factors:
// a NaN in a rendered plane propagates exactly as `im * mask` propagates it in torch).
struct EvalPixel {
    float vf, pf;       // valid, presence (1 when the variant does not use the silhouette)
};
SPLAT_HD EvalPixel eval_masks(float gt_depth, float sil, float sil_thres, bool sil_mask) {
    EvalPixel m;
    m.vf = gt_depth > 0.f ? 1.f : 0.f;
    m.pf = sil_mask ? (sil > sil_thres ? 1.f : 0.f) : 1.f;
    return m;
}
// weighted_im / weighted_gt_im: im * presence * valid  (sil_mask)  or  im * valid
SPLAT_HD float eval_weighted(float v, const EvalPixel &m, bool sil_mask) { return sil_mask ? (v * m.pf) * m.vf : v * m.vf; }
// |(rastered_depth * valid - depth) [* presence]| * valid: the reference's "RMSE" term sqrt(d^2) and its L1 term |d| are this same number
SPLAT_HD float eval_depth_term(float rendered, float gt_depth, const EvalPixel &m, bool sil_mask) {
    const float d = rendered * m.vf - gt_depth;
    return fabsf(sil_mask ? d * m.pf : d) * m.vf;
}

// A hole of a novel view (eval_nvs(): ~(presence_sil_mask | ~valid_depth_mask)): the frame has depth here and the map does not
// cover the pixel.  A NaN silhouette compares false and is therefore a hole, as in torch; the rule does not depend on sil_mask.
SPLAT_HD bool eval_hole(float gt_depth, float sil, float sil_thres) { return gt_depth > 0.f && !(sil > sil_thres); }
// The frame counts towards the novel-view averages unless holes / (H * W) * 100 > 0.1, evaluated in float32 as torch evaluates
// the reference's expression (an integer tensor divided by a Python int is a float32 tensor).
SPLAT_HD bool eval_nvs_valid(long long holes, int W, int H) { return !((float)holes / (float)((long long)W * H) * 100.f > 0.1f); }

// One window position: mu1 = G*x, mu2 = G*y, e11 = G*(x x), e22 = G*(y y), e12 = G*(x y).  Returns ssim, *cs = the
// contrast-structure term.  IEEE divisions: sigma^2 = e - mu^2 cancels to ~1e-3 of its operands on flat regions, a 1-ulp
// reciprocal on top of that would show in the level means.
SPLAT_HD float eval_ssim_pixel(float mu1, float mu2, float e11, float e22, float e12, float *cs) {
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
    const float c = (2.f * s12 + kSsimC2) / (s1 + s2 + kSsimC2);
    *cs = c;
    return (2.f * mu12 + kSsimC1) / (mu1_sq + mu2_sq + kSsimC1) * c;
}

// The frame's numbers from the totals of the sums (tot: kEvalSums doubles), in double, in three steps so that a kernel can spread
// the eighteen transcendental calls over lanes: per channel the PSNR term, per (channel, level) the factor of the MS-SSIM product,
// then the row.  valid count 0 divides by zero and a NaN sum stays NaN, as the torch form gives them.
// 20 log10(1 / sqrt(mse)) of one channel; the mean runs over ALL W * H pixels
SPLAT_HD double eval_psnr_channel(const double *tot, int W, int H, int ch) {
    return 20.0 * log10(1.0 / sqrt(tot[kEvalSumSq + ch] / ((double)W * (double)H)));
}
// relu(mean cs) ^ weight for levels 0..3, relu(mean ssim) ^ weight for the last level
SPLAT_HD double eval_level_factor(const double *tot, int W, int H, int level, int ch) {
    const double cnt = (double)(eval_level_size(W, level) - 10) * (double)(eval_level_size(H, level) - 10);
    double v = tot[eval_level_slot(level, ch) + (level == kEvalLevels - 1 ? 1 : 0)] / cnt;
    v = v > 0.0 ? v : (v == v ? 0.0 : v);          // relu (a NaN stays)
    return pow(v, eval_level_weight(level));
}
// row: 8 doubles, [0] psnr, [1] depth_rmse, [2] depth_l1, [3] ms_ssim (NaN when off), [4] valid count; [5..7] are the caller's ([6]: the hole count, from the totals).
// psnr: [3] by channel; factor: [3][kEvalLevels] by channel, level (not read when ms_ssim is off)
SPLAT_HD void eval_row(const double *tot, const double *psnr, const double *factor, bool ms_ssim, double *row) {
    row[0] = (psnr[0] + psnr[1] + psnr[2]) / 3.0;
    row[1] = tot[kEvalSumDepth] / tot[kEvalSumValid];
    row[2] = row[1];
    row[4] = tot[kEvalSumValid];
    double ms = nan("");
    if (ms_ssim) {
        ms = 0.0;
        for (int ch = 0; ch < 3; ++ch) {
            double prod = 1.0;
            for (int l = 0; l < kEvalLevels; ++l) prod *= factor[ch * kEvalLevels + l];
            ms += prod;
        }
        ms /= 3.0;
    }
    row[3] = ms;
}
// W, H: the frame
SPLAT_HD void eval_finish(const double *tot, int W, int H, bool ms_ssim, double *row) {
    double psnr[3], factor[3 * kEvalLevels];
    for (int ch = 0; ch < 3; ++ch) {
        psnr[ch] = eval_psnr_channel(tot, W, H, ch);
        for (int l = 0; l < kEvalLevels; ++l) factor[ch * kEvalLevels + l] = ms_ssim ? eval_level_factor(tot, W, H, l, ch) : 0.0;
    }
    eval_row(tot, psnr, factor, ms_ssim, row);
}

}  // namespace splat
