// lpips_math.h -- the index and per-pixel arithmetic of LPIPS (AlexNet taps), written once as host/device inline functions:
// lpips.hip calls them per lane, tests/test_lpips_cpu.py compiles the same header with g++ (tests/lpips_math_shim.cpp).
//
// The definition is restated from the public implementation (torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type='alex',
// normalize=True), i.e. the `lpips` package on torchvision's AlexNet `features`), AS RECALLED -- DESIGN.md 4 says what that means:
//   input     x in 0..1 (clamped)  ->  2x - 1  ->  (x - shift_c) / scale_c
//   taps      after each of the five ReLUs; a 3x3 stride-2 max-pool (no padding, floor) in front of conv2 and conv3
//   distance  per tap and pixel: u = f / (sqrt(sum_c f_c^2) + 1e-10) for both images, sum_c w_c (u0_c - u1_c)^2; mean over the
//             tap's pixels; the five means are added
#pragma once

#include <math.h>
#include <stddef.h>

#include "eval_math.h"

namespace splat {

constexpr int kLpipsLayers = 5;
constexpr int kLpipsMinSize = 31;        // the smallest extent for which every tap has an output
constexpr int kLpipsKStep = 32;          // K of one staged operand tile: every layer's packed K is a multiple of it (zero rows behind conv1's 363)
constexpr int kLpipsTile = 64;           // output pixels x output channels of one workgroup: 64 x 64
constexpr int kLpipsDistPixels = 64;     // pixels per workgroup of the distance kernel = pixels per double partial

struct LpipsLayer {
    int cin, cout, k, stride, pad, pool;     // pool != 0: a 3x3 stride-2 max-pool in front of the convolution
};
SPLAT_HD LpipsLayer lpips_layer(int l) {
    return l == 0 ? LpipsLayer{3, 64, 11, 4, 2, 0} : l == 1 ? LpipsLayer{64, 192, 5, 1, 2, 1} : l == 2 ? LpipsLayer{192, 384, 3, 1, 1, 1}
         : l == 3 ? LpipsLayer{384, 256, 3, 1, 1, 0} : LpipsLayer{256, 256, 3, 1, 1, 0};
}
SPLAT_HD int lpips_conv_out(int n, int k, int stride, int pad) { return n + 2 * pad < k ? 0 : (n + 2 * pad - k) / stride + 1; }
SPLAT_HD int lpips_pool_out(int n) { return n < 3 ? 0 : (n - 3) / 2 + 1; }
// along a dimension of n image pixels: the extent the convolution of layer l reads (behind its pool), and the extent of tap l
SPLAT_HD int lpips_layer_in(int n, int l) {
    for (int i = 0;; ++i) {
        const LpipsLayer L = lpips_layer(i);
        if (L.pool) n = lpips_pool_out(n);
        if (i == l) return n;
        n = lpips_conv_out(n, L.k, L.stride, L.pad);
    }
}
SPLAT_HD int lpips_tap_size(int n, int l) {
    const LpipsLayer L = lpips_layer(l);
    return lpips_conv_out(lpips_layer_in(n, l), L.k, L.stride, L.pad);
}
SPLAT_HD int lpips_layer_K(int l) { const LpipsLayer L = lpips_layer(l); return L.cin * L.k * L.k; }
SPLAT_HD int lpips_layer_Kpad(int l) { return (lpips_layer_K(l) + kLpipsKStep - 1) / kLpipsKStep * kLpipsKStep; }

// THE k order of the implicit GEMM: k = (c * KH + dy) * KH + dx, the order of a [Cout][Cin][KH][KH] weight's inner three indices
template <int KH>
SPLAT_HD void lpips_k_map(int k, int *c, int *dy, int *dx) {
    *c = k / (KH * KH);
    const int r = k - *c * (KH * KH);
    *dy = r / KH;
    *dx = r - *dy * KH;
}

// floats of the canonical weight buffer: per layer weight [Cout][Cin][KH][KH] then bias [Cout]; then lin0 .. lin4 ([Cout] each)
SPLAT_HD size_t lpips_weight_offset(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += (size_t)lpips_layer(i).cout * (lpips_layer_K(i) + 1);
    return o;
}
SPLAT_HD size_t lpips_bias_offset(int l) { return lpips_weight_offset(l) + (size_t)lpips_layer(l).cout * lpips_layer_K(l); }
SPLAT_HD size_t lpips_lin_offset(int l) {
    size_t o = lpips_weight_offset(kLpipsLayers);
    for (int i = 0; i < l; ++i) o += lpips_layer(i).cout;
    return o;
}
SPLAT_HD size_t lpips_weight_floats() { return lpips_lin_offset(kLpipsLayers); }
// floats of the PACKED network, the one buffer the kernels read: per layer the weights as [Kpad][Cout] (k-major: the row a k-step reads is
// contiguous over the channels; rows K .. Kpad - 1 zero), then the five biases, then the five lin vectors
SPLAT_HD size_t lpips_pack_offset(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += (size_t)lpips_layer_Kpad(i) * lpips_layer(i).cout;
    return o;
}
SPLAT_HD size_t lpips_pack_bias_offset(int l) {
    size_t o = lpips_pack_offset(kLpipsLayers);
    for (int i = 0; i < l; ++i) o += lpips_layer(i).cout;
    return o;
}
SPLAT_HD size_t lpips_pack_lin_offset(int l) {
    size_t o = lpips_pack_bias_offset(kLpipsLayers);
    for (int i = 0; i < l; ++i) o += lpips_layer(i).cout;
    return o;
}
SPLAT_HD size_t lpips_pack_floats() { return lpips_pack_lin_offset(kLpipsLayers); }

// double partials of the distance: one per kLpipsDistPixels pixels of a tap
SPLAT_HD int lpips_tap_rows(int W, int H, int l) {
    return (lpips_tap_size(W, l) * lpips_tap_size(H, l) + kLpipsDistPixels - 1) / kLpipsDistPixels;
}

// input stage: clamp to 0..1 (a NaN stays), 2x - 1, (x - shift) / scale with an IEEE division
SPLAT_HD float lpips_shift(int ch) { return ch == 0 ? -0.030f : ch == 1 ? -0.088f : -0.188f; }
SPLAT_HD float lpips_scale(int ch) { return ch == 0 ? 0.458f : ch == 1 ? 0.448f : 0.450f; }
SPLAT_HD float lpips_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
SPLAT_HD float lpips_input(float v, int ch) {
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return lpips_div((2.f * v - 1.f) - lpips_shift(ch), lpips_scale(ch));     // (2 v is exact: a contracted 2 v - 1 rounds as the plain one)
}
// ... of a pixel of eval(): weighted by the masks first (eval_math.h)
SPLAT_HD float lpips_input_masked(float v, int ch, float gt_depth, float sil, float sil_thres, bool sil_mask) {
    return lpips_input(eval_weighted(v, eval_masks(gt_depth, sil, sil_thres, sil_mask), sil_mask), ch);
}

}  // namespace splat
