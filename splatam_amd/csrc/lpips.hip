// lpips.hip -- LPIPS (AlexNet taps) of two images on the device; the index and per-pixel arithmetic is lpips_math.h's.  The two images
// are a batch of two through every kernel ([2][C][H][W] activations), so identical inputs give identical bits and a distance of 0.0.
//
//   L0 lpips_pack_kernel      once per network: a layer's [Cout][K] weights to [Kpad][Cout], rows K .. Kpad - 1 ZERO (conv1: 363 -> 384); the
//                             biases and lin vectors follow in the same buffer, the only one the other kernels read weights from.
//   L1 lpips_input_kernel     one lane per pixel: eval()'s masks (planes form), clamp, 2x - 1, shift / scale, both images -> [2][3][H][W].
//   L2 lpips_pool_kernel      3x3 stride-2 max-pool in front of conv2 and conv3, a kernel of its own (profiles/lpips.md says why).
//   L3 lpips_conv_kernel      ONE templated implicit GEMM on v_mfma_f32_32x32x2_f32 for the five layers.  M = output pixels of both
//                             images, N = output channels, K = Cin KH KH in lpips_k_map's order.  A workgroup (4 waves) owns a 64 pixel x
//                             64 channel tile, a wave a 32 x 32 quarter in one accumulator; a k-step stages 32 x 64 gathered input
//                             values and 32 x 64 weights through LDS (the next step's global loads are issued before this step's
//                             sixteen MFMAs).  The MFMA takes the WEIGHT tile as its row operand and the pixel tile as its column
//                             operand: a lane's sixteen results are sixteen channels of one pixel and a store instruction writes 32
//                             consecutive pixels of a channel plane.  BLOCKED SUMMATION in one fixed order: the sixteen MFMAs of a
//                             k-step are a k-ordered fmaf chain of 32 terms from zero, and the steps' sums are added in order of k (one
//                             float32 add per step).  One chain over all of K (3456 terms for conv4) measured 4.5 x the error of
//                             torch's float32 convolution on the CPU at the fourth tap; blocked it is as good (profiles/lpips.md).  No
//                             split of K over workgroups, no atomics: the same bits on every run.  Bias and ReLU in the epilogue.
//   L4 lpips_distance_kernel  per tap: 64 pixels x 4 channel quarters per workgroup; the channel norms of both images, then
//                             sum_c w_c (u0_c - u1_c)^2, float32 per pixel (quarters added in order); the 64 pixels go down wave 0 in
//                             double (__shfl_down: a fixed order): one double partial per workgroup.  No atomics.
//   L5 lpips_finish_kernel    one workgroup: per tap the partials in a fixed order, / (H_l W_l), the five added, one double stored.
#include "splat_device.h"
#include "lpips_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__global__ void __launch_bounds__(kBlock) lpips_pack_kernel(const float *w, int K, int Kpad, int Cout, float *packed) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= Kpad * Cout) return;
    const int k = i / Cout, n = i - k * Cout;
    packed[i] = k < K ? w[(size_t)n * K + k] : 0.f;
}

struct InputArgs {
    const float *im0, *im1, *sil, *gt_depth;     // gt_depth == NULL: two plain images
    float sil_thres;
    int sil_mask, HW;
    float *x;                                    // [2][3][HW]
};
__global__ void __launch_bounds__(kBlock) lpips_input_kernel(InputArgs a) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.HW) return;
    if (a.gt_depth) {
        const float d = a.gt_depth[i], sil = a.sil_mask ? a.sil[i] : 0.f;
        for (int ch = 0; ch < 3; ++ch) {
            a.x[(size_t)ch * a.HW + i] = lpips_input_masked(a.im0[(size_t)ch * a.HW + i], ch, d, sil, a.sil_thres, a.sil_mask != 0);
            a.x[(size_t)(3 + ch) * a.HW + i] = lpips_input_masked(a.im1[(size_t)ch * a.HW + i], ch, d, sil, a.sil_thres, a.sil_mask != 0);
        }
    } else {
        for (int ch = 0; ch < 3; ++ch) {
            a.x[(size_t)ch * a.HW + i] = lpips_input(a.im0[(size_t)ch * a.HW + i], ch);
            a.x[(size_t)(3 + ch) * a.HW + i] = lpips_input(a.im1[(size_t)ch * a.HW + i], ch);
        }
    }
}

// y [planes][Ho][Wo] = max over the 3x3 window at (2 oy, 2 ox) of x [planes][Hin][Win]; a NaN wins, as in torch
__global__ void __launch_bounds__(kBlock) lpips_pool_kernel(const float *x, int planes, int Hin, int Win, int Ho, int Wo, float *y) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)planes * Ho * Wo) return;
    const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
    const long long pl = i / ((long long)Wo * Ho);
    const float *p = x + (pl * Hin + 2 * oy) * Win + 2 * ox;
    float m = p[0];
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
            const float v = p[dy * Win + dx];
            m = (v > m || v != v) ? v : m;
        }
    y[i] = m;
}

struct ConvArgs {
    const float *x;          // [2][Cin][Hin][Win]
    const float *wt;         // [Kpad][Cout]
    const float *bias;       // [Cout]
    float *y;                // [2][Cout][Ho][Wo]
    int Cin, Hin, Win, Ho, Wo, Cout, K, Kpad, M;     // M = 2 Ho Wo
};

template <int KH, int S, int P>
__global__ void __launch_bounds__(kBlock) lpips_conv_kernel(ConvArgs a) {
    constexpr int kPer = kLpipsKStep * kLpipsTile / kBlock;          // staged values per lane and operand: 8
    static_assert(kLpipsTile == 64 && kBlock == 256 && kLpipsKStep % 4 == 0, "4 waves: 64 columns x 4 k rows per pass");
    __shared__ float s_x[kLpipsKStep][kLpipsTile];
    __shared__ float s_w[kLpipsKStep][kLpipsTile];
    const int col = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * kLpipsTile, n0 = blockIdx.y * kLpipsTile;
    const int HoWo = a.Ho * a.Wo;
    // the pixel this lane gathers for
    const int m = m0 + col;
    const bool m_ok = m < a.M;
    int img = 0, oy = 0, ox = 0;
    if (m_ok) {
        img = m / HoWo;
        const int p = m - img * HoWo;
        oy = p / a.Wo;
        ox = p - oy * a.Wo;
    }
    const int iy0 = oy * S - P, ix0 = ox * S - P;
    const float *xin = a.x + (size_t)img * a.Cin * a.Hin * a.Win;
    const float *wcol = a.wt + n0 + col;
    float rx[kPer], rw[kPer];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int k = k0 + wave + 4 * i;                            // (uniform over the wave)
            int c, dy, dx;
            lpips_k_map<KH>(k, &c, &dy, &dx);
            const int iy = iy0 + dy, ix = ix0 + dx;
            const bool ok = m_ok && k < a.K && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;      // padding and the rows behind K: zero
            rx[i] = ok ? xin[((size_t)c * a.Hin + iy) * a.Win + ix] : 0.f;
            rw[i] = wcol[(size_t)k * a.Cout];                           // (k < Kpad; the packed rows behind K are zero)
        }
    };
    const int lane = threadIdx.x & 63, l31 = lane & 31, khalf = lane >> 5;
    const int wp = wave & 1, wc = wave >> 1;                            // the wave's pixel half and channel half of the tile
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < a.Kpad; k0 += kLpipsKStep) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            s_x[wave + 4 * i][col] = rx[i];
            s_w[wave + 4 * i][col] = rw[i];
        }
        __syncthreads();
        if (k0 + kLpipsKStep < a.Kpad) fetch(k0 + kLpipsKStep);
        // 32x32x2: row operand lane l = A[i = l & 31][k = l >> 5] (channel i), column operand B[k = l >> 5][j = l & 31] (pixel j)
        f32x16 part;
#pragma unroll
        for (int r = 0; r < 16; ++r) part[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < kLpipsKStep / 2; ++kk)
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[2 * kk + khalf][wc * 32 + l31], s_x[2 * kk + khalf][wp * 32 + l31], part, 0, 0, 0);
        acc += part;                                                     // (the step's sum joins the total: blocked summation, fixed order)
        __syncthreads();
    }
    // D: column (pixel) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int mm = m0 + wp * 32 + l31;
    if (mm >= a.M) return;
    const int img2 = mm / HoWo, p2 = mm - img2 * HoWo;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = n0 + wc * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        const float v = acc[r] + a.bias[n];
        a.y[((size_t)img2 * a.Cout + n) * HoWo + p2] = v < 0.f ? 0.f : v;       // (a NaN stays)
    }
}

__global__ void __launch_bounds__(kBlock) lpips_distance_kernel(const float *f, const float *w, int C, int HW, double *partials) {
    static_assert(kLpipsDistPixels == 64, "one wave of pixels");
    __shared__ float s_a[4][kLpipsDistPixels], s_b[4][kLpipsDistPixels];
    const int px = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int pix = blockIdx.x * kLpipsDistPixels + px;
    const bool ok = pix < HW;
    const float *f0 = f + pix, *f1 = f + (size_t)C * HW + pix;
    float a0 = 0.f, a1 = 0.f;
    if (ok)
        for (int c = g; c < C; c += 4) {
            const float v0 = f0[(size_t)c * HW], v1 = f1[(size_t)c * HW];
            a0 = fmaf(v0, v0, a0);
            a1 = fmaf(v1, v1, a1);
        }
    s_a[g][px] = a0;
    s_b[g][px] = a1;
    __syncthreads();
    const float nrm0 = __fsqrt_rn(((s_a[0][px] + s_a[1][px]) + s_a[2][px]) + s_a[3][px]) + 1e-10f;
    const float nrm1 = __fsqrt_rn(((s_b[0][px] + s_b[1][px]) + s_b[2][px]) + s_b[3][px]) + 1e-10f;
    __syncthreads();
    float d = 0.f;
    if (ok)
        for (int c = g; c < C; c += 4) {
            const float diff = lpips_div(f0[(size_t)c * HW], nrm0) - lpips_div(f1[(size_t)c * HW], nrm1);
            d = fmaf(w[c], diff * diff, d);
        }
    s_a[g][px] = d;
    __syncthreads();
    if (g != 0) return;
    double v = ok ? (double)(((s_a[0][px] + s_a[1][px]) + s_a[2][px]) + s_a[3][px]) : 0.0;
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_down(v, h, 64);
    if (px == 0) partials[blockIdx.x] = v;
}

struct FinishArgs {
    int rows[kLpipsLayers];
    double count[kLpipsLayers];
};
__global__ void __launch_bounds__(kBlock) lpips_finish_kernel(const double *partials, FinishArgs a, double *out) {
    __shared__ double s_v[kBlock];
    double total = 0.0;
    for (int l = 0; l < kLpipsLayers; ++l) {
        double v = 0.0;
        for (int i = threadIdx.x; i < a.rows[l]; i += kBlock) v += partials[i];
        s_v[threadIdx.x] = v;
        __syncthreads();
        for (int h = kBlock / 2; h >= 1; h >>= 1) {
            if ((int)threadIdx.x < h) s_v[threadIdx.x] += s_v[threadIdx.x + h];
            __syncthreads();
        }
        total += s_v[0] / a.count[l];
        __syncthreads();
        partials += a.rows[l];
    }
    if (threadIdx.x == 0) *out = total;
}

unsigned blocks_for(long long n) { return splat::blocks_for(n, kBlock); }

}  // namespace

size_t lpips_partial_rows(int W, int H) {
    size_t n = 0;
    for (int l = 0; l < kLpipsLayers; ++l) n += (size_t)lpips_tap_rows(W, H, l);
    return n;
}

hipError_t launch_lpips_pack(const float *weights, float *net, hipStream_t s) {
    for (int l = 0; l < kLpipsLayers; ++l) {
        const LpipsLayer L = lpips_layer(l);
        const int K = lpips_layer_K(l), Kpad = lpips_layer_Kpad(l);
        hipLaunchKernelGGL(lpips_pack_kernel, dim3(blocks_for((long long)Kpad * L.cout)), dim3(kBlock), 0, s, weights + lpips_weight_offset(l), K,
                           Kpad, L.cout, net + lpips_pack_offset(l));
        // the bias and the lin vector as they are: a [Cout][1] "weight" with K = Kpad = 1 is a copy
        hipLaunchKernelGGL(lpips_pack_kernel, dim3(blocks_for(L.cout)), dim3(kBlock), 0, s, weights + lpips_bias_offset(l), 1, 1, L.cout,
                           net + lpips_pack_bias_offset(l));
        hipLaunchKernelGGL(lpips_pack_kernel, dim3(blocks_for(L.cout)), dim3(kBlock), 0, s, weights + lpips_lin_offset(l), 1, 1, L.cout,
                           net + lpips_pack_lin_offset(l));
    }
    return hipGetLastError();
}

// layer l's convolution + bias + ReLU of x [2][Cin][Hin][Win] into y [2][Cout][Ho][Wo]; net: the packed network
hipError_t launch_lpips_conv(int l, int Win, int Hin, const float *x, const float *net, float *y, hipStream_t s) {
    const LpipsLayer L = lpips_layer(l);
    ConvArgs a{};
    a.x = x; a.wt = net + lpips_pack_offset(l); a.bias = net + lpips_pack_bias_offset(l); a.y = y;
    a.Cin = L.cin; a.Hin = Hin; a.Win = Win;
    a.Ho = lpips_conv_out(Hin, L.k, L.stride, L.pad); a.Wo = lpips_conv_out(Win, L.k, L.stride, L.pad);
    a.Cout = L.cout; a.K = lpips_layer_K(l); a.Kpad = lpips_layer_Kpad(l);
    a.M = 2 * a.Ho * a.Wo;
    if (a.M <= 0 || L.cout % kLpipsTile != 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.M + kLpipsTile - 1) / kLpipsTile), (unsigned)(L.cout / kLpipsTile));
    if (l == 0) hipLaunchKernelGGL((lpips_conv_kernel<11, 4, 2>), grid, dim3(kBlock), 0, s, a);
    else if (l == 1) hipLaunchKernelGGL((lpips_conv_kernel<5, 1, 2>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((lpips_conv_kernel<3, 1, 1>), grid, dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// gt_depth == NULL: im0 / im1 are two plain images; otherwise im0 = the rendered colour, im1 = the frame's, weighted as eval() weighs them
hipError_t launch_lpips(int W, int H, const float *im0, const float *im1, const float *sil, const float *gt_depth, float sil_thres, int sil_mask,
                        const float *net, const SplatLpipsWorkspace &ws, double *out, hipStream_t s) {
    InputArgs in{im0, im1, sil, gt_depth, sil_thres, sil_mask, W * H, ws.input};
    hipLaunchKernelGGL(lpips_input_kernel, dim3(blocks_for((long long)W * H)), dim3(kBlock), 0, s, in);
    const float *x = ws.input;
    int w = W, h = H, pools = 0;
    FinishArgs fin{};
    double *partials = ws.partials;
    for (int l = 0; l < kLpipsLayers; ++l) {
        const LpipsLayer L = lpips_layer(l);
        if (L.pool) {
            const int ho = lpips_pool_out(h), wo = lpips_pool_out(w);
            float *y = ws.pooled[pools++];
            hipLaunchKernelGGL(lpips_pool_kernel, dim3(blocks_for(2LL * L.cin * ho * wo)), dim3(kBlock), 0, s, x, 2 * L.cin, h, w, ho, wo, y);
            x = y; w = wo; h = ho;
        }
        hipError_t e = launch_lpips_conv(l, w, h, x, net, ws.taps[l], s);
        if (e != hipSuccess) return e;
        w = lpips_conv_out(w, L.k, L.stride, L.pad);
        h = lpips_conv_out(h, L.k, L.stride, L.pad);
        x = ws.taps[l];
        fin.rows[l] = lpips_tap_rows(W, H, l);
        fin.count[l] = (double)w * (double)h;
        hipLaunchKernelGGL(lpips_distance_kernel, dim3((unsigned)fin.rows[l]), dim3(kBlock), 0, s, x, net + lpips_pack_lin_offset(l), L.cout, w * h,
                           partials);
        partials += fin.rows[l];
    }
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(kBlock), 0, s, ws.partials, fin, out);
    return hipGetLastError();
}

}  // namespace splat
