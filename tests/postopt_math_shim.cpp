// Host build of the get_loss_gs arithmetic in splatam_amd/csrc/fused_math.h for tests/test_postopt_cpu.py: the functions one by one and
// a plain-loop model of a frame's depth term (pm_frame) that calls nothing but them, the way ssim_forward_kernel /
// map_loss_backward_kernel / pose_finish_kernel do in their GS form.  With POSTOPT_SHIM_MAIN it is a stand-alone program (its own
// main) that runs the model on a seeded frame and checks it against a second, independent loop: the build the test runs under
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../splatam_amd/csrc/fused_math.h"

using namespace splat;

extern "C" {

// per pixel: mask, |gt - depth| on the mask, d|.|/d(depth)
void pm_depth_pixel_gs(int n, const float *depth, const float *gt, int *mask, float *err, float *sign) {
    for (int i = 0; i < n; ++i) {
        const Pixel p = depth_pixel_gs(depth[i], gt[i]);
        mask[i] = p.mask ? 1 : 0;
        err[i] = p.d_err;
        sign[i] = p.d_sign;
    }
}

// get_loss' mask on the same inputs (no outlier rejection, no silhouette), for the comparison of the two modes
void pm_depth_pixel_map(int n, const float *depth, const float *depth_sq, const float *gt, int *mask, float *err, float *sign) {
    for (int i = 0; i < n; ++i) {
        const Pixel p = depth_pixel(false, false, 0.f, depth[i], 1.f, depth_sq[i], gt[i], 0.f);
        mask[i] = p.mask ? 1 : 0;
        err[i] = p.d_err;
        sign[i] = p.d_sign;
    }
}

float pm_depth_divisor(int gs, float mask_count, float num_pixels) { return map_depth_divisor(gs != 0, mask_count, num_pixels); }
float pm_depth_grad(int use_l1, float w_depth, float sign, float divisor) { return map_depth_grad(use_l1 != 0, w_depth, sign, divisor); }

// one frame in either mode: depth / depth_sq / gt [HW] -> sums[0] masked |gt - depth|, sums[1] mask count (doubles, as the kernels
// accumulate them), the weighted depth term and dL/d(depth) [HW]
void pm_frame(int gs, int HW, const float *depth, const float *depth_sq, const float *gt, float w_depth, double *sums, float *term, float *grad) {
    sums[0] = sums[1] = 0.0;
    for (int i = 0; i < HW; ++i) {
        const Pixel p = gs ? depth_pixel_gs(depth[i], gt[i]) : depth_pixel(false, false, 0.f, depth[i], 1.f, depth_sq[i], gt[i], 0.f);
        sums[0] += (double)p.d_err;
        sums[1] += p.mask ? 1.0 : 0.0;
    }
    const float divisor = map_depth_divisor(gs != 0, (float)sums[1], (float)HW);
    *term = w_depth * ((float)sums[0] / divisor);
    for (int i = 0; i < HW; ++i) {
        const Pixel p = gs ? depth_pixel_gs(depth[i], gt[i]) : depth_pixel(false, false, 0.f, depth[i], 1.f, depth_sq[i], gt[i], 0.f);
        grad[i] = map_depth_grad(true, w_depth, p.d_sign, divisor);
    }
}

}  // extern "C"

#ifdef POSTOPT_SHIM_MAIN
int main() {
    const int W = 37, H = 23, HW = W * H;
    std::vector<float> depth(HW), dsq(HW), gt(HW), grad(HW);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    for (int i = 0; i < HW; ++i) {
        depth[i] = 1.0f + 3.0f * rnd();
        dsq[i] = depth[i] * depth[i] + 0.01f * rnd();
        gt[i] = depth[i] + 0.2f * (rnd() - 0.5f);
        const int x = i % W, y = i / W;
        if (x < (2 * W) / 5 && y < H / 2) gt[i] = 0.f;         // a block of missing depth
    }
    gt[HW / 2 + 3] = -gt[HW / 2 + 3];                          // one negative depth: inside the gs mask, outside get_loss'
    gt[HW - 1] = depth[HW - 1];                                // an exact match: zero gradient
    double sums[2];
    float term = 0.f;
    pm_frame(1, HW, depth.data(), dsq.data(), gt.data(), 1.0f, sums, &term, grad.data());
    double want = 0.0, count = 0.0;
    int bad = 0;
    for (int i = 0; i < HW; ++i) {
        const bool valid = gt[i] != 0.0f;
        want += std::fabs((double)(valid ? depth[i] : 0.f) - (double)gt[i]);
        count += valid ? 1.0 : 0.0;
        const float d = depth[i] - gt[i];
        const float g = valid ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) / (float)HW : 0.f;
        if (g != grad[i]) ++bad;
    }
    const double rel = std::fabs(sums[0] - want) / want;
    double sums_map[2];
    float term_map = 0.f;
    pm_frame(0, HW, depth.data(), dsq.data(), gt.data(), 1.0f, sums_map, &term_map, grad.data());
    std::printf("gs: sum %.9g (want %.9g), count %.0f (want %.0f), term %.9g; get_loss: count %.0f, term %.9g; gradient mismatches %d\n", sums[0], want,
                sums[1], count, (double)term, sums_map[1], (double)term_map, bad);
    const bool ok = rel < 1e-6 && sums[1] == count && bad == 0 && sums_map[1] == count - 1.0 && std::fabs((double)term - want / HW) < 1e-6 * want / HW &&
                    grad[HW - 1] == 0.f;
    return ok ? 0 : 1;
}
#endif
