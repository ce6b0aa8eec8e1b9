// Host build of splatam_amd/csrc/eval_math.h for tests/test_eval_cpu.py: the functions one by one, and a plain-loop model of a
// whole frame (em_frame) that calls nothing but them -- window, weighting, ssim pixel, pooling rule, finish -- so that the index
// rules the kernels follow are checked against the torch restatement without a GPU.
#include <vector>

#include "../splatam_amd/csrc/eval_math.h"

using namespace splat;

extern "C" {

void em_window(float *g) { eval_window(g); }
int em_pool_size(int n) { return eval_pool_size(n); }
int em_pool_first(int p, int n) { return eval_pool_first(p, n); }
int em_level_size(int n, int level) { return eval_level_size(n, level); }
size_t em_pyramid_floats(int W, int H) { return eval_pyramid_floats(W, H); }
int em_level_slot(int level, int ch) { return eval_level_slot(level, ch); }

void em_ssim_pixel(int n, const float *mu1, const float *mu2, const float *e11, const float *e22, const float *e12, float *ss, float *cs) {
    for (int i = 0; i < n; ++i) ss[i] = eval_ssim_pixel(mu1[i], mu2[i], e11[i], e22[i], e12[i], &cs[i]);
}

// per pixel: weighted rendered value, weighted ground truth, depth term, valid factor
void em_pixel(int n, const float *im, const float *gt, const float *depth, const float *gt_depth, const float *sil, float sil_thres,
              int sil_mask, float *wx, float *wy, float *dterm, float *vf) {
    for (int i = 0; i < n; ++i) {
        const EvalPixel m = eval_masks(gt_depth[i], sil[i], sil_thres, sil_mask != 0);
        wx[i] = eval_weighted(im[i], m, sil_mask != 0);
        wy[i] = eval_weighted(gt[i], m, sil_mask != 0);
        dterm[i] = eval_depth_term(depth[i], gt_depth[i], m, sil_mask != 0);
        vf[i] = m.vf;
    }
}

void em_finish(const double *tot, int W, int H, int ms_ssim, double *row) { eval_finish(tot, W, H, ms_ssim != 0, row); }

// one frame: rgb / gt_im [3][H][W], depth / sil / gt_depth [H][W] -> totals [kEvalSums] and the row [8]
void em_frame(int W, int H, const float *rgb, const float *depth, const float *sil, const float *gt_im, const float *gt_depth,
              float sil_thres, int sil_mask, double *tot, double *row) {
    float g[kEvalTaps];
    eval_window(g);
    for (int k = 0; k < kEvalSums; ++k) tot[k] = 0.0;
    const size_t HW = (size_t)W * H;
    std::vector<float> X(3 * HW), Y(3 * HW);
    for (size_t i = 0; i < HW; ++i) {
        const EvalPixel m = eval_masks(gt_depth[i], sil[i], sil_thres, sil_mask != 0);
        for (int ch = 0; ch < 3; ++ch) {
            X[ch * HW + i] = eval_weighted(rgb[ch * HW + i], m, sil_mask != 0);
            Y[ch * HW + i] = eval_weighted(gt_im[ch * HW + i], m, sil_mask != 0);
            const float d = X[ch * HW + i] - Y[ch * HW + i];
            tot[kEvalSumSq + ch] += (double)(d * d);
        }
        tot[kEvalSumDepth] += (double)eval_depth_term(depth[i], gt_depth[i], m, sil_mask != 0);
        tot[kEvalSumValid] += (double)m.vf;
    }
    int w = W, h = H;
    for (int level = 0; level < kEvalLevels; ++level) {
        const size_t hw = (size_t)w * h;
        for (int ch = 0; ch < 3; ++ch) {
            const float *x = X.data() + ch * hw, *y = Y.data() + ch * hw;
            // vertical pass, then horizontal, as the kernels order them
            std::vector<float> v(5 * (size_t)(h - 10) * w);
            for (int oy = 0; oy + 10 < h; ++oy)
                for (int xx = 0; xx < w; ++xx) {
                    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                    for (int t = 0; t < kEvalTaps; ++t) {
                        const float a = x[(size_t)(oy + t) * w + xx], b = y[(size_t)(oy + t) * w + xx];
                        s[0] += g[t] * a; s[1] += g[t] * b; s[2] += g[t] * (a * a); s[3] += g[t] * (b * b); s[4] += g[t] * (a * b);
                    }
                    for (int k = 0; k < 5; ++k) v[((size_t)k * (h - 10) + oy) * w + xx] = s[k];
                }
            double cs_sum = 0.0, ss_sum = 0.0;
            for (int oy = 0; oy + 10 < h; ++oy)
                for (int ox = 0; ox + 10 < w; ++ox) {
                    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                    for (int t = 0; t < kEvalTaps; ++t)
                        for (int k = 0; k < 5; ++k) s[k] += g[t] * v[((size_t)k * (h - 10) + oy) * w + ox + t];
                    float cs;
                    const float ss = eval_ssim_pixel(s[0], s[1], s[2], s[3], s[4], &cs);
                    cs_sum += (double)cs;
                    ss_sum += (double)ss;
                }
            tot[eval_level_slot(level, ch)] = cs_sum;
            tot[eval_level_slot(level, ch) + 1] = ss_sum;
        }
        if (level == kEvalLevels - 1) break;
        const int pw = eval_pool_size(w), ph = eval_pool_size(h);
        std::vector<float> PX(3 * (size_t)pw * ph), PY(3 * (size_t)pw * ph);
        for (int ch = 0; ch < 3; ++ch)
            for (int py = 0; py < ph; ++py)
                for (int px = 0; px < pw; ++px) {
                    float sx = 0.f, sy = 0.f;
                    for (int k = 0; k < 4; ++k) {
                        const int ix = eval_pool_first(px, w) + (k & 1), iy = eval_pool_first(py, h) + (k >> 1);
                        if (ix < 0 || iy < 0) continue;
                        sx += X[ch * hw + (size_t)iy * w + ix];
                        sy += Y[ch * hw + (size_t)iy * w + ix];
                    }
                    PX[((size_t)ch * ph + py) * pw + px] = 0.25f * sx;
                    PY[((size_t)ch * ph + py) * pw + px] = 0.25f * sy;
                }
        X.swap(PX);
        Y.swap(PY);
        w = pw;
        h = ph;
    }
    eval_finish(tot, W, H, true, row);
}

}  // extern "C"
