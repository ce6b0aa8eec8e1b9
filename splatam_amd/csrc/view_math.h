// view_math.h -- arithmetic of the view layer (view.hip), written once as host/device inline functions: the kernels call them per
// lane, tests/test_view_math_cpu.py compiles the very same header with g++ (tests/view_math_shim.cpp, -ffp-contract=off) and checks it
// against the float64 numpy form of the same definitions (tests/view_ref.py).
//
//   V1  a rigid world-to-camera matrix -> what a camera of the fused engine reads: w2c (row-major), viewmatrix (its transpose),
//       projmatrix ((P w2c)^T with the OpenGL-style P of slam.setup_camera) and campos (-R^T t).  Sixteen-odd numbers per view, so every
//       step is taken in DOUBLE and each output is rounded to float32 once: at most half an ulp from the float64 evaluation, whatever
//       the translation's size (a float32 chain -- torch's setup_camera -- carries a few ulps of |t| into the projection's entries).
//   V2  one pixel of the 6-channel composite (r, g, b, depth, silhouette, depth^2) -> a display byte per channel (colour on any
//       background, depth through a 256-entry table, silhouette as grey) and a world-space point with its colour.  Every float32 step
//       of the bytes and colours is an operation of its own (view_mul / view_sub / view_div / view_fma: round-to-nearest intrinsics on the device, plain
//       operators under -ffp-contract=off on the host), so the byte a pixel gets does not depend on what a compiler contracts.
//
// Restates (in this project's words; nothing is copied) what the reference's viewers and saved evaluation frames compute on the host:
// the white-background composite and rgbd2pcd of /root/reference/viz_scripts/online_recon.py:119-181, the depth normalisation of
// /root/reference/utils/eval_helpers.py:509-528.
#pragma once

#include <math.h>
#include <stdint.h>

#include "splat_math.h"

namespace splat {

#if defined(__HIP_DEVICE_COMPILE__)
SPLAT_HD float view_mul(float a, float b) { return __fmul_rn(a, b); }
SPLAT_HD float view_sub(float a, float b) { return __fsub_rn(a, b); }
SPLAT_HD float view_div(float a, float b) { return __fdiv_rn(a, b); }
SPLAT_HD float view_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
SPLAT_HD float view_mul(float a, float b) { return a * b; }
SPLAT_HD float view_sub(float a, float b) { return a - b; }
SPLAT_HD float view_div(float a, float b) { return a / b; }
SPLAT_HD float view_fma(float a, float b, float c) { return fmaf(a, b, c); }
#endif

// ---------------------------------------------------------------------------------------------------------------- V1 (double)
// C = A B, row-major 4 x 4; C may not alias A or B
SPLAT_HD void view_mat4_mul(const double *A, const double *B, double *C) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) C[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + A[4 * r + 3] * B[12 + c];
}

// rel_w2c of a frame of the map as transform_to_frame forms it: R = build_rotation(normalize(q_raw)) (which normalises once more), t;
// q_raw[k] at q_ptr[k * stride], t[k] at t_ptr[k * stride] (fused_math.h pose_from_params is the loop's float32 form)
SPLAT_HD void view_rel_w2c(const float *q_ptr, const float *t_ptr, int stride, double *M) {
    double q[4] = {(double)q_ptr[0], (double)q_ptr[stride], (double)q_ptr[2 * stride], (double)q_ptr[3 * stride]};
    for (int pass = 0; pass < 2; ++pass) {
        double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (pass == 0 && n < 1e-12) n = 1e-12;                      // F.normalize's eps
        for (int k = 0; k < 4; ++k) q[k] /= n;
    }
    const double r = q[0], x = q[1], y = q[2], z = q[3];
    M[0] = 1.0 - 2.0 * (y * y + z * z); M[1] = 2.0 * (x * y - r * z); M[2] = 2.0 * (x * z + r * y); M[3] = (double)t_ptr[0];
    M[4] = 2.0 * (x * y + r * z); M[5] = 1.0 - 2.0 * (x * x + z * z); M[6] = 2.0 * (y * z - r * x); M[7] = (double)t_ptr[stride];
    M[8] = 2.0 * (x * z - r * y); M[9] = 2.0 * (y * z + r * x); M[10] = 1.0 - 2.0 * (x * x + y * y); M[11] = (double)t_ptr[2 * stride];
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

// the four outputs from the view's w2c M (row-major, double); viewmatrix / projmatrix in the library's layout (element (r, c) at [c*4+r])
SPLAT_HD void view_camera_outputs(const double *M, int w, int h, double fx, double fy, double cx, double cy, double near_z, double far_z,
                                  float *w2c, float *viewmatrix, float *projmatrix, float *campos) {
    const double P[16] = {2.0 * fx / w, 0.0, -(w - 2.0 * cx) / w, 0.0,
                          0.0, 2.0 * fy / h, -(h - 2.0 * cy) / h, 0.0,
                          0.0, 0.0, far_z / (far_z - near_z), -(far_z * near_z) / (far_z - near_z),
                          0.0, 0.0, 1.0, 0.0};
    double full[16];
    view_mat4_mul(P, M, full);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            w2c[4 * r + c] = (float)M[4 * r + c];
            viewmatrix[4 * c + r] = (float)M[4 * r + c];
            projmatrix[4 * c + r] = (float)full[4 * r + c];
        }
    for (int k = 0; k < 3; ++k) campos[k] = (float)-(M[k] * M[3] + M[4 + k] * M[7] + M[8 + k] * M[11]);
}

// ---------------------------------------------------------------------------------------------------------------- V2 (float32)
SPLAT_HD float view_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }      // (NaN -> 0: fmaxf returns its other operand)

// colour mode: the composite ran on a zero background and sum(weights) = silhouette, so a background of any colour is added here
SPLAT_HD float view_colour(float v, float sil, float bg) { return view_clamp01(view_fma(view_sub(1.f, sil), bg, v)); }
// silhouette mode: the viewers' show_sil, grey 1 - silhouette
SPLAT_HD float view_grey(float sil) { return view_clamp01(view_sub(1.f, sil)); }
// a value in 0..1 as a display byte: one multiplication, rounded to nearest (ties to even)
SPLAT_HD uint8_t view_byte(float c01) { return (uint8_t)(int)rintf(view_mul(c01, 255.f)); }
// depth mode: row of the colour table, trunc(clip((depth - vmin) / (vmax - vmin), 0, 1) * 255); vmin == vmax: 255 above it, else 0
SPLAT_HD int view_depth_index(float depth, float vmin, float vmax) {
    return (int)view_mul(view_clamp01(view_div(view_sub(depth, vmin), view_sub(vmax, vmin))), 255.f);
}

// c2w of a rigid w2c (row-major 4 x 4): rotation R^T (row-major), translation -R^T t.  The cloud is evaluated in DOUBLE from the float32
// planes and matrix and rounded once per coordinate: a float32 chain carries the translation's ulps (|t| ~ 10: 1e-6) into every point,
// and a dozen double operations per pixel cost nothing next to the 24 bytes the point and its colour take to store.
struct ViewC2W {
    double R[9], t[3];
};
SPLAT_HD void view_c2w(const float *w2c, ViewC2W &o) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = (double)w2c[4 * c + r];
        o.t[r] = -((double)w2c[r] * (double)w2c[3] + (double)w2c[4 + r] * (double)w2c[7] + (double)w2c[8 + r] * (double)w2c[11]);
    }
}
// pixel (u, v) at depth z in the world: c2w ((u - cx) / fx z, (v - cy) / fy z, z)
SPLAT_HD void view_point(const ViewC2W &m, float u, float v, float z, float fx, float fy, float cx, float cy, float *p) {
    const double Z = (double)z, X = ((double)u - (double)cx) / (double)fx * Z, Y = ((double)v - (double)cy) / (double)fy * Z;
    for (int r = 0; r < 3; ++r) p[r] = (float)(m.R[3 * r] * X + m.R[3 * r + 1] * Y + m.R[3 * r + 2] * Z + m.t[r]);
}

// what view.hip does with one pixel, for the kernel and for the host model alike
struct ViewFinish {
    int mode;                   // SPLAT_VIEW_COLOR / _DEPTH / _SILHOUETTE (0, 1, 2)
    float bg[3], vmin, vmax;
    const uint8_t *lut;         // [256][3], depth mode
    float fx, fy, cx, cy;
};
// rgb8[3] of a pixel from its r, g, b, depth, silhouette
SPLAT_HD void view_pixel_bytes(const ViewFinish &f, const float *rgb, float depth, float sil, uint8_t *out) {
    if (f.mode == 1) {
        const uint8_t *row = f.lut + 3 * view_depth_index(depth, f.vmin, f.vmax);
        out[0] = row[0]; out[1] = row[1]; out[2] = row[2];
    } else if (f.mode == 2) {
        out[0] = out[1] = out[2] = view_byte(view_grey(sil));
    } else {
        for (int c = 0; c < 3; ++c) out[c] = view_byte(view_colour(rgb[c], sil, f.bg[c]));
    }
}

}  // namespace splat
