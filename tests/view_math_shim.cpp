// Host build of splatam_amd/csrc/view_math.h for tests/test_view_math_cpu.py: the camera arithmetic of splat_view_camera in both of its
// forms, and a plain-loop model of splat_view_finish (vm_finish) that calls nothing but the header's per-pixel functions, so that the
// view layer is checked against the float64 restatement (tests/view_ref.py) without a GPU.  Built with -ffp-contract=off: every
// float32 step of the header is then one operation, as the device's round-to-nearest intrinsics make it there.
#include "../splatam_amd/csrc/view_math.h"

using namespace splat;

extern "C" {

// matrix form: w2c_in (16 floats, row-major), offset (16 doubles or NULL)
void vm_camera_matrix(const float *w2c_in, const double *offset, int w, int h, double fx, double fy, double cx, double cy, double near_z,
                      double far_z, float *w2c, float *viewmatrix, float *projmatrix, float *campos) {
    double M[16], T[16];
    for (int i = 0; i < 16; ++i) M[i] = (double)w2c_in[i];
    if (offset) {
        view_mat4_mul(offset, M, T);
        for (int i = 0; i < 16; ++i) M[i] = T[i];
    }
    view_camera_outputs(M, w, h, fx, fy, cx, cy, near_z, far_z, w2c, viewmatrix, projmatrix, campos);
}

// map-pose form: cam_unnorm_rots [1][4][num_frames], cam_trans [1][3][num_frames], first_w2c (16 floats)
void vm_camera_pose(const float *rots, const float *trans, int num_frames, int time_idx, const float *first_w2c, const double *offset, int w,
                    int h, double fx, double fy, double cx, double cy, double near_z, double far_z, float *w2c, float *viewmatrix,
                    float *projmatrix, float *campos) {
    double first[16], M[16], T[16];
    for (int i = 0; i < 16; ++i) first[i] = (double)first_w2c[i];
    view_rel_w2c(rots + time_idx, trans + time_idx, num_frames, T);
    view_mat4_mul(first, T, M);
    if (offset) {
        view_mat4_mul(offset, M, T);
        for (int i = 0; i < 16; ++i) M[i] = T[i];
    }
    view_camera_outputs(M, w, h, fx, fy, cx, cy, near_z, far_z, w2c, viewmatrix, projmatrix, campos);
}

// out6 [>= 5][H][W] -> rgb8 [H][W][3], points / colors [H W][3] (each may be NULL): the kernel's loop body over every pixel
void vm_finish(int W, int H, const float *out6, int mode, const float *bg, float vmin, float vmax, const uint8_t *lut, float fx, float fy,
               float cx, float cy, const float *w2c, uint8_t *rgb8, float *points, float *colors) {
    ViewFinish f;
    f.mode = mode;
    for (int c = 0; c < 3; ++c) f.bg[c] = bg[c];
    f.vmin = vmin; f.vmax = vmax; f.lut = lut;
    f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy;
    ViewC2W m;
    if (points) view_c2w(w2c, m);
    const size_t plane = (size_t)W * H;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t o = (size_t)y * W + x;
            const float rgb[3] = {out6[o], out6[plane + o], out6[2 * plane + o]};
            const float depth = out6[3 * plane + o], sil = out6[4 * plane + o];
            if (rgb8) view_pixel_bytes(f, rgb, depth, sil, rgb8 + 3 * o);
            if (points) view_point(m, (float)x, (float)y, depth, fx, fy, cx, cy, points + 3 * o);
            if (colors)
                for (int c = 0; c < 3; ++c) colors[3 * o + c] = view_colour(rgb[c], sil, bg[c]);
        }
}

}
