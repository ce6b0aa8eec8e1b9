// view.hip -- the view layer: a camera that moves in place, and the 6-channel composite as something a window, a PNG writer or a
// point-cloud consumer takes.  The arithmetic is view_math.h's.
//
//   V1 view_camera_kernel        one workgroup, one working lane: a rigid w2c (16 device floats, or a pose of the map composed with the
//                                first frame's w2c), an optional offset multiplied from the left -> the view's w2c, viewmatrix, projmatrix,
//                                campos in buffers the caller owns.  ~300 double operations; the launch is its cost.  Nothing is read on
//                                the host: the pose may be one an earlier kernel on the stream has just written.
//   V2 view_finish_kernel<V>     one lane = V consecutive pixels of one row (V = 4 when the width is a multiple of 4 and every buffer
//                                involved starts where its vector accesses need it, else 1), consecutive lanes consecutive pixels.
//                                With V = 4 a lane loads 16 bytes per plane it needs, stores the 12 bytes of rgb8 as three dwords and
//                                the cloud as three float4 per array (a wave: 768 contiguous bytes of rgb8, 3 KiB of each cloud
//                                array).  No LDS, no atomics, plain stores; the 768-byte colour table stays in the vector cache.
#include "splat_device.h"
#include "view_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;

struct ViewCameraArgs {
    const float *w2c_in;                    // matrix form, or NULL for the map-pose form:
    const float *cam_unnorm_rots, *cam_trans, *first_w2c;
    int num_frames, time_idx;
    int has_offset;
    double offset[16];
    int w, h;
    double fx, fy, cx, cy, near_z, far_z;
    float *w2c, *viewmatrix, *projmatrix, *campos;
};

__global__ void __launch_bounds__(64) view_camera_kernel(ViewCameraArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double M[16], T[16];
    if (a.w2c_in) {
        for (int i = 0; i < 16; ++i) M[i] = (double)a.w2c_in[i];
    } else {
        double first[16];
        for (int i = 0; i < 16; ++i) first[i] = (double)a.first_w2c[i];
        view_rel_w2c(a.cam_unnorm_rots + a.time_idx, a.cam_trans + a.time_idx, a.num_frames, T);
        view_mat4_mul(first, T, M);
    }
    if (a.has_offset) {
        view_mat4_mul(a.offset, M, T);
        for (int i = 0; i < 16; ++i) M[i] = T[i];
    }
    view_camera_outputs(M, a.w, a.h, a.fx, a.fy, a.cx, a.cy, a.near_z, a.far_z, a.w2c, a.viewmatrix, a.projmatrix, a.campos);
}

struct ViewFinishArgs {
    ViewFinish f;
    int W, H;
    const float *out6, *w2c;
    uint8_t *rgb8;
    float *points, *colors;
};

template <int V>
__global__ void __launch_bounds__(kBlock) view_finish_kernel(ViewFinishArgs a) {
    const int per_row = a.W / V;                                    // (V divides W: the launcher's choice)
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)per_row * a.H) return;
    const int y = (int)(i / per_row), x0 = (int)(i % per_row) * V;
    const size_t plane = (size_t)a.W * a.H, o = (size_t)y * a.W + x0;
    const bool cloud = a.points != nullptr || a.colors != nullptr;
    const bool need_rgb = cloud || (a.rgb8 && a.f.mode == 0), need_depth = a.points || (a.rgb8 && a.f.mode == 1);
    const bool need_sil = cloud || (a.rgb8 && a.f.mode != 1);
    float ch[5][V];                                                 // r, g, b, depth, silhouette of the lane's pixels
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const bool need = c < 3 ? need_rgb : (c == 3 ? need_depth : need_sil);
        if (need) {
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(a.out6 + c * plane + o);
                ch[c][0] = q.x; ch[c][1] = q.y; ch[c][2] = q.z; ch[c][3] = q.w;
            } else {
                ch[c][0] = a.out6[c * plane + o];
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) ch[c][v] = 0.f;
        }
    }
    if (a.rgb8) {
        uint8_t b[3 * V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float rgb[3] = {ch[0][v], ch[1][v], ch[2][v]};
            view_pixel_bytes(a.f, rgb, ch[3][v], ch[4][v], b + 3 * v);
        }
        if constexpr (V == 4) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(a.rgb8 + 3 * o);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                dst[q] = (uint32_t)b[4 * q] | ((uint32_t)b[4 * q + 1] << 8) | ((uint32_t)b[4 * q + 2] << 16) | ((uint32_t)b[4 * q + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.rgb8[3 * o + k] = b[k];
        }
    }
    if (cloud) {
        float pts[3 * V], col[3 * V];
        ViewC2W m;
        if (a.points) view_c2w(a.w2c, m);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (a.points) view_point(m, (float)(x0 + v), (float)y, ch[3][v], a.f.fx, a.f.fy, a.f.cx, a.f.cy, pts + 3 * v);
#pragma unroll
            for (int c = 0; c < 3; ++c) col[3 * v + c] = view_colour(ch[c][v], ch[4][v], a.f.bg[c]);
        }
        if constexpr (V == 4) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (a.points) reinterpret_cast<float4 *>(a.points + 3 * o)[q] = make_float4(pts[4 * q], pts[4 * q + 1], pts[4 * q + 2], pts[4 * q + 3]);
                if (a.colors) reinterpret_cast<float4 *>(a.colors + 3 * o)[q] = make_float4(col[4 * q], col[4 * q + 1], col[4 * q + 2], col[4 * q + 3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (a.points) a.points[3 * o + k] = pts[k];
                if (a.colors) a.colors[3 * o + k] = col[k];
            }
        }
    }
}

}  // namespace

hipError_t launch_view_camera(const SplatViewArgs &v, hipStream_t s) {
    ViewCameraArgs a;
    a.w2c_in = v.w2c_in;
    a.cam_unnorm_rots = v.cam_unnorm_rots; a.cam_trans = v.cam_trans; a.first_w2c = v.first_w2c;
    a.num_frames = v.num_frames; a.time_idx = v.time_idx;
    a.has_offset = v.offset != nullptr;
    for (int i = 0; i < 16; ++i) a.offset[i] = v.offset ? v.offset[i] : 0.0;
    a.w = v.width; a.h = v.height;
    a.fx = v.fx; a.fy = v.fy; a.cx = v.cx; a.cy = v.cy; a.near_z = v.near_z; a.far_z = v.far_z;
    a.w2c = v.w2c; a.viewmatrix = v.viewmatrix; a.projmatrix = v.projmatrix; a.campos = v.campos;
    hipLaunchKernelGGL(view_camera_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_view_finish(const SplatViewArgs &v, hipStream_t s) {
    ViewFinishArgs a;
    a.f.mode = v.mode;
    for (int c = 0; c < 3; ++c) a.f.bg[c] = v.bg[c];
    a.f.vmin = v.vmin; a.f.vmax = v.vmax; a.f.lut = v.lut;
    a.f.fx = (float)v.fx; a.f.fy = (float)v.fy; a.f.cx = (float)v.cx; a.f.cy = (float)v.cy;
    a.W = v.width; a.H = v.height;
    a.out6 = v.out6; a.w2c = v.w2c; a.rgb8 = v.rgb8; a.points = v.points; a.colors = v.colors;
    // V = 4: every plane's every row on 16 bytes (width a multiple of 4, out6 aligned), a lane's 12 bytes of rgb8 on 4, its 48 bytes of
    // each cloud array on 16
    const bool vec = v.width % 4 == 0 && ((uintptr_t)v.out6 & 15) == 0 && ((uintptr_t)v.rgb8 & 3) == 0
                     && (((uintptr_t)v.points | (uintptr_t)v.colors) & 15) == 0;
    const long long items = (long long)(vec ? v.width / 4 : v.width) * v.height;
    const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));
    if (vec) hipLaunchKernelGGL(view_finish_kernel<4>, grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(view_finish_kernel<1>, grid, dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace splat
