// viewoverlay.hip -- the view overlay: where the cameras of a run went and where the map's Gaussians sit, drawn into a view of the map.
// Points and line segments share ONE depth-tested key plane; a last pass puts the winners' bytes into the picture.  The arithmetic is
// viewoverlay_math.h's.
//
//   O1 vo_run_kernel        one lane per frame of a range: its pose (the map's pose parameters or a given matrix, read on the device),
//                           its frustum's eight segments and the trajectory segment that ends at it, with their colours, into arrays
//                           the caller owns.  A few hundred double operations per lane; a full run is a few thousand lanes.
//   O0 (fill64)             the key plane to all ones (meshshade.hip's fill).
//   O2 vo_points_kernel     one lane per Gaussian row: its pixel, then one 64-bit unsigned atomic min per pixel of its footprint
//                           (at most 8 x 8, clipped).  The atomic returns nothing the lane waits for.
//   O3 vo_segments_kernel   one WAVE per segment: every lane sets the walk up (the same few dozen double operations: uniform, no LDS,
//                           no broadcast), then lanes stride over the steps, one atomic min per pixel of a step's width.  One LANE
//                           per segment, with the long walks of a wave taken by the whole wave in turn, was built and measured: no
//                           faster at any threshold, half as slow again at 16 steps (profiles/view_overlay.md 2).  The step count is
//                           bounded by max(W, H) + 1 (vo_line).
//   O4 vo_finish_kernel     one lane per pixel: its key, the scene's depth there, and -- where the primitive is seen -- three bytes.
//                           With `fill` the pixels nothing is drawn on get the background (the `centers` picture: no composite ran).
#include "splat_device.h"
#include "viewoverlay_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
struct OverlayCam {
    MrPinhole cam;
    float near_z;
    const float *w2c;
    uint64_t *keys;
};

OverlayCam overlay_cam(const SplatViewOverlay &v) {
    OverlayCam o;
    o.cam.W = v.width; o.cam.H = v.height;
    o.cam.fx = v.fx; o.cam.fy = v.fy; o.cam.cx = v.cx; o.cam.cy = v.cy;
    o.near_z = v.near_z; o.w2c = v.w2c; o.keys = v.keys;
    return o;
}

__device__ __forceinline__ void vo_put(uint64_t *keys, uint32_t o, float z, uint32_t id) {
    // (the result is not used: an atomic without return)
    __hip_atomic_fetch_min((unsigned long long *)keys + o, (unsigned long long)msh_key(z, id), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kBlock) vo_run_kernel(VoRun r, int first, int count, float *segments, uint8_t *colors) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    vo_run_frame(r, first + i, segments, colors);
}

__global__ void __launch_bounds__(kBlock) vo_points_kernel(OverlayCam o, const float *__restrict__ means3D, int32_t count, int size) {
    const long long row = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (row >= count) return;
    float m[12];
    for (int k = 0; k < 12; ++k) m[k] = o.w2c[k];
    const float p[3] = {means3D[3 * row], means3D[3 * row + 1], means3D[3 * row + 2]};
    const VoBox b = vo_point(o.cam, o.near_z, m, p, size);
    for (int j = b.j0; j <= b.j1; ++j)
        for (int i = b.i0; i <= b.i1; ++i) vo_put(o.keys, (uint32_t)j * (uint32_t)o.cam.W + (uint32_t)i, b.z, (uint32_t)row);
}

__global__ void __launch_bounds__(kBlock) vo_segments_kernel(OverlayCam o, const float *__restrict__ segments, int32_t first, int32_t count,
                                                             int width) {
    const long long s = (long long)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (s >= count) return;
    const uint32_t index = (uint32_t)first + (uint32_t)s;
    float m[12], seg[6];
    for (int k = 0; k < 12; ++k) m[k] = o.w2c[k];
    for (int k = 0; k < 6; ++k) seg[k] = segments[6 * (size_t)index + k];
    const VoLine L = vo_line(o.cam, o.near_z, m, seg);
    uint64_t *keys = o.keys;
    for (int k = threadIdx.x % kWave; k < L.steps; k += kWave)
        vo_line_stamp(o.cam, L, k, width, [=](uint32_t at, float z) { vo_put(keys, at, z, kVoSegmentBit | index); });
}

struct FinishArgs {
    VoResolve r;
    const uint64_t *keys;
    const float *depth;
    int fill;
    uint8_t bg[3];
    uint8_t *rgb8;
    long long pixels;
};

__global__ void __launch_bounds__(kBlock) vo_finish_kernel(FinishArgs a) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.pixels) return;
    const uint64_t key = a.keys[p];
    if (key == kMshNoKey && !a.fill) return;
    uint8_t out[3] = {a.bg[0], a.bg[1], a.bg[2]};
    const float d = a.depth && key != kMshNoKey ? a.depth[p] : 0.f;
    if (!vo_resolve(a.r, key, d, out) && !a.fill) return;
    a.rgb8[3 * p] = out[0]; a.rgb8[3 * p + 1] = out[1]; a.rgb8[3 * p + 2] = out[2];
}

}  // namespace

hipError_t launch_view_run_segments(const SplatViewRun &run, hipStream_t s) {
    VoRun r;
    r.num_frames = run.num_frames;
    r.w2c_all = run.w2c_all;
    r.cam_unnorm_rots = run.cam_unnorm_rots; r.cam_trans = run.cam_trans; r.first_w2c = run.first_w2c;
    r.w = run.width; r.h = run.height;
    r.fx = run.fx; r.fy = run.fy; r.cx = run.cx; r.cy = run.cy; r.scale = run.scale;
    r.frusta = run.frusta; r.fixed = run.fixed_color;
    for (int k = 0; k < 3; ++k) r.color[k] = run.color[k];
    if (run.count > 0)
        hipLaunchKernelGGL(vo_run_kernel, dim3(blocks_for(run.count, kBlock)), dim3(kBlock), 0, s, r, run.first, run.count, run.segments, run.colors);
    return hipGetLastError();
}

hipError_t launch_view_overlay_clear(const SplatViewOverlay &v, hipStream_t s) {
    return fill64(v.keys, (long long)v.width * v.height, kMshNoKey, s);
}

hipError_t launch_view_points(const SplatViewOverlay &v, const float *means3D, int32_t count, int32_t point_size, hipStream_t s) {
    if (count > 0)
        hipLaunchKernelGGL(vo_points_kernel, dim3(blocks_for(count, kBlock)), dim3(kBlock), 0, s, overlay_cam(v), means3D, count, point_size);
    return hipGetLastError();
}

hipError_t launch_view_segments(const SplatViewOverlay &v, const float *segments, int32_t first, int32_t count, int32_t line_width,
                                hipStream_t s) {
    if (count > 0)
        hipLaunchKernelGGL(vo_segments_kernel, dim3(blocks_for(count, kBlock / kWave)), dim3(kBlock), 0, s, overlay_cam(v), segments, first, count,
                           line_width);
    return hipGetLastError();
}

hipError_t launch_view_overlay_finish(const SplatViewOverlay &v, const SplatViewOverlayFinish &f, hipStream_t s) {
    FinishArgs a;
    a.r.occlude = f.occlude; a.r.rgb_colors = f.rgb_colors; a.r.rows = f.num_rows;
    a.r.segment_colors = f.segment_colors; a.r.segments = f.num_segments;
    a.keys = v.keys; a.depth = f.depth; a.fill = f.fill;
    for (int k = 0; k < 3; ++k) a.bg[k] = view_byte(view_clamp01(f.bg[k]));
    a.rgb8 = f.rgb8; a.pixels = (long long)v.width * v.height;
    hipLaunchKernelGGL(vo_finish_kernel, dim3(blocks_for(a.pixels, kBlock)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace splat
