// meshshade.hip -- the mesh shade layer: pictures of a triangle mesh.  Area-weighted vertex normals, a z-buffer that remembers WHICH
// triangle won each pixel, and a shading pass from that buffer to display bytes.  The arithmetic is meshshade_math.h's (and, for the
// raster, meshrender_math.h's, unchanged).
//
//   N0 ms_fill64_kernel   the sums [V][3] int64 to zero (16-byte stores where the buffer allows).
//   N1 ms_normal_faces    one lane per face: its normal's quanta added to its three vertices by 64-bit integer atomics.  Integer sums
//                         are exact and do not depend on order: the same bits on every run and for every order of the faces.
//   N2 ms_normal_vertices one lane per vertex: the three sums, normalised in double, rounded once.
//   V0 ms_fill64_kernel   the key plane to all ones.
//   V1 ms_raster_kernel   meshrender.hip's R1 with an identity attached: the SAME walk (mesh_device.h's mesh_raster_walk, one
//                         definition for both), which hands every hit the index of its face.  A hit enters the plane by a 64-bit
//                         unsigned atomic min of (bits(z) << 32) | face, which returns nothing the lane waits for (a guarding load in
//                         front of it lost in R1: profiles/mesh_render.md 2).
//   S  ms_shade_kernel    one lane per OUTPUT pixel: its samples x samples keys, each decoded (the face id is range-checked before any
//                         load), set up again and shaded (msh_sample), summed and written as three bytes; with samples == 1 the depth,
//                         face and normal planes too.  The only loop is bounded by samples^2 <= 16.
#include "mesh_device.h"
#include "meshshade_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;

// n words of 8 bytes to `value`; vec: the buffer starts on 16 bytes and lane i stores words 2 i and 2 i + 1 at once
__global__ void __launch_bounds__(kBlock) ms_fill64_kernel(uint64_t *p, long long n, uint64_t value, int vec) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (vec) {
        const uint32_t lo = (uint32_t)value, hi = (uint32_t)(value >> 32);
        if (2 * i + 1 < n) reinterpret_cast<uint4 *>(p)[i] = make_uint4(lo, hi, lo, hi);
        else if (2 * i < n) p[2 * i] = value;
    } else if (i < n) {
        p[i] = value;
    }
}

}  // namespace

hipError_t fill64(void *p, long long n, uint64_t value, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int vec = ((uintptr_t)p & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(ms_fill64_kernel, dim3(blocks_for(vec ? (n + 1) / 2 : n, kBlock)), dim3(kBlock), 0, s, (uint64_t *)p, n, value, vec);
    return hipGetLastError();
}

namespace {

__global__ void __launch_bounds__(kBlock) ms_normal_faces(const float *__restrict__ vertices, int32_t V, const int32_t *__restrict__ faces, int32_t F,
                                                          int64_t *accum) {
    const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    const int32_t idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    msh_add_face(vertices, V, idx, accum);
}

__global__ void __launch_bounds__(kBlock) ms_normal_vertices(const int64_t *__restrict__ accum, int32_t V, float *normals) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const int64_t acc[3] = {accum[3 * v], accum[3 * v + 1], accum[3 * v + 2]};
    float n[3];
    msh_vertex_normal(acc, n);
    normals[3 * v] = n[0]; normals[3 * v + 1] = n[1]; normals[3 * v + 2] = n[2];
}

__device__ __forceinline__ void ms_put(uint64_t *keys, uint32_t o, float z, uint32_t f) {
    // (the result is not used: an atomic without return, nothing the lane waits for)
    __hip_atomic_fetch_min((unsigned long long *)keys + o, (unsigned long long)msh_key(z, f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the walk is mesh_device.h's, hit for hit meshrender.hip's mr_raster_kernel; a hit is ms_put's
__global__ void __launch_bounds__(kBlock) ms_raster_kernel(MrPinhole cam, float near_z, const float *__restrict__ w2c,
                                                           const float *__restrict__ vertices, int32_t V, const int32_t *__restrict__ faces,
                                                           int32_t F, int split, uint64_t *keys) {
    mesh_raster_walk<kBlock>(cam, near_z, w2c, vertices, V, faces, F, split, [=](uint32_t o, float z, uint32_t f) { ms_put(keys, o, z, f); });
}

struct ShadeOut {
    uint8_t *rgb8;
    float *depth;
    int32_t *face;
    float *normal;
};

__global__ void __launch_bounds__(kBlock) ms_shade_kernel(MrPinhole cam, float near_z, const float *__restrict__ w2c,
                                                          const float *__restrict__ vertices, int32_t V, const int32_t *__restrict__ faces,
                                                          int32_t F, const float *__restrict__ colors, const float *__restrict__ normals,
                                                          MshShade args, const uint64_t *__restrict__ keys, int W, int H, ShadeOut out) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (long long)W * H) return;
    const int j = (int)(p / W), i = (int)(p - (long long)j * W);
    float m[12];
    for (int k = 0; k < 12; ++k) m[k] = w2c[k];
    uint8_t rgb[3];
    MshSample last;
    msh_pixel(cam, near_z, m, vertices, V, faces, F, colors, normals, args, keys, i, j, rgb, last);
    out.rgb8[3 * p] = rgb[0]; out.rgb8[3 * p + 1] = rgb[1]; out.rgb8[3 * p + 2] = rgb[2];
    if (out.depth) out.depth[p] = last.z;                               // (samples == 1: `last` is the pixel's one sample)
    if (out.face) out.face[p] = last.face;
    if (out.normal) { out.normal[3 * p] = last.n[0]; out.normal[3 * p + 1] = last.n[1]; out.normal[3 * p + 2] = last.n[2]; }
}

}  // namespace

hipError_t launch_mesh_vertex_normals(const float *vertices, int32_t V, const int32_t *faces, int32_t F, int64_t *accum, float *normals,
                                      hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipError_t e = fill64(accum, 3LL * V, 0, s);
    if (e != hipSuccess) return e;
    if (F > 0) hipLaunchKernelGGL(ms_normal_faces, dim3(blocks_for(F, kBlock)), dim3(kBlock), 0, s, vertices, V, faces, F, accum);
    hipLaunchKernelGGL(ms_normal_vertices, dim3(blocks_for(V, kBlock)), dim3(kBlock), 0, s, accum, V, normals);
    return hipGetLastError();
}

hipError_t launch_mesh_visibility(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const SplatMeshView &view, uint64_t *keys,
                                  hipStream_t s) {
    hipError_t e = fill64(keys, (long long)view.width * view.height, kMshNoKey, s);
    if (e != hipSuccess) return e;
    if (F > 0 && V > 0) {
        const int split = g_debug_mesh_split > 0 ? g_debug_mesh_split : kMrSplit;
        hipLaunchKernelGGL(ms_raster_kernel, dim3(blocks_for(F, kBlock)), dim3(kBlock), 0, s, pinhole_of(view), view.near_z, view.w2c, vertices, V,
                           faces, F, split, keys);
    }
    return hipGetLastError();
}

hipError_t launch_mesh_shade(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const float *colors, const float *normals,
                             const SplatMeshView &view, const uint64_t *keys, const SplatMeshShade &a, uint8_t *rgb8, float *depth, int32_t *face,
                             float *normal, hipStream_t s) {
    MshShade args;
    args.mode = a.mode; args.samples = a.samples; args.smooth = a.smooth; args.normal_frame = a.normal_frame;
    for (int k = 0; k < 3; ++k) { args.bg[k] = a.bg[k]; args.albedo[k] = a.albedo[k]; }
    args.ambient = a.ambient; args.vmin = a.vmin; args.vmax = a.vmax;
    args.lut = a.lut;
    const int W = view.width / a.samples, H = view.height / a.samples;
    const ShadeOut out = {rgb8, depth, face, normal};
    hipLaunchKernelGGL(ms_shade_kernel, dim3(blocks_for((long long)W * H, kBlock)), dim3(kBlock), 0, s, pinhole_of(view), view.near_z, view.w2c,
                       vertices, V, V > 0 ? faces : nullptr, V > 0 ? F : 0, colors, normals, args, keys, W, H, out);
    return hipGetLastError();
}

}  // namespace splat
