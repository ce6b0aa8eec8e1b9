// meshrender.hip -- the mesh render layer: the depth image of a triangle mesh through a z-buffer, how many of a set of views see each
// vertex, and the sums depth L1 between two such images is made of.  The arithmetic is meshrender_math.h's.
//
//   R0 mr_clear_kernel    the plane, as uint32, to the bit pattern of +inf (16-byte stores where the plane allows).
//   R1 mr_raster_kernel   the raster walk of mesh_device.h (mesh_raster_walk: one lane per triangle, boxes of at most kMrSplit = 16
//                         pixels walked by their lane, the others by the whole wave), shared with meshshade.hip's V1.
//                         A hit enters the plane by an integer atomic min on the float's bits (positive floats order as their bits).
//                         A minimum does not depend on order: the same bits on every run.  (A plain load in front of the atomic, to
//                         spare it where the pixel already holds something nearer, was measured and lost.)
//   R2 mr_finish_kernel   +inf -> 0, the datasets' "no depth".
//   S  mr_seen_kernel     one lane per vertex loops over the views (the pose loads are wave-uniform) and adds its count to seen[v]:
//                         no atomics.
//   D  mr_compare_kernel  a workgroup per slice of the two planes, per lane running sums in double, a tree over the 256 lanes in LDS,
//                         one row of partials per workgroup; mr_compare_finish_kernel adds the rows in workgroup order.  No atomics.
#include "mesh_device.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kInfBits = 0x7f800000u;
constexpr int kCmp = 6;                 // partial sums per workgroup of D

__global__ void __launch_bounds__(kBlock) mr_clear_kernel(uint32_t *plane, long long n, int vec) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (vec) {
        if (4 * i + 3 < n) reinterpret_cast<uint4 *>(plane)[i] = make_uint4(kInfBits, kInfBits, kInfBits, kInfBits);
        else
            for (long long k = 4 * i; k < n; ++k) plane[k] = kInfBits;
    } else if (i < n) {
        plane[i] = kInfBits;
    }
}

__global__ void __launch_bounds__(kBlock) mr_finish_kernel(uint32_t *plane, long long n, int vec) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (vec) {
        if (4 * i + 3 < n) {
            uint4 q = reinterpret_cast<uint4 *>(plane)[i];
            q.x = q.x == kInfBits ? 0u : q.x; q.y = q.y == kInfBits ? 0u : q.y;
            q.z = q.z == kInfBits ? 0u : q.z; q.w = q.w == kInfBits ? 0u : q.w;
            reinterpret_cast<uint4 *>(plane)[i] = q;
        } else {
            for (long long k = 4 * i; k < n; ++k)
                if (plane[k] == kInfBits) plane[k] = 0u;
        }
    } else if (i < n && plane[i] == kInfBits) {
        plane[i] = 0u;
    }
}

// MODE 0 is the product: every hit goes to the atomic min, which returns nothing the lane waits for.  1 and 2 are the measurement builds
// of splat_debug_option(6, .): a plain load in front that spares the atomic when the pixel already holds something nearer (the plane
// only decreases, so a stale load can only let through an atomic that changes nothing: the same result) -- measured SLOWER, 93 us
// against 78 and 557 against 335 (profiles/mesh_render.md 2): the lane waits for the load, not for the atomic --, and a plain store.
template <int MODE>
__device__ __forceinline__ void mr_put(uint32_t *plane, uint32_t o, float z) {
    const uint32_t bits = __float_as_uint(z);                           // (z >= near > 0: the bits order as the values)
    if (MODE == 2) plane[o] = bits;
    else if (MODE == 0 || bits < plane[o]) atomicMin(plane + o, bits);
}

// the walk is mesh_device.h's; a hit is mr_put<MODE>'s and needs no face index
template <int MODE>
__global__ void __launch_bounds__(kBlock) mr_raster_kernel(MrPinhole cam, float near_z, const float *__restrict__ w2c,
                                                           const float *__restrict__ vertices, int32_t V, const int32_t *__restrict__ faces,
                                                           int32_t F, int split, uint32_t *plane) {
    mesh_raster_walk<kBlock>(cam, near_z, w2c, vertices, V, faces, F, split, [=](uint32_t o, float z, uint32_t) { mr_put<MODE>(plane, o, z); });
}

__global__ void __launch_bounds__(kBlock) mr_seen_kernel(MrPinhole cam, const float *__restrict__ w2c, int32_t n,
                                                         const float *__restrict__ vertices, int32_t V, int edge,
                                                         const float *__restrict__ depth, float eps, int32_t *seen) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const float p[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
    const size_t pixels = (size_t)cam.W * cam.H;
    int32_t count = 0;
    for (int32_t k = 0; k < n; ++k) {
        float m[12];
        for (int c = 0; c < 12; ++c) m[c] = w2c[16 * (size_t)k + c];
        count += mr_seen(cam, m, p, edge, depth ? depth + pixels * k : nullptr, eps) ? 1 : 0;
    }
    seen[v] += count;
}

__global__ void __launch_bounds__(kBlock) mr_compare_kernel(const float *__restrict__ a, const float *__restrict__ b, long long n, double *partials) {
    __shared__ double s[kCmp][kBlock];
    double all = 0.0, valid = 0.0, both = 0.0, ha = 0.0, hb = 0.0, mx = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float x = a[i], y = b[i];
        const bool okx = x > 0.f, oky = y > 0.f;
        const double d = fabs((okx ? (double)x : 0.0) - (oky ? (double)y : 0.0));      // (in double: no rounding at depths in metres)
        all += d;
        if (okx && oky) { valid += d; both += 1.0; }
        ha += okx ? 0.0 : 1.0;
        hb += oky ? 0.0 : 1.0;
        mx = d > mx ? d : mx;
    }
    const int t = threadIdx.x;
    s[0][t] = all; s[1][t] = valid; s[2][t] = both; s[3][t] = ha; s[4][t] = hb; s[5][t] = mx;
    __syncthreads();
    for (int h = kBlock / 2; h >= 1; h >>= 1) {
        if (t < h) {
            for (int c = 0; c < 5; ++c) s[c][t] += s[c][t + h];
            if (s[5][t + h] > s[5][t]) s[5][t] = s[5][t + h];
        }
        __syncthreads();
    }
    if (t < kCmp) partials[kCmp * blockIdx.x + t] = s[t][0];
}

__global__ void __launch_bounds__(kBlock) mr_compare_finish_kernel(const double *partials, int rows, long long n, double *row) {
    __shared__ double s_part[kCmp * SPLAT_MESH_COMPARE_ROWS];
    for (int k = threadIdx.x; k < kCmp * rows; k += kBlock) s_part[k] = partials[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double acc[kCmp] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < rows; ++r) {
        for (int c = 0; c < 5; ++c) acc[c] += s_part[kCmp * r + c];
        if (s_part[kCmp * r + 5] > acc[5]) acc[5] = s_part[kCmp * r + 5];
    }
    row[0] = acc[0]; row[1] = acc[1]; row[2] = acc[2]; row[3] = acc[3]; row[4] = acc[4];
    row[5] = (double)n; row[6] = acc[5]; row[7] = 0.0;
}

}  // namespace

int g_debug_mesh_split = 0;             // splat_debug_option(5, pixels): 0 = kMrSplit
int g_debug_mesh_bits = 0;              // splat_debug_option(6, bits)

hipError_t launch_mesh_depth(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const SplatMeshView &view, float *depth,
                             hipStream_t s) {
    const long long n = (long long)view.width * view.height;
    uint32_t *plane = reinterpret_cast<uint32_t *>(depth);
    const int vec = ((uintptr_t)depth & 15) == 0 ? 1 : 0;
    const unsigned blocks = blocks_for(vec ? (n + 3) / 4 : n, kBlock);
    hipLaunchKernelGGL(mr_clear_kernel, dim3(blocks), dim3(kBlock), 0, s, plane, n, vec);
    if (F > 0 && V > 0) {
        const int split = g_debug_mesh_split > 0 ? g_debug_mesh_split : kMrSplit;
        auto kernel = g_debug_mesh_bits == 1 ? mr_raster_kernel<1> : (g_debug_mesh_bits == 2 ? mr_raster_kernel<2> : mr_raster_kernel<0>);
        hipLaunchKernelGGL(kernel, dim3(blocks_for(F, kBlock)), dim3(kBlock), 0, s, pinhole_of(view), view.near_z, view.w2c, vertices, V, faces, F,
                           split, plane);
    }
    hipLaunchKernelGGL(mr_finish_kernel, dim3(blocks), dim3(kBlock), 0, s, plane, n, vec);
    return hipGetLastError();
}

hipError_t launch_mesh_seen(const float *vertices, int32_t V, const SplatMeshView &view, const float *w2c, int32_t n, int32_t edge,
                            const float *depth, float eps, int32_t *seen, hipStream_t s) {
    if (V == 0 || n == 0) return hipSuccess;
    hipLaunchKernelGGL(mr_seen_kernel, dim3(blocks_for(V, kBlock)), dim3(kBlock), 0, s, pinhole_of(view), w2c, n, vertices, V, edge, depth, eps, seen);
    return hipGetLastError();
}

hipError_t launch_mesh_depth_compare(const float *a, const float *b, long long n, double *partials, double *row, hipStream_t s) {
    long long rows = (n + kBlock - 1) / kBlock;
    rows = rows < 1 ? 1 : (rows > SPLAT_MESH_COMPARE_ROWS ? SPLAT_MESH_COMPARE_ROWS : rows);
    hipLaunchKernelGGL(mr_compare_kernel, dim3((unsigned)rows), dim3(kBlock), 0, s, a, b, n, partials);
    hipLaunchKernelGGL(mr_compare_finish_kernel, dim3(1), dim3(kBlock), 0, s, partials, (int)rows, n, row);
    return hipGetLastError();
}

}  // namespace splat
