// meshrender.hip -- the mesh render layer: the depth image of a triangle mesh through a z-buffer, how many of a set of views see each
// vertex, and the sums depth L1 between two such images is made of.  The arithmetic is meshrender_math.h's.
//
//   R0 mr_clear_kernel    the plane, as uint32, to the bit pattern of +inf (16-byte stores where the plane allows).
//   R1 mr_raster_kernel   one lane per triangle sets it up (camera-space vertices, the three edge planes, the normal, the box).  A lane
//                         whose box holds at most 16 pixels (kMrSplit) walks it alone.  The others are taken one after the other by the whole
//                         WAVE: the owner's lane broadcasts the 13 floats and the box, and lane l tests pixels l, l + 64, ... of the box
//                         (a running row and column: no division per pixel),
//                         so no lane's loop is proportional to a large triangle's pixel count while 63 idle.  Large faces are found by
//                         a ballot, not a list: nothing is deferred, nothing can overflow.  Every loop is bounded by width x height.
//                         A hit enters the plane by an integer atomic min on the float's bits (positive floats order as their bits).
//                         A minimum does not depend on order: the same bits on every run.  (A plain load in front of the atomic, to
//                         spare it where the pixel already holds something nearer, was measured and lost.)
//   R2 mr_finish_kernel   +inf -> 0, the datasets' "no depth".
//   S  mr_seen_kernel     one lane per vertex loops over the views (the pose loads are wave-uniform) and adds its count to seen[v]:
//                         no atomics.
//   D  mr_compare_kernel  a workgroup per slice of the two planes, per lane running sums in double, a tree over the 256 lanes in LDS,
//                         one row of partials per workgroup; mr_compare_finish_kernel adds the rows in workgroup order.  No atomics.
#include "splat_device.h"
#include "meshrender_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr uint32_t kInfBits = 0x7f800000u;
constexpr int kCmp = 6;                 // partial sums per workgroup of D

unsigned blocks_for(long long n, int block) { return (unsigned)((n + block - 1) / block); }

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

// Faces are [F][3] int32 and vertices [V][3] float32: rows of 12 bytes, which no 16-byte access fits without straddling rows, so a
// lane reads its three indices and nine coordinates as 4-byte loads (consecutive lanes read consecutive rows: the wave's loads of the
// faces are contiguous).  Pixel offsets fit 32 bits: the entry point refuses more than 2^30 - 1 pixels.
template <int MODE>
__global__ void __launch_bounds__(kBlock) mr_raster_kernel(MrPinhole cam, float near_z, const float *__restrict__ w2c,
                                                           const float *__restrict__ vertices, int32_t V, const int32_t *__restrict__ faces,
                                                           int32_t F, int split, uint32_t *plane) {
    const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
    float m[12];
    for (int k = 0; k < 12; ++k) m[k] = w2c[k];
    MrFace face = {};                                                   // (kind 0: nothing)
    if (f < F) {
        const int32_t idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        mr_face_setup(cam, near_z, m, vertices, V, idx, split, face);
    }
    if (face.kind == kMrSmall) {
        for (int j = face.j0; j <= face.j1; ++j) {
            const float dy = mr_ray_y(cam, j);
            for (int i = face.i0; i <= face.i1; ++i) {
                float z;
                if (mr_hit(face, near_z, mr_ray_x(cam, i), dy, z)) mr_put<MODE>(plane, (uint32_t)j * cam.W + i, z);
            }
        }
    }
    // (no lane has left: the ballot and the broadcasts below need the whole wave)
    unsigned long long large = __ballot(face.kind == kMrLarge);
    const int lane = threadIdx.x & (kWave - 1);
    while (large) {
        const int src = __ffsll((long long)large) - 1;
        large &= large - 1;
        MrFace g;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) g.e[a][b] = __shfl(face.e[a][b], src, kWave);
        for (int a = 0; a < 3; ++a) g.n[a] = __shfl(face.n[a], src, kWave);
        g.na = __shfl(face.na, src, kWave);
        g.i0 = __shfl(face.i0, src, kWave); g.i1 = __shfl(face.i1, src, kWave);
        g.j0 = __shfl(face.j0, src, kWave); g.j1 = __shfl(face.j1, src, kWave);
        // lane l tests pixels l, l + 64, ... of the box in row order.  Two divisions per FACE (wave-uniform), none per pixel: a step of
        // 64 pixels is `rows` rows and `cols` columns, with one carry when the column leaves the box.
        const int bw = g.i1 - g.i0 + 1;
        const int rows = kWave / bw, cols = kWave % bw;
        int j = g.j0 + lane / bw, i = g.i0 + lane % bw;                 // (at most width x height / 64 trips: j grows every trip or two)
        float dy = mr_ray_y(cam, j);
        int row = j;
        while (j <= g.j1) {
            if (j != row) { dy = mr_ray_y(cam, j); row = j; }
            float z;
            if (mr_hit(g, near_z, mr_ray_x(cam, i), dy, z)) mr_put<MODE>(plane, (uint32_t)j * cam.W + i, z);
            i += cols;
            j += rows;
            if (i > g.i1) { i -= bw; ++j; }
        }
    }
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

MrPinhole pinhole_of(const SplatMeshView &v) {
    MrPinhole c;
    c.W = v.width; c.H = v.height;
    c.fx = v.fx; c.fy = v.fy; c.cx = v.cx; c.cy = v.cy;
    return c;
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
