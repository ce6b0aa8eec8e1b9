// tsdf.hip -- the mesh layer: rendered depth fused into a truncated signed distance volume, and the volume's zero surface as a
// triangle mesh.  The arithmetic is tsdf_math.h's; what these kernels share with the sparse volume's (tsdf_sparse.hip) is defined once,
// in tsdf_device.h, named below.
//
//   T0 tsdf_reset_kernel<V>      tsdf = 1, weight = r = g = b = 0: V floats per lane and array (16-byte stores where the arrays allow).
//   T1 tsdf_integrate_kernel<V>  one launch per view.  A workgroup owns a brick of 64 x 4 x 8 grid points and first projects the
//                                brick's eight corners (tsdf_brick_outside; pushed out by half a voxel, so that no rounding of the
//                                per-point arithmetic can disagree with the corners): a brick wholly behind the camera, wholly beside
//                                one side of the image, or -- with depth_max -- wholly beyond depth_max + trunc returns before it
//                                touches the volume.  Most of a room-sized volume is outside any one view.  Inside, consecutive lanes
//                                take consecutive x: a lane owns V grid points of a row (V = 4 where nx is a multiple of 4 and the five
//                                arrays start on 16 bytes, else 1) and gives them to tsdf_integrate_lane<V>, which looks its pixels up
//                                (a gather over five planes; neighbouring points share pixels, the vector cache serves them) and loads /
//                                stores the volume only where a point is updated: a row of a brick is 256 contiguous bytes per array.
//                                `skip` (device, the view camera's truncation status) gates the whole launch on the device
//                                (tsdf_view_skipped): nothing is read on the host per view.
//   T2 tsdf_triangles_kernel     one lane per cell, lanes along x: the eight corners' signs (and, where they differ, their weights);
//                                then tsdf_emit_cell: 0..12 triangles as three keys each, the slots of a wave reserved with one atomic.
//      tsdf_triangles_kernel<true>   the same pass by marching cubes (tsdf_math.h "SURFACE, cubes"): the same mask, the same seen rule,
//                                tsdf_emit_cell<true>: 0..5 triangles from the lane's row of the case table.
//   T3 tsdf_vertices_kernel      one lane per unique key: position and colour.
#include "tsdf_device.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
constexpr int kBrickX = 64, kBrickY = 4, kBrickZ = 8;

bool aligned16(const SplatTsdfVolume &v) {
    return (((uintptr_t)v.tsdf | (uintptr_t)v.weight | (uintptr_t)v.r | (uintptr_t)v.g | (uintptr_t)v.b) & 15) == 0;
}

// ---------------------------------------------------------------------------------------------------------------- T0
template <int V>
__global__ void __launch_bounds__(kBlock) tsdf_reset_kernel(TsdfArrays a, long long items) {      // items of V floats
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < items; i += stride) {
        if constexpr (V == 4) {
            const float4 one = make_float4(1.f, 1.f, 1.f, 1.f), zero = make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4 *>(a.tsdf)[i] = one;
            reinterpret_cast<float4 *>(a.weight)[i] = zero;
            reinterpret_cast<float4 *>(a.r)[i] = zero;
            reinterpret_cast<float4 *>(a.g)[i] = zero;
            reinterpret_cast<float4 *>(a.b)[i] = zero;
        } else {
            a.tsdf[i] = 1.f;
            a.weight[i] = a.r[i] = a.g[i] = a.b[i] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- T1
struct IntegrateArgs {
    TsdfGrid grid;
    TsdfArrays vol;
    TsdfCamera cam;
    const float *out6, *w2c;
    const int32_t *skip;
    int32_t *skipped;
    int bx, by, bz;                 // bricks per axis
};

template <int V>
__global__ void __launch_bounds__(kBlock) tsdf_integrate_kernel(IntegrateArgs a) {
    if (tsdf_view_skipped(a.skip, a.skipped)) return;
    const TsdfCamera cam = tsdf_view_camera(a.cam, a.w2c);
    constexpr int kLanesX = kBrickX / V;                            // lanes along a brick's row
    constexpr int kRowsPerPass = kBlock / kLanesX;                  // rows (y, z) of the brick taken at once
    constexpr int kPasses = kBrickY * kBrickZ / kRowsPerPass;
    const TsdfGrid &g = a.grid;
    const long long bricks = (long long)a.bx * a.by * a.bz;
    for (long long brick = blockIdx.x; brick < bricks; brick += gridDim.x) {         // (uniform bounds: tsdf_brick_outside)
        const int i0 = (int)(brick % a.bx) * kBrickX, j0 = (int)((brick / a.bx) % a.by) * kBrickY, k0 = (int)(brick / ((long long)a.bx * a.by)) * kBrickZ;
        if (tsdf_brick_outside(g, cam, i0, min(i0 + kBrickX, g.nx) - 1, j0, min(j0 + kBrickY, g.ny) - 1, k0, min(k0 + kBrickZ, g.nz) - 1)) continue;
        const int i = i0 + (int)(threadIdx.x % kLanesX) * V;
        if (i >= g.nx) continue;                                    // (V = 4: nx is a multiple of 4, so a lane's four points are inside together)
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const int row = pass * kRowsPerPass + (int)(threadIdx.x / kLanesX);
            const int j = j0 + (row % kBrickY), k = k0 + (row / kBrickY);
            if (j >= g.ny || k >= g.nz) continue;
            tsdf_integrate_lane<V>(g, cam, a.out6, a.vol, i, j, k, (size_t)tsdf_linear(g, i, j, k));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- T2
struct TrianglesArgs {
    TsdfGrid grid;
    const float *tsdf, *weight;
    float min_weight;
    int64_t *keys;
    long long capacity;
    unsigned long long *count;
    int bx, by;                     // blocks of 64 x 4 cells per axis (z: one layer per block)
    long long blocks;
};

template <bool kCubes>
__global__ void __launch_bounds__(kBlock) tsdf_triangles_kernel(TrianglesArgs a) {
    const TsdfGrid &g = a.grid;
    const int lane = lane_id();
    for (long long blk = blockIdx.x; blk < a.blocks; blk += gridDim.x) {        // (uniform bounds: tsdf_emit_cell)
        const int i = (int)(blk % a.bx) * 64 + lane, j = (int)((blk / a.bx) % a.by) * 4 + (int)(threadIdx.x / kWave);
        const int k = (int)(blk / ((long long)a.bx * a.by));
        int mask = 0;
        if (i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1) {
            float f8[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) f8[c] = a.tsdf[tsdf_linear(g, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))];
            mask = tsdf_cell_mask(f8);
            if (mask != 0 && mask != 255) {                                     // (the weights only where the signs differ: most cells need none)
                bool seen = true;
#pragma unroll
                for (int c = 0; c < 8; ++c) seen &= a.weight[tsdf_linear(g, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))] >= a.min_weight;
                if (!seen) mask = 0;
            }
        }
        tsdf_emit_cell<kCubes>(g, i, j, k, mask, a.keys, (unsigned long long)a.capacity, a.count);
    }
}

// ---------------------------------------------------------------------------------------------------------------- T3
__global__ void __launch_bounds__(kBlock) tsdf_vertices_kernel(TsdfGrid g, TsdfArrays vol, const int64_t *keys, long long n, float *vertices,
                                                               float *colors) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += stride) {
        float pos[3], col[3];
        tsdf_vertex(g, keys[v], vol.tsdf, vol.r, vol.g, vol.b, pos, col);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            vertices[3 * v + c] = pos[c];
            if (colors) colors[3 * v + c] = col[c];
        }
    }
}

}  // namespace

hipError_t launch_tsdf_reset(const SplatTsdfVolume &v, hipStream_t s) {
    const long long n = (long long)v.nx * v.ny * v.nz;
    const bool vec = n % 4 == 0 && aligned16(v);
    const long long items = vec ? n / 4 : n;
    const unsigned grid = tsdf_grid_for((items + kBlock - 1) / kBlock);
    if (vec) hipLaunchKernelGGL(tsdf_reset_kernel<4>, dim3(grid), dim3(kBlock), 0, s, tsdf_arrays_of(v), items);
    else hipLaunchKernelGGL(tsdf_reset_kernel<1>, dim3(grid), dim3(kBlock), 0, s, tsdf_arrays_of(v), items);
    return hipGetLastError();
}

hipError_t launch_tsdf_integrate(const SplatTsdfVolume &v, const SplatTsdfView &w, hipStream_t s) {
    IntegrateArgs a;
    a.grid = tsdf_grid_of(v);
    a.vol = tsdf_arrays_of(v);
    a.cam = tsdf_camera_of(v, w);
    a.out6 = w.out6; a.w2c = w.w2c; a.skip = w.skip; a.skipped = w.skipped;
    a.bx = (v.nx + kBrickX - 1) / kBrickX; a.by = (v.ny + kBrickY - 1) / kBrickY; a.bz = (v.nz + kBrickZ - 1) / kBrickZ;
    const unsigned grid = tsdf_grid_for((long long)a.bx * a.by * a.bz);
    if (v.nx % 4 == 0 && aligned16(v)) hipLaunchKernelGGL(tsdf_integrate_kernel<4>, dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(tsdf_integrate_kernel<1>, dim3(grid), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tsdf_triangles(const SplatTsdfVolume &v, float min_weight, int64_t *keys, long long capacity, int64_t *count, bool cubes,
                                 hipStream_t s) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    if (v.nx < 2 || v.ny < 2 || v.nz < 2) return hipSuccess;        // no cell
    TrianglesArgs a;
    a.grid = tsdf_grid_of(v);
    a.tsdf = v.tsdf; a.weight = v.weight; a.min_weight = min_weight;
    a.keys = keys; a.capacity = capacity; a.count = reinterpret_cast<unsigned long long *>(count);
    a.bx = (v.nx - 1 + 63) / 64; a.by = (v.ny - 1 + 3) / 4;
    a.blocks = (long long)a.bx * a.by * (v.nz - 1);
    if (cubes) hipLaunchKernelGGL(tsdf_triangles_kernel<true>, dim3(tsdf_grid_for(a.blocks)), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(tsdf_triangles_kernel<false>, dim3(tsdf_grid_for(a.blocks)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tsdf_vertices(const SplatTsdfVolume &v, const int64_t *keys, long long n, float *vertices, float *colors, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tsdf_vertices_kernel, dim3(tsdf_grid_for((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tsdf_grid_of(v), tsdf_arrays_of(v), keys, n,
                       vertices, colors);
    return hipGetLastError();
}

}  // namespace splat
