// tsdf.hip -- the mesh layer: rendered depth fused into a truncated signed distance volume, and the volume's zero surface as a
// triangle mesh.  The arithmetic is tsdf_math.h's.
//
//   T0 tsdf_reset_kernel<V>      tsdf = 1, weight = r = g = b = 0: V floats per lane and array (16-byte stores where the arrays allow).
//   T1 tsdf_integrate_kernel<V>  one launch per view.  A workgroup owns a brick of 64 x 4 x 8 grid points and first projects the
//                                brick's eight corners (pushed out by half a voxel, so that no rounding of the per-point arithmetic can
//                                disagree with the corners): a brick wholly behind the camera, wholly beside one side of the image, or
//                                -- with depth_max -- wholly beyond depth_max + trunc returns before it touches the volume.  Most of a
//                                room-sized volume is outside any one view.  Inside, consecutive lanes take consecutive x: a lane
//                                owns V grid points of a row (V = 4 where nx is a multiple of 4 and the five arrays start on 16 bytes,
//                                else 1), looks its pixels up (a gather over five planes; neighbouring points share pixels, the vector
//                                cache serves them) and loads / stores the volume only where a point is updated: a row of a brick is
//                                256 contiguous bytes per array.  `skip` (device, the view camera's truncation status) gates the
//                                whole launch on the device: nothing is read on the host per view.
//   T2 tsdf_triangles_kernel     one lane per cell, lanes along x: the eight corners' signs (and, where they differ, their weights),
//                                0..12 triangles as three keys each.  A wave reserves the slots of all its lanes with ONE returning atomic (prefix sum over the
//                                lanes' counts, the last lane adds the total, every lane reads the base): the group-binning
//                                reservation's idiom.  count[0] gets what is wanted; nothing is written at or beyond `capacity`.
//      tsdf_triangles_kernel<true>   the same pass by marching cubes (tsdf_math.h "SURFACE, cubes"): the same mask, the same seen rule, the
//                                same reservation; 0..5 triangles from the lane's 16-byte row of the case table, held in four
//                                registers, the five slots unrolled and predicated on the count (no loop over a lane's own bound).
//   T3 tsdf_vertices_kernel      one lane per unique key: position and colour.
#include "splat_device.h"
#include "tsdf_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
constexpr int kBrickX = 64, kBrickY = 4, kBrickZ = 8;
constexpr long long kMaxGrid = 1ll << 30;

struct TsdfArrays {
    float *tsdf, *weight, *r, *g, *b;
};

TsdfGrid grid_of(const SplatTsdfVolume &v) {
    TsdfGrid g;
    g.nx = v.nx; g.ny = v.ny; g.nz = v.nz;
    g.ox = v.origin[0]; g.oy = v.origin[1]; g.oz = v.origin[2]; g.voxel = v.voxel;
    return g;
}
TsdfArrays arrays_of(const SplatTsdfVolume &v) { return TsdfArrays{v.tsdf, v.weight, v.r, v.g, v.b}; }
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
    TsdfCamera cam;                 // (m is filled in the kernel, from w2c)
    const float *out6, *w2c;
    const int32_t *skip;
    int32_t *skipped;
    int bx, by, bz;                 // bricks per axis
};

// The brick's box, pushed out by half a voxel, against the planes every updated point satisfies: z > 0; 0 <= u + 0.5 < W and
// 0 <= v + 0.5 < H, which for z > 0 are fx x + (cx + 0.5) z >= 0 and fx x + (cx + 0.5 - W) z < 0 (y likewise); z <= depth_max + trunc.
// Each is linear in p, so a box whose eight corners all fail one of them holds no point that passes.  Plain float arithmetic: the
// half voxel of margin is orders of magnitude beyond its rounding.  Lane l of a wave projects corner l mod 8 and six ballots combine
// them (every lane of the workgroup is here: the brick loop's bounds are uniform), so the test costs a wave one corner, not eight.
__device__ __forceinline__ bool brick_outside(const IntegrateArgs &a, const float *m, int i0, int j0, int k0) {
    const TsdfGrid &g = a.grid;
    const int c = threadIdx.x & 7;
    const int i1 = min(i0 + kBrickX, g.nx) - 1, j1 = min(j0 + kBrickY, g.ny) - 1, k1 = min(k0 + kBrickZ, g.nz) - 1;
    const float p[3] = {g.ox + g.voxel * ((c & 1) ? (float)i1 + 0.5f : (float)i0 - 0.5f),
                        g.oy + g.voxel * ((c & 2) ? (float)j1 + 0.5f : (float)j0 - 0.5f),
                        g.oz + g.voxel * ((c & 4) ? (float)k1 + 0.5f : (float)k0 - 0.5f)};
    const float ax = a.cam.cx + 0.5f, ay = a.cam.cy + 0.5f, far_z = a.cam.depth_max + a.cam.trunc;
    const float x = m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3];
    const float y = m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7];
    const float z = m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11];
    // a plane is failed by the brick when the ballot of its eight corners (lanes 0..7; the other lanes repeat them) is full
    bool outside = (__builtin_amdgcn_ballot_w64(!(z > 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(a.cam.fx * x + ax * z >= 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(a.cam.fx * x + (ax - (float)a.cam.W) * z < 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(a.cam.fy * y + ay * z >= 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(a.cam.fy * y + (ay - (float)a.cam.H) * z < 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(a.cam.depth_max > 0.f && z > far_z) & 0xffull) == 0xffull;
    return outside;
}

template <int V>
__global__ void __launch_bounds__(kBlock) tsdf_integrate_kernel(IntegrateArgs a) {
    if (a.skip && *a.skip != 0) {                                   // the view's lists did not fit: its planes are incomplete
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.skipped, 1);
        return;
    }
    TsdfCamera cam = a.cam;
#pragma unroll
    for (int q = 0; q < 12; ++q) cam.m[q] = a.w2c[q];
    constexpr int kLanesX = kBrickX / V;                            // lanes along a brick's row
    constexpr int kRowsPerPass = kBlock / kLanesX;                  // rows (y, z) of the brick taken at once
    constexpr int kPasses = kBrickY * kBrickZ / kRowsPerPass;
    const TsdfGrid &g = a.grid;
    const size_t plane = (size_t)cam.W * cam.H;
    const long long bricks = (long long)a.bx * a.by * a.bz;
    for (long long brick = blockIdx.x; brick < bricks; brick += gridDim.x) {
        const int i0 = (int)(brick % a.bx) * kBrickX, j0 = (int)((brick / a.bx) % a.by) * kBrickY, k0 = (int)(brick / ((long long)a.bx * a.by)) * kBrickZ;
        if (brick_outside(a, cam.m, i0, j0, k0)) continue;
        const int i = i0 + (int)(threadIdx.x % kLanesX) * V;
        if (i >= g.nx) continue;                                    // (V = 4: nx is a multiple of 4, so a lane's four points are inside together)
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const int row = pass * kRowsPerPass + (int)(threadIdx.x / kLanesX);
            const int j = j0 + (row % kBrickY), k = k0 + (row / kBrickY);
            if (j >= g.ny || k >= g.nz) continue;
            // the lane's V points in three rounds of independent loads (a chain of dependent gathers per point is what this kernel
            // would otherwise wait for): pixel offsets; silhouette and depth of all V; colours and the volume where a point is hit
            float z[V], s[V], dep[V], f[V], rgb[V][3];
            size_t px[V];
            bool hit[V], any = false;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float p[3];
                tsdf_point(g, i + v, j, k, p);
                hit[v] = tsdf_project(cam, p, z[v], px[v]);
                if (!hit[v]) px[v] = 0;
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                s[v] = hit[v] ? a.out6[4 * plane + px[v]] : 0.f;
                dep[v] = hit[v] ? a.out6[3 * plane + px[v]] : 0.f;
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                hit[v] = hit[v] && tsdf_measure(cam, s[v], dep[v], z[v], f[v]);
                any |= hit[v];
            }
            if (!any) continue;
#pragma unroll
            for (int v = 0; v < V; ++v)
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[v][c] = hit[v] ? tsdf_colour(a.out6[c * plane + px[v]], s[v]) : 0.f;
            const long long o = tsdf_linear(g, i, j, k);
            if constexpr (V == 4) {
                float4 q[5] = {*reinterpret_cast<const float4 *>(a.vol.tsdf + o), *reinterpret_cast<const float4 *>(a.vol.weight + o),
                               *reinterpret_cast<const float4 *>(a.vol.r + o), *reinterpret_cast<const float4 *>(a.vol.g + o),
                               *reinterpret_cast<const float4 *>(a.vol.b + o)};
                float *t = &q[0].x, *w = &q[1].x, *r = &q[2].x, *gg = &q[3].x, *b = &q[4].x;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (hit[v]) tsdf_blend(f[v], rgb[v], cam.weight_max, t[v], w[v], r[v], gg[v], b[v]);
                *reinterpret_cast<float4 *>(a.vol.tsdf + o) = q[0];
                *reinterpret_cast<float4 *>(a.vol.weight + o) = q[1];
                *reinterpret_cast<float4 *>(a.vol.r + o) = q[2];
                *reinterpret_cast<float4 *>(a.vol.g + o) = q[3];
                *reinterpret_cast<float4 *>(a.vol.b + o) = q[4];
            } else {
                float t = a.vol.tsdf[o], w = a.vol.weight[o], r = a.vol.r[o], gg = a.vol.g[o], b = a.vol.b[o];
                tsdf_blend(f[0], rgb[0], cam.weight_max, t, w, r, gg, b);
                a.vol.tsdf[o] = t; a.vol.weight[o] = w; a.vol.r[o] = r; a.vol.g[o] = gg; a.vol.b[o] = b;
            }
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
    const int lane = threadIdx.x & (kWave - 1);
    for (long long blk = blockIdx.x; blk < a.blocks; blk += gridDim.x) {        // (uniform bounds: every lane of a wave reaches the scan)
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
        TsdfCubesRow cubes;                                                     // (row 0 of the table is empty: an idle lane's)
        if constexpr (kCubes) cubes = tsdf_cubes_row(mask);
        const unsigned n = kCubes ? (unsigned)tsdf_cubes_row_entry(cubes, 0) : (unsigned)tsdf_cell_triangles(mask);
        if (__builtin_amdgcn_ballot_w64(n != 0) == 0ull) continue;              // (wave-uniform)
        const unsigned incl = wave_scan_incl_u32(n);
        unsigned long long base = 0;
        if (lane == kWave - 1) base = atomicAdd(a.count, (unsigned long long)incl);
        base = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(base >> 32), kWave - 1) << 32)
               | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)base, kWave - 1);
        if (n == 0) continue;
        unsigned long long slot = base + (incl - n);
        if constexpr (kCubes) {
            tsdf_cubes_store(g, i, j, k, cubes, slot, (unsigned long long)a.capacity, a.keys);
            continue;
        }
#pragma unroll 1
        for (int q = 0; q < 6; ++q) {
            const int8_t *row = kTsdfTetCases[tsdf_tet_mask(mask, q)];
            for (int t = 0; t < row[0]; ++t, ++slot) {
                if (slot >= (unsigned long long)a.capacity) continue;
                int64_t key[3];
                tsdf_tet_triangle(g, i, j, k, q, row, t, key);
                a.keys[3 * slot] = key[0];
                a.keys[3 * slot + 1] = key[1];
                a.keys[3 * slot + 2] = key[2];
            }
        }
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

unsigned grid_for(long long blocks) { return (unsigned)(blocks < 1 ? 1 : (blocks > kMaxGrid ? kMaxGrid : blocks)); }

}  // namespace

hipError_t launch_tsdf_reset(const SplatTsdfVolume &v, hipStream_t s) {
    const long long n = (long long)v.nx * v.ny * v.nz;
    const bool vec = n % 4 == 0 && aligned16(v);
    const long long items = vec ? n / 4 : n;
    const unsigned grid = grid_for((items + kBlock - 1) / kBlock);
    if (vec) hipLaunchKernelGGL(tsdf_reset_kernel<4>, dim3(grid), dim3(kBlock), 0, s, arrays_of(v), items);
    else hipLaunchKernelGGL(tsdf_reset_kernel<1>, dim3(grid), dim3(kBlock), 0, s, arrays_of(v), items);
    return hipGetLastError();
}

hipError_t launch_tsdf_integrate(const SplatTsdfVolume &v, const SplatTsdfView &w, hipStream_t s) {
    IntegrateArgs a;
    a.grid = grid_of(v);
    a.vol = arrays_of(v);
    a.cam.W = w.width; a.cam.H = w.height;
    a.cam.fx = w.fx; a.cam.fy = w.fy; a.cam.cx = w.cx; a.cam.cy = w.cy;
    a.cam.trunc = v.trunc; a.cam.sil_thres = w.sil_thres; a.cam.depth_max = w.depth_max; a.cam.weight_max = w.weight_max;
    for (int q = 0; q < 12; ++q) a.cam.m[q] = 0.f;
    a.out6 = w.out6; a.w2c = w.w2c; a.skip = w.skip; a.skipped = w.skipped;
    a.bx = (v.nx + kBrickX - 1) / kBrickX; a.by = (v.ny + kBrickY - 1) / kBrickY; a.bz = (v.nz + kBrickZ - 1) / kBrickZ;
    const unsigned grid = grid_for((long long)a.bx * a.by * a.bz);
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
    a.grid = grid_of(v);
    a.tsdf = v.tsdf; a.weight = v.weight; a.min_weight = min_weight;
    a.keys = keys; a.capacity = capacity; a.count = reinterpret_cast<unsigned long long *>(count);
    a.bx = (v.nx - 1 + 63) / 64; a.by = (v.ny - 1 + 3) / 4;
    a.blocks = (long long)a.bx * a.by * (v.nz - 1);
    if (cubes) hipLaunchKernelGGL(tsdf_triangles_kernel<true>, dim3(grid_for(a.blocks)), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(tsdf_triangles_kernel<false>, dim3(grid_for(a.blocks)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tsdf_vertices(const SplatTsdfVolume &v, const int64_t *keys, long long n, float *vertices, float *colors, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tsdf_vertices_kernel, dim3(grid_for((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, grid_of(v), arrays_of(v), keys, n,
                       vertices, colors);
    return hipGetLastError();
}

}  // namespace splat
