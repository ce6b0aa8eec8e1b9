// tsdf_sparse.hip -- the mesh layer on a SPARSE volume: the virtual grid of tsdf.hip, of which only the bricks near observed surfaces
// are stored (tsdf_math.h, "sparse volume": 2048 grid points per brick, 8 KiB contiguous per array in a pool, a directory of slots
// over all bricks).  The arithmetic per grid point, cell and vertex is the dense kernels', call for call, so a sparse volume whose
// bricks cover tsdf_mark_box of every pixel of every view, and that was then given every view, yields the dense volume's mesh bit
// for bit.
//
//   S1 tsdf_mark_kernel              one lane per pixel: tsdf_mark_box, then a plain store of 1 into the flag of every brick the box
//                                    meets (every writer stores the same value: no atomics).  Gated by `skip` as T1 is.
//      allocation                    is the caller's (a prefix sum over the flags on the device); new slots are reset by T0 over the
//                                    slot range (launch_tsdf_sparse_reset_slots).
//   S2 tsdf_sparse_integrate_kernel  one workgroup per allocated brick (brick_of_slot): T1's eight-corner frustum test on the brick's
//                                    box, then T1's per-point body on the brick's 2048 points, four per lane (a brick row is a
//                                    multiple of four points and a brick starts on 8 KiB: always 16-byte accesses), points at or
//                                    beyond nx, ny, nz masked.
//   S3 tsdf_sparse_triangles_kernel  one workgroup per allocated brick, lanes over the cells whose corner 0 is in the brick; corners
//                                    in the +x, +y, +z neighbour bricks come through the directory (the eight slots a brick's cells
//                                    can touch are looked up once per workgroup), a missing neighbour makes the cell unseen.  T2's
//                                    reservation: scan, one returning atomic by the last lane, readlane.
//      tsdf_sparse_triangles_kernel<true>  the same pass by marching cubes, as T2's (tsdf.hip): the lane's row of the case table in four
//                                    registers, its five slots unrolled and predicated.
//   S4 tsdf_sparse_vertices_kernel   one lane per unique key, the edge's two grid points through the directory.
#include "splat_device.h"
#include "tsdf_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
constexpr long long kMaxGrid = 1ll << 30;

struct SparseArrays {
    float *tsdf, *weight, *r, *g, *b;
    const int32_t *directory, *brick_of_slot;
    int slots;
};

TsdfGrid grid_of(const SplatTsdfSparse &v) {
    TsdfGrid g;
    g.nx = v.nx; g.ny = v.ny; g.nz = v.nz;
    g.ox = v.origin[0]; g.oy = v.origin[1]; g.oz = v.origin[2]; g.voxel = v.voxel;
    return g;
}
int log2_of(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
TsdfBricks bricks_of(const SplatTsdfSparse &v) { return tsdf_bricks(grid_of(v), log2_of(v.brick[0]), log2_of(v.brick[1]), log2_of(v.brick[2])); }
SparseArrays arrays_of(const SplatTsdfSparse &v) { return SparseArrays{v.tsdf, v.weight, v.r, v.g, v.b, v.directory, v.brick_of_slot, v.slots}; }
TsdfCamera camera_of(const SplatTsdfSparse &v, const SplatTsdfView &w) {
    TsdfCamera c;
    c.W = w.width; c.H = w.height;
    c.fx = w.fx; c.fy = w.fy; c.cx = w.cx; c.cy = w.cy;
    c.trunc = v.trunc; c.sil_thres = w.sil_thres; c.depth_max = w.depth_max; c.weight_max = w.weight_max;
    for (int q = 0; q < 12; ++q) c.m[q] = 0.f;              // (filled in the kernel, from w2c)
    return c;
}
unsigned grid_for(long long blocks) { return (unsigned)(blocks < 1 ? 1 : (blocks > kMaxGrid ? kMaxGrid : blocks)); }

// ---------------------------------------------------------------------------------------------------------------- S1
struct MarkArgs {
    TsdfGrid grid;
    TsdfBricks bricks;
    TsdfCamera cam;
    const float *out6, *w2c;
    const int32_t *skip;
    int32_t *skipped;
    int32_t *flags;                 // [bricks]
};

__global__ void __launch_bounds__(kBlock) tsdf_mark_kernel(MarkArgs a) {
    if (a.skip && *a.skip != 0) {                                   // the view's lists did not fit: its planes are incomplete
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.skipped, 1);
        return;
    }
    TsdfCamera cam = a.cam;
#pragma unroll
    for (int q = 0; q < 12; ++q) cam.m[q] = a.w2c[q];
    const size_t plane = (size_t)cam.W * cam.H;
    const TsdfBricks &b = a.bricks;
    for (size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x; px < plane; px += (size_t)gridDim.x * kBlock) {
        int lo[3], hi[3];
        if (!tsdf_mark_box(a.grid, cam, (int)(px % cam.W), (int)(px / cam.W), a.out6[4 * plane + px], a.out6[3 * plane + px], lo, hi)) continue;
        // (the box is clipped to the grid, so every brick index below is inside the directory)
        for (int bk = lo[2] >> b.lz; bk <= hi[2] >> b.lz; ++bk)
            for (int bj = lo[1] >> b.ly; bj <= hi[1] >> b.ly; ++bj)
                for (int bi = lo[0] >> b.lx; bi <= hi[0] >> b.lx; ++bi) a.flags[((long long)bk * b.by + bj) * b.bx + bi] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- S2
struct SparseIntegrateArgs {
    TsdfGrid grid;
    TsdfBricks bricks;
    SparseArrays vol;
    TsdfCamera cam;
    const float *out6, *w2c;
    const int32_t *skip;
    int32_t *skipped;
};

// T1's test (tsdf.hip brick_outside) on a brick of this file's shape: the brick's box, pushed out by half a voxel, against the planes
// every updated point satisfies; lane l of a wave projects corner l mod 8 and six ballots combine them.
__device__ __forceinline__ bool sparse_brick_outside(const TsdfGrid &g, const TsdfBricks &b, const TsdfCamera &cam, int i0, int j0, int k0) {
    const int c = threadIdx.x & 7;
    const int i1 = min(i0 + (1 << b.lx), g.nx) - 1, j1 = min(j0 + (1 << b.ly), g.ny) - 1, k1 = min(k0 + (1 << b.lz), g.nz) - 1;
    const float p[3] = {g.ox + g.voxel * ((c & 1) ? (float)i1 + 0.5f : (float)i0 - 0.5f),
                        g.oy + g.voxel * ((c & 2) ? (float)j1 + 0.5f : (float)j0 - 0.5f),
                        g.oz + g.voxel * ((c & 4) ? (float)k1 + 0.5f : (float)k0 - 0.5f)};
    const float *m = cam.m;
    const float ax = cam.cx + 0.5f, ay = cam.cy + 0.5f, far_z = cam.depth_max + cam.trunc;
    const float x = m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3];
    const float y = m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7];
    const float z = m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11];
    bool outside = (__builtin_amdgcn_ballot_w64(!(z > 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fx * x + ax * z >= 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fx * x + (ax - (float)cam.W) * z < 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fy * y + ay * z >= 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fy * y + (ay - (float)cam.H) * z < 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(cam.depth_max > 0.f && z > far_z) & 0xffull) == 0xffull;
    return outside;
}

__global__ void __launch_bounds__(kBlock) tsdf_sparse_integrate_kernel(SparseIntegrateArgs a) {
    if (a.skip && *a.skip != 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.skipped, 1);
        return;
    }
    TsdfCamera cam = a.cam;
#pragma unroll
    for (int q = 0; q < 12; ++q) cam.m[q] = a.w2c[q];
    constexpr int V = 4, kPasses = kTsdfBrickPoints / (kBlock * V);
    const TsdfGrid &g = a.grid;
    const TsdfBricks &b = a.bricks;
    const size_t plane = (size_t)cam.W * cam.H;
    for (int slot = blockIdx.x; slot < a.vol.slots; slot += gridDim.x) {
        int i0, j0, k0;
        tsdf_brick_origin(b, a.vol.brick_of_slot[slot], i0, j0, k0);
        if (sparse_brick_outside(g, b, cam, i0, j0, k0)) continue;
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const int local = (pass * kBlock + (int)threadIdx.x) * V;
            int li, lj, lk;
            tsdf_brick_unlocal(b, local, li, lj, lk);
            const int i = i0 + li, j = j0 + lj, k = k0 + lk;
            if (i >= g.nx || j >= g.ny || k >= g.nz) continue;
            // T1's three rounds of independent loads; a point at or beyond nx is never hit
            float z[V], s[V], dep[V], f[V], rgb[V][3];
            size_t px[V];
            bool hit[V], any = false;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float p[3];
                tsdf_point(g, i + v, j, k, p);
                hit[v] = i + v < g.nx && tsdf_project(cam, p, z[v], px[v]);
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
            const size_t o = (size_t)slot * kTsdfBrickPoints + local;
            float4 q[5] = {*reinterpret_cast<const float4 *>(a.vol.tsdf + o), *reinterpret_cast<const float4 *>(a.vol.weight + o),
                           *reinterpret_cast<const float4 *>(a.vol.r + o), *reinterpret_cast<const float4 *>(a.vol.g + o),
                           *reinterpret_cast<const float4 *>(a.vol.b + o)};
            float *t = &q[0].x, *w = &q[1].x, *r = &q[2].x, *gg = &q[3].x, *bb = &q[4].x;
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (hit[v]) tsdf_blend(f[v], rgb[v], cam.weight_max, t[v], w[v], r[v], gg[v], bb[v]);
            *reinterpret_cast<float4 *>(a.vol.tsdf + o) = q[0];
            *reinterpret_cast<float4 *>(a.vol.weight + o) = q[1];
            *reinterpret_cast<float4 *>(a.vol.r + o) = q[2];
            *reinterpret_cast<float4 *>(a.vol.g + o) = q[3];
            *reinterpret_cast<float4 *>(a.vol.b + o) = q[4];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- S3
struct SparseTrianglesArgs {
    TsdfGrid grid;
    TsdfBricks bricks;
    SparseArrays vol;
    float min_weight;
    int64_t *keys;
    long long capacity;
    unsigned long long *count;
};

template <bool kCubes>
__global__ void __launch_bounds__(kBlock) tsdf_sparse_triangles_kernel(SparseTrianglesArgs a) {
    __shared__ int nb[8];                                           // slots of the brick and its +x, +y, +z neighbours (dx + 2 dy + 4 dz), -1 = none
    const TsdfGrid &g = a.grid;
    const TsdfBricks &b = a.bricks;
    const int lane = threadIdx.x & (kWave - 1);
    const int mx = (1 << b.lx) - 1, my = (1 << b.ly) - 1, mz = (1 << b.lz) - 1;
    for (int slot = blockIdx.x; slot < a.vol.slots; slot += gridDim.x) {       // (uniform bounds: every lane of a wave reaches the scan)
        const long long brick = a.vol.brick_of_slot[slot];
        if (brick < 0 || brick >= tsdf_brick_count(b)) continue;    // (not a brick of this grid; uniform over the workgroup)
        int i0, j0, k0;
        tsdf_brick_origin(b, brick, i0, j0, k0);
        __syncthreads();                                            // (the previous brick's readers are done with nb)
        if (threadIdx.x < 8) {
            const int c = threadIdx.x;
            const int bi = (i0 >> b.lx) + (c & 1), bj = (j0 >> b.ly) + ((c >> 1) & 1), bk = (k0 >> b.lz) + ((c >> 2) & 1);
            const int s = (bi < b.bx && bj < b.by && bk < b.bz) ? a.vol.directory[((long long)bk * b.by + bj) * b.bx + bi] : -1;
            nb[c] = s < a.vol.slots ? s : -1;                       // (a slot beyond the pool is no slot)
        }
        __syncthreads();
#pragma unroll 1
        for (int pass = 0; pass < kTsdfBrickPoints / kBlock; ++pass) {
            int li, lj, lk;
            tsdf_brick_unlocal(b, pass * kBlock + (int)threadIdx.x, li, lj, lk);
            const int i = i0 + li, j = j0 + lj, k = k0 + lk;
            int mask = 0;
            if (i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1) {
                size_t at[8];                                       // the corners' offsets in the pool
                bool have = true;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int ci = li + (c & 1), cj = lj + ((c >> 1) & 1), ck = lk + ((c >> 2) & 1);
                    const int s = nb[(ci >> b.lx) | ((cj >> b.ly) << 1) | ((ck >> b.lz) << 2)];
                    have &= s >= 0;
                    at[c] = (size_t)(s < 0 ? 0 : s) * kTsdfBrickPoints + (size_t)(((((ck & mz) << b.ly) | (cj & my)) << b.lx) | (ci & mx));
                }
                if (have) {                                         // (a missing neighbour: the cell is unseen, as in the dense volume)
                    float f8[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) f8[c] = a.vol.tsdf[at[c]];
                    mask = tsdf_cell_mask(f8);
                    if (mask != 0 && mask != 255) {
                        bool seen = true;
#pragma unroll
                        for (int c = 0; c < 8; ++c) seen &= a.vol.weight[at[c]] >= a.min_weight;
                        if (!seen) mask = 0;
                    }
                }
            }
            TsdfCubesRow cubes;                                                 // (row 0 of the table is empty: an idle lane's)
            if constexpr (kCubes) cubes = tsdf_cubes_row(mask);
            const unsigned n = kCubes ? (unsigned)tsdf_cubes_row_entry(cubes, 0) : (unsigned)tsdf_cell_triangles(mask);
            if (__builtin_amdgcn_ballot_w64(n != 0) == 0ull) continue;          // (wave-uniform)
            const unsigned incl = wave_scan_incl_u32(n);
            unsigned long long base = 0;
            if (lane == kWave - 1) base = atomicAdd(a.count, (unsigned long long)incl);
            base = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(base >> 32), kWave - 1) << 32)
                   | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)base, kWave - 1);
            if (n == 0) continue;
            unsigned long long out = base + (incl - n);
            if constexpr (kCubes) {
                tsdf_cubes_store(g, i, j, k, cubes, out, (unsigned long long)a.capacity, a.keys);
                continue;
            }
#pragma unroll 1
            for (int q = 0; q < 6; ++q) {
                const int8_t *row = kTsdfTetCases[tsdf_tet_mask(mask, q)];
                for (int t = 0; t < row[0]; ++t, ++out) {
                    if (out >= (unsigned long long)a.capacity) continue;
                    int64_t key[3];
                    tsdf_tet_triangle(g, i, j, k, q, row, t, key);
                    a.keys[3 * out] = key[0];
                    a.keys[3 * out + 1] = key[1];
                    a.keys[3 * out + 2] = key[2];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- S4
// the five values of grid point (i, j, k); the reset values where its brick is not allocated (no key S3 emits names such a point)
__device__ __forceinline__ void sparse_fetch(const TsdfBricks &b, const SparseArrays &vol, int i, int j, int k, float *v5) {
    const int s = vol.directory[tsdf_brick_of(b, i, j, k)];
    if (s < 0 || s >= vol.slots) {
        v5[0] = 1.f;
        v5[1] = v5[2] = v5[3] = v5[4] = 0.f;
        return;
    }
    const size_t o = (size_t)s * kTsdfBrickPoints + tsdf_brick_local(b, i, j, k);
    v5[0] = vol.tsdf[o]; v5[1] = vol.weight[o]; v5[2] = vol.r[o]; v5[3] = vol.g[o]; v5[4] = vol.b[o];
}

__global__ void __launch_bounds__(kBlock) tsdf_sparse_vertices_kernel(TsdfGrid g, TsdfBricks b, SparseArrays vol, const int64_t *keys, long long n,
                                                                      long long points, float *vertices, float *colors) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += stride) {
        const int64_t key = keys[v];
        const int dir = (int)(key & 7);
        int i, j, k;
        tsdf_unlinear(g, key >> 3, i, j, k);
        const int ib = i + (dir & 1), jb = j + ((dir >> 1) & 1), kb = k + ((dir >> 2) & 1);
        float pos[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
        if (key >= 0 && (key >> 3) < points && ib < g.nx && jb < g.ny && kb < g.nz) {      // (a key outside the grid: zeros, nothing read)
            float va[5], vb[5];
            sparse_fetch(b, vol, i, j, k, va);
            sparse_fetch(b, vol, ib, jb, kb, vb);
            tsdf_vertex_values(g, key, va, vb, pos, col);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            vertices[3 * v + c] = pos[c];
            if (colors) colors[3 * v + c] = col[c];
        }
    }
}

}  // namespace

hipError_t launch_tsdf_sparse_mark(const SplatTsdfSparse &v, const SplatTsdfView &w, int32_t *flags, hipStream_t s) {
    MarkArgs a;
    a.grid = grid_of(v);
    a.bricks = bricks_of(v);
    a.cam = camera_of(v, w);
    a.out6 = w.out6; a.w2c = w.w2c; a.skip = w.skip; a.skipped = w.skipped; a.flags = flags;
    const long long pixels = (long long)w.width * w.height;
    hipLaunchKernelGGL(tsdf_mark_kernel, dim3(grid_for((pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// T0 over the pool's slots [first, first + count): the five arrays of a slot range are contiguous, 8 KiB-aligned runs of floats
hipError_t launch_tsdf_sparse_reset_slots(const SplatTsdfSparse &v, long long first, long long count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    SplatTsdfVolume run;
    run.nx = kTsdfBrickPoints; run.ny = (int32_t)count; run.nz = 1;       // (T0 forms nx ny nz in 64 bits; count is below 2^31)
    run.origin[0] = run.origin[1] = run.origin[2] = 0.f;
    run.voxel = v.voxel; run.trunc = v.trunc;
    const size_t o = (size_t)first * kTsdfBrickPoints;
    run.tsdf = v.tsdf + o; run.weight = v.weight + o; run.r = v.r + o; run.g = v.g + o; run.b = v.b + o;
    return launch_tsdf_reset(run, s);
}

hipError_t launch_tsdf_sparse_integrate(const SplatTsdfSparse &v, const SplatTsdfView &w, hipStream_t s) {
    SparseIntegrateArgs a;
    a.grid = grid_of(v);
    a.bricks = bricks_of(v);
    a.vol = arrays_of(v);
    a.cam = camera_of(v, w);
    a.out6 = w.out6; a.w2c = w.w2c; a.skip = w.skip; a.skipped = w.skipped;
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel, dim3(grid_for(v.slots)), dim3(kBlock), 0, s, a);      // (one block even without slots: `skip` is counted)
    return hipGetLastError();
}

hipError_t launch_tsdf_sparse_triangles(const SplatTsdfSparse &v, float min_weight, int64_t *keys, long long capacity, int64_t *count, bool cubes,
                                        hipStream_t s) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    if (v.nx < 2 || v.ny < 2 || v.nz < 2 || v.slots == 0) return hipSuccess;       // no cell
    SparseTrianglesArgs a;
    a.grid = grid_of(v);
    a.bricks = bricks_of(v);
    a.vol = arrays_of(v);
    a.min_weight = min_weight;
    a.keys = keys; a.capacity = capacity; a.count = reinterpret_cast<unsigned long long *>(count);
    if (cubes) hipLaunchKernelGGL(tsdf_sparse_triangles_kernel<true>, dim3(grid_for(v.slots)), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(tsdf_sparse_triangles_kernel<false>, dim3(grid_for(v.slots)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tsdf_sparse_vertices(const SplatTsdfSparse &v, const int64_t *keys, long long n, float *vertices, float *colors, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tsdf_sparse_vertices_kernel, dim3(grid_for((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, grid_of(v), bricks_of(v),
                       arrays_of(v), keys, n, (long long)v.nx * v.ny * v.nz, vertices, colors);
    return hipGetLastError();
}

}  // namespace splat
