// tsdf_sparse.hip -- the mesh layer on a SPARSE volume: the virtual grid of tsdf.hip, of which only the bricks near observed surfaces
// are stored (tsdf_math.h, "sparse volume": 2048 grid points per brick, 8 KiB contiguous per array in a pool, a directory of slots
// over all bricks).  The arithmetic per grid point, cell and vertex is the dense kernels' -- tsdf_math.h's, through the very functions
// of tsdf_device.h that tsdf.hip calls --, so a sparse volume whose bricks cover tsdf_mark_box of every pixel of every view, and that
// was then given every view, yields the dense volume's mesh bit for bit.
//
//   S1 tsdf_mark_kernel              one lane per pixel: tsdf_mark_box, then a plain store of 1 into the flag of every brick the box
//                                    meets (every writer stores the same value: no atomics).  Gated by `skip` (tsdf_view_skipped).
//      allocation                    is the caller's (a prefix sum over the flags on the device); new slots are reset by T0 over the
//                                    slot range (launch_tsdf_sparse_reset_slots).
//   S2 tsdf_sparse_integrate_kernel  one workgroup per allocated brick (brick_of_slot): tsdf_brick_outside on the brick's box, then
//                                    tsdf_integrate_lane<4> on the brick's 2048 points, four per lane (a brick row is a multiple of
//                                    four points and a brick starts on 8 KiB: always 16-byte accesses), points at or beyond nx, ny,
//                                    nz masked.
//   S3 tsdf_sparse_triangles_kernel  one workgroup per allocated brick, lanes over the cells whose corner 0 is in the brick; corners
//                                    in the +x, +y, +z neighbour bricks come through the directory (the eight slots a brick's cells
//                                    can touch are looked up once per workgroup), a missing neighbour makes the cell unseen.  Then
//                                    tsdf_emit_cell, by marching tetrahedra or (<true>) marching cubes.
//   S4 tsdf_sparse_vertices_kernel   one lane per unique key, the edge's two grid points through the directory.
#include "tsdf_device.h"

namespace splat {
namespace {

constexpr int kBlock = 256;

struct SparseArrays : TsdfArrays {                          // (the pool's five arrays)
    const int32_t *directory, *brick_of_slot;
    int slots;
};

int log2_of(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
TsdfBricks bricks_of(const SplatTsdfSparse &v) { return tsdf_bricks(tsdf_grid_of(v), log2_of(v.brick[0]), log2_of(v.brick[1]), log2_of(v.brick[2])); }
SparseArrays arrays_of(const SplatTsdfSparse &v) { return SparseArrays{tsdf_arrays_of(v), v.directory, v.brick_of_slot, v.slots}; }

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
    if (tsdf_view_skipped(a.skip, a.skipped)) return;
    const TsdfCamera cam = tsdf_view_camera(a.cam, a.w2c);
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

__global__ void __launch_bounds__(kBlock) tsdf_sparse_integrate_kernel(SparseIntegrateArgs a) {
    if (tsdf_view_skipped(a.skip, a.skipped)) return;
    const TsdfCamera cam = tsdf_view_camera(a.cam, a.w2c);
    constexpr int V = 4, kPasses = kTsdfBrickPoints / (kBlock * V);
    const TsdfGrid &g = a.grid;
    const TsdfBricks &b = a.bricks;
    for (int slot = blockIdx.x; slot < a.vol.slots; slot += gridDim.x) {       // (uniform bounds: tsdf_brick_outside)
        int i0, j0, k0;
        tsdf_brick_origin(b, a.vol.brick_of_slot[slot], i0, j0, k0);
        if (tsdf_brick_outside(g, cam, i0, min(i0 + (1 << b.lx), g.nx) - 1, j0, min(j0 + (1 << b.ly), g.ny) - 1, k0, min(k0 + (1 << b.lz), g.nz) - 1)) continue;
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const int local = (pass * kBlock + (int)threadIdx.x) * V;
            int li, lj, lk;
            tsdf_brick_unlocal(b, local, li, lj, lk);
            const int i = i0 + li, j = j0 + lj, k = k0 + lk;
            if (i >= g.nx || j >= g.ny || k >= g.nz) continue;
            tsdf_integrate_lane<V>(g, cam, a.out6, a.vol, i, j, k, (size_t)slot * kTsdfBrickPoints + local);
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
    const int mx = (1 << b.lx) - 1, my = (1 << b.ly) - 1, mz = (1 << b.lz) - 1;
    for (int slot = blockIdx.x; slot < a.vol.slots; slot += gridDim.x) {       // (uniform bounds: tsdf_emit_cell)
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
            tsdf_emit_cell<kCubes>(g, i, j, k, mask, a.keys, (unsigned long long)a.capacity, a.count);
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
    a.grid = tsdf_grid_of(v);
    a.bricks = bricks_of(v);
    a.cam = tsdf_camera_of(v, w);
    a.out6 = w.out6; a.w2c = w.w2c; a.skip = w.skip; a.skipped = w.skipped; a.flags = flags;
    const long long pixels = (long long)w.width * w.height;
    hipLaunchKernelGGL(tsdf_mark_kernel, dim3(tsdf_grid_for((pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
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
    a.grid = tsdf_grid_of(v);
    a.bricks = bricks_of(v);
    a.vol = arrays_of(v);
    a.cam = tsdf_camera_of(v, w);
    a.out6 = w.out6; a.w2c = w.w2c; a.skip = w.skip; a.skipped = w.skipped;
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel, dim3(tsdf_grid_for(v.slots)), dim3(kBlock), 0, s, a);      // (one block even without slots: `skip` is counted)
    return hipGetLastError();
}

hipError_t launch_tsdf_sparse_triangles(const SplatTsdfSparse &v, float min_weight, int64_t *keys, long long capacity, int64_t *count, bool cubes,
                                        hipStream_t s) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    if (v.nx < 2 || v.ny < 2 || v.nz < 2 || v.slots == 0) return hipSuccess;       // no cell
    SparseTrianglesArgs a;
    a.grid = tsdf_grid_of(v);
    a.bricks = bricks_of(v);
    a.vol = arrays_of(v);
    a.min_weight = min_weight;
    a.keys = keys; a.capacity = capacity; a.count = reinterpret_cast<unsigned long long *>(count);
    if (cubes) hipLaunchKernelGGL(tsdf_sparse_triangles_kernel<true>, dim3(tsdf_grid_for(v.slots)), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(tsdf_sparse_triangles_kernel<false>, dim3(tsdf_grid_for(v.slots)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tsdf_sparse_vertices(const SplatTsdfSparse &v, const int64_t *keys, long long n, float *vertices, float *colors, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tsdf_sparse_vertices_kernel, dim3(tsdf_grid_for((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tsdf_grid_of(v), bricks_of(v),
                       arrays_of(v), keys, n, (long long)v.nx * v.ny * v.nz, vertices, colors);
    return hipGetLastError();
}

}  // namespace splat
