// meshscore.hip -- the mesh score layer: points sampled uniformly by area on a triangle mesh, and the exact nearest neighbour of every
// query among the targets through a uniform grid.  The arithmetic is meshscore_math.h's.
//
//   M0 ms_areas_kernel      one lane per triangle: its area in double (0 for a triangle that names no vertex or has no area).
//   M1 ms_sample_kernel     one lane per sample: Philox at counter i, a binary search in the inclusive prefix sum, the point.
//   M2 ms_cell_keys_kernel  one lane per point: the key of its cell.  Targets and queries alike: both are sorted by key before M3 / M4,
//                           so that a wave's 64 queries sit in the same or neighbouring cells and read the same records.
//   M3 ms_cell_starts_kernel lane i < count packs sorted target i as a 16-byte record (x, y, z, original index); lane k <= cells finds
//                           start[k], the first sorted position of key >= k, by binary search in the sorted keys (18 cached reads at
//                           200 000 targets; the table of an empty grid is all zero).  Lanes filling the gaps between consecutive keys
//                           instead took 225 us at the protocol's size: a gap of a thousand empty cells is one lane's loop.
//   M4 ms_nearest_kernel    one lane per sorted query: ms_nearest, results stored at the query's ORIGINAL position.  (A staged form --
//                           a workgroup of 256 sorted queries copies the records of the box of its cells, grown by one shell, into
//                           LDS and every lane compares against all of them -- gave the same bits in 327 us against this form's
//                           95 us at the protocol's size and was not kept: profiles/mesh_score.md 3.)
//   M5 ms_reduce_kernel     a workgroup per slice of dist2 (lane l of workgroup b takes b 256 + l, then strides by the whole launch):
//                           per lane a running sum / count / max of sqrt((double)d2) in that order, then a tree over the 256 lanes in
//                           LDS (lane l += lane l + h, h = 128 .. 1), one row of partials per workgroup; ms_reduce_finish_kernel
//                           (one workgroup) adds the rows in workgroup order.  No atomics: the same bits on every run.
#include "splat_device.h"
#include "meshscore_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
constexpr int kQueryBlock = 64;         // M4: one wave per workgroup, so that a wave with a long walk holds no other wave's slot

MsGrid grid_of(const SplatNnGrid &g) {
    MsGrid m;
    for (int k = 0; k < 3; ++k) { m.lo[k] = g.lo[k]; m.dims[k] = g.dims[k]; }
    m.cell = g.cell;
    m.count = g.count;
    return m;
}

__global__ void __launch_bounds__(kBlock) ms_areas_kernel(const float *vertices, int32_t V, const int32_t *faces, int32_t F, double *area) {
    const int32_t f = blockIdx.x * kBlock + threadIdx.x;
    if (f < F) area[f] = ms_face_area(vertices, V, faces + 3 * (int64_t)f);
}

__global__ void __launch_bounds__(kBlock) ms_sample_kernel(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const double *prefix,
                                                           uint64_t seed, long long n, float *points, int32_t *face) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float p[3];
    face[i] = ms_sample(vertices, V, faces, F, prefix, seed, (uint64_t)i, p);
    points[3 * i] = p[0];
    points[3 * i + 1] = p[1];
    points[3 * i + 2] = p[2];
}

__global__ void __launch_bounds__(kBlock) ms_cell_keys_kernel(MsGrid g, const float *points, long long n, int32_t *key) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    int32_t c[3];
    ms_cell(g, p, c);
    key[i] = ms_key(g, c);
}

__global__ void __launch_bounds__(kBlock) ms_cell_starts_kernel(int32_t cells, int32_t count, const int32_t *sorted_key, const int32_t *order,
                                                                const float *points, MsRecord *records, int32_t *start) {
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < count) {
        const int32_t src = order[i];
        const bool ok = src >= 0 && src < count;                        // (a permutation is the caller's promise; never read outside)
        MsRecord r;
        r.x = ok ? points[3 * (int64_t)src] : NAN;
        r.y = ok ? points[3 * (int64_t)src + 1] : NAN;
        r.z = ok ? points[3 * (int64_t)src + 2] : NAN;
        r.index = src;
        records[i] = r;
    }
    if (i <= cells) {                                                   // start[i]: the first sorted position whose key is >= i
        int32_t lo = 0, hi = count;
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (sorted_key[mid] >= i) hi = mid;
            else lo = mid + 1;
        }
        start[i] = lo;
    }
}

__global__ void __launch_bounds__(kQueryBlock) ms_nearest_kernel(MsGrid g, const MsRecord *records, const int32_t *start, const float *points,
                                                                 const int32_t *order, long long n, float *dist2, int32_t *index, int32_t *account) {
    const long long i = (long long)blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= n) return;
    long long src = i;
    if (order) {
        src = order[i];
        if (src < 0 || src >= n) return;
    }
    const float q[3] = {points[3 * src], points[3 * src + 1], points[3 * src + 2]};
    float d2;
    int32_t best;
    const MsWalk w = ms_nearest(g, records, start, q, d2, best);
    dist2[src] = d2;
    index[src] = best;
    if (account) {
        account[2 * src] = w.candidates;
        account[2 * src + 1] = w.shells;
    }
}

__global__ void __launch_bounds__(kBlock) ms_reduce_kernel(const float *dist2, long long n, double threshold, double *partials) {
    __shared__ double s_sum[kBlock], s_cnt[kBlock], s_max[kBlock];
    double sum = 0.0, cnt = 0.0, mx = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double d = ms_sqrtd((double)dist2[i]);
        sum = ms_addd(sum, d);
        cnt += d < threshold ? 1.0 : 0.0;
        mx = d > mx ? d : mx;
    }
    s_sum[threadIdx.x] = sum; s_cnt[threadIdx.x] = cnt; s_max[threadIdx.x] = mx;
    __syncthreads();
    for (int h = kBlock / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_sum[threadIdx.x] = ms_addd(s_sum[threadIdx.x], s_sum[threadIdx.x + h]);
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
            const double o = s_max[threadIdx.x + h];
            if (o > s_max[threadIdx.x]) s_max[threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[3 * blockIdx.x] = s_sum[0];
        partials[3 * blockIdx.x + 1] = s_cnt[0];
        partials[3 * blockIdx.x + 2] = s_max[0];
    }
}

__global__ void __launch_bounds__(kBlock) ms_reduce_finish_kernel(const double *partials, int rows, long long n, double *row) {
    __shared__ double s_part[3 * SPLAT_NN_REDUCE_ROWS];
    for (int k = threadIdx.x; k < 3 * rows; k += kBlock) s_part[k] = partials[k];       // (every lane fetches; one lane adds, in order)
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0, cnt = 0.0, mx = 0.0;
    for (int b = 0; b < rows; ++b) {
        sum = ms_addd(sum, s_part[3 * b]);
        cnt += s_part[3 * b + 1];
        const double o = s_part[3 * b + 2];
        mx = o > mx ? o : mx;
    }
    row[0] = sum; row[1] = cnt; row[2] = mx; row[3] = (double)n;
}

}  // namespace

hipError_t launch_mesh_areas(const float *vertices, int32_t V, const int32_t *faces, int32_t F, double *area, hipStream_t s) {
    if (F == 0) return hipSuccess;
    hipLaunchKernelGGL(ms_areas_kernel, dim3(blocks_for(F, kBlock)), dim3(kBlock), 0, s, vertices, V, faces, F, area);
    return hipGetLastError();
}

hipError_t launch_mesh_sample(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const double *prefix, uint64_t seed, long long n,
                              float *points, int32_t *face, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ms_sample_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, s, vertices, V, faces, F, prefix, seed, n, points, face);
    return hipGetLastError();
}

hipError_t launch_nn_cell_keys(const SplatNnGrid &g, const float *points, long long n, int32_t *key, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ms_cell_keys_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, s, grid_of(g), points, n, key);
    return hipGetLastError();
}

hipError_t launch_nn_cell_starts(const SplatNnGrid &g, const int32_t *sorted_key, const int32_t *order, const float *points, float *records,
                                 int32_t *start, hipStream_t s) {
    const int32_t cells = ms_cells(grid_of(g));
    const long long lanes = g.count > cells + 1 ? g.count : cells + 1;
    hipLaunchKernelGGL(ms_cell_starts_kernel, dim3(blocks_for(lanes, kBlock)), dim3(kBlock), 0, s, cells, g.count, sorted_key, order, points,
                       reinterpret_cast<MsRecord *>(records), start);
    return hipGetLastError();
}

hipError_t launch_nn_query(const SplatNnGrid &g, const float *points, const int32_t *order, long long n, float *dist2, int32_t *index,
                           int32_t *account, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ms_nearest_kernel, dim3(blocks_for(n, kQueryBlock)), dim3(kQueryBlock), 0, s, grid_of(g),
                       reinterpret_cast<const MsRecord *>(g.records), g.start, points, order, n, dist2, index, account);
    return hipGetLastError();
}

hipError_t launch_nn_reduce(const float *dist2, long long n, double threshold, double *partials, double *row, hipStream_t s) {
    long long rows = (n + kBlock - 1) / kBlock;
    rows = rows < 1 ? 1 : (rows > SPLAT_NN_REDUCE_ROWS ? SPLAT_NN_REDUCE_ROWS : rows);
    hipLaunchKernelGGL(ms_reduce_kernel, dim3((unsigned)rows), dim3(kBlock), 0, s, dist2, n, threshold, partials);
    hipLaunchKernelGGL(ms_reduce_finish_kernel, dim3(1), dim3(kBlock), 0, s, partials, (int)rows, n, row);
    return hipGetLastError();
}

}  // namespace splat
