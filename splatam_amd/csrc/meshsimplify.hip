// meshsimplify.hip -- the mesh simplification layer: vertex clustering on a uniform world-anchored grid with quadric placement.  The
// loop bodies are meshsimplify_math.h's (its header comment carries the definitions and the bounds); here are the launches and the
// cross-lane work.
//
//   S0 sq_keys_kernel      one lane per vertex: sq_key.
//   S1 sq_vertices_kernel  one lane per vertex: the count and the six words of sq_vertex_terms, added to the vertex's cluster.
//   S2 sq_quadrics_kernel  one lane per face: sq_face_terms -- up to three slots of ten words, one per distinct cluster of the face.
//   S3 sq_place_kernel     one lane per cluster: sq_place.
//   S4 sq_faces_kernel     one lane per face: sq_face_triple.
//
// S1 and S2 add by integer atomics only, so the sums do not depend on order or on the run.  A 64-bit atomic of a lane of its own is
// the slowest access the memory side knows (64 lanes to 64 rows run at a seventeenth of the rate of a coalesced wave-instruction, and
// every lane adding into ONE row is as slow), and neighbouring faces share clusters almost always: so a wave first adds up each RUN of
// consecutive lanes that hold the same cluster by a segmented scan over shuffles (six steps, whatever the number of runs), and only
// the last lane of a run issues atomics -- to words that lie side by side.  Lanes of one cluster that are not neighbours simply make
// two runs: the sums are the same.
#include "splat_device.h"
#include "meshsimplify_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;

unsigned blocks_for(long long n) { return splat::blocks_for(n, kBlock); }

// Every lane of the wave calls it.  g: the cluster this lane's N words t belong to, -1 for none.  After it, the last lane of each run
// of equal g holds the run's sums in t and gets true.
template <int N>
__device__ bool wave_sum_runs(int32_t g, unsigned long long (&t)[N]) {
    const int lane = threadIdx.x & 63;
    const int32_t before = __shfl_up(g, 1, 64), after = __shfl_down(g, 1, 64);
    int head = lane == 0 || before != g;
    for (int h = 1; h < 64; h <<= 1) {
        unsigned long long up[N];
        for (int k = 0; k < N; ++k) up[k] = __shfl_up(t[k], h, 64);
        const int head_up = __shfl_up(head, h, 64);
        if (lane >= h) {
            if (!head)
                for (int k = 0; k < N; ++k) t[k] += up[k];              // (unsigned: a sum beyond the range wraps as the atomic would)
            head |= head_up;
        }
    }
    return g >= 0 && (lane == 63 || after != g);
}

__global__ void __launch_bounds__(kBlock) sq_keys_kernel(const float *vertices, int32_t V, double cell, int64_t *keys) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v < V) keys[v] = sq_key(vertices + 3 * v, cell);
}

__global__ void __launch_bounds__(kBlock) sq_vertices_kernel(const float *vertices, const float *colors, int32_t V, const int32_t *cluster,
                                                             double cell, int32_t *count, int64_t *sums) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    int32_t g = -1;
    unsigned long long t[7] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (v < V) {
        const int32_t c = cluster[v];
        int64_t q[6];
        if (c >= 0 && c < V && sq_vertex_terms(vertices + 3 * v, colors ? colors + 3 * v : nullptr, cell, q)) {
            g = c;
            for (int k = 0; k < 6; ++k) t[k] = (unsigned long long)q[k];
            t[6] = 1ull;
        }
    }
    if (!__any(g >= 0)) return;
    if (!wave_sum_runs<7>(g, t)) return;
    mc_add(count + g, (int32_t)t[6]);
    int64_t *row = sums + (long long)kSqSums * g;
    for (int k = 0; k < 6; ++k)
        if (t[k] != 0ull) mc_add64(row + k, (int64_t)t[k]);
}

__global__ void __launch_bounds__(kBlock) sq_quadrics_kernel(const float *vertices, int32_t V, const int32_t *faces, int32_t F,
                                                             const int32_t *cluster, double cell, int64_t *sums, int32_t *refused) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    int32_t g[3] = {-1, -1, -1};
    int64_t q[3][10];
    if (i < F) {
        const int32_t f[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
        double d[3];
        int32_t bad = 0;
        sq_face_terms(vertices, V, f, cluster, cell, g, q, d, &bad);
        if (bad) mc_max(refused, 1);
    }
    for (int s = 0; s < 3; ++s) {
        if (!__any(g[s] >= 0)) continue;                                // (wave-uniform: slots 1 and 2 are live only where a face crosses cells)
        unsigned long long t[10];
        for (int k = 0; k < 10; ++k) t[k] = g[s] >= 0 ? (unsigned long long)q[s][k] : 0ull;
        if (!wave_sum_runs<10>(g[s], t)) continue;
        int64_t *row = sums + (long long)kSqSums * g[s] + kSqA;
        for (int k = 0; k < 10; ++k)
            if (t[k] != 0ull) mc_add64(row + k, (int64_t)t[k]);
    }
}

__global__ void __launch_bounds__(kBlock) sq_place_kernel(const int32_t *count, const int64_t *sums, const int64_t *cell_keys, int32_t n,
                                                          double cell, int quadric, float *positions, float *colors, int32_t *rank,
                                                          int32_t *fallback, double *value) {
    const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n) return;
    sq_place(count[c], sums + (long long)kSqSums * c, cell_keys[c], cell, quadric != 0, positions + 3 * c, colors ? colors + 3 * c : nullptr,
             rank + c, fallback + c, value + c);
}

__global__ void __launch_bounds__(kBlock) sq_faces_kernel(const int32_t *faces, int32_t F, int32_t V, const int32_t *cluster, int32_t *triples) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= F) return;
    const int32_t f[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
    int32_t tri[3];
    sq_face_triple(f, V, cluster, tri);
    for (int k = 0; k < 3; ++k) triples[3 * i + k] = tri[k];
}

}  // namespace

hipError_t launch_mesh_simplify_keys(const float *vertices, int32_t V, double cell, int64_t *keys, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipLaunchKernelGGL(sq_keys_kernel, dim3(blocks_for(V)), dim3(kBlock), 0, s, vertices, V, cell, keys);
    return hipGetLastError();
}

hipError_t launch_mesh_simplify_vertices(const float *vertices, const float *colors, int32_t V, const int32_t *cluster, double cell,
                                         int32_t *count, int64_t *sums, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipLaunchKernelGGL(sq_vertices_kernel, dim3(blocks_for(V)), dim3(kBlock), 0, s, vertices, colors, V, cluster, cell, count, sums);
    return hipGetLastError();
}

hipError_t launch_mesh_simplify_quadrics(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const int32_t *cluster, double cell,
                                         int64_t *sums, int32_t *refused, hipStream_t s) {
    if (V == 0 || F == 0) return hipSuccess;
    hipLaunchKernelGGL(sq_quadrics_kernel, dim3(blocks_for(F)), dim3(kBlock), 0, s, vertices, V, faces, F, cluster, cell, sums, refused);
    return hipGetLastError();
}

hipError_t launch_mesh_simplify_place(const int32_t *count, const int64_t *sums, const int64_t *cell_keys, int32_t n, double cell, int quadric,
                                      float *positions, float *colors, int32_t *rank, int32_t *fallback, double *value, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sq_place_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, count, sums, cell_keys, n, cell, quadric, positions, colors, rank,
                       fallback, value);
    return hipGetLastError();
}

hipError_t launch_mesh_simplify_faces(const int32_t *faces, int32_t F, int32_t V, const int32_t *cluster, int32_t *triples, hipStream_t s) {
    if (F == 0) return hipSuccess;
    hipLaunchKernelGGL(sq_faces_kernel, dim3(blocks_for(F)), dim3(kBlock), 0, s, faces, F, V, cluster, triples);
    return hipGetLastError();
}

}  // namespace splat
