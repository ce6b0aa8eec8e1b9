// meshclean.hip -- the mesh cleaning layer: connected components of a triangle mesh given by its faces, and per-component statistics.
// The loop bodies are meshclean_math.h's (its header comment carries the memory and termination arguments); here are the launches and
// the cross-lane work.
//
//   C1 mc_init_kernel       one lane per vertex: parent[v] = v.
//      mc_link_kernel       one lane per face: mc_link_face -- link(f0, f1), link(f1, f2) on a concurrent union-find: find with path
//                           halving, the larger root hooked under the smaller by a compare-and-swap.  Every access to `parent` is an
//                           agent-scope atomic; both loops are bounded because parent[v] <= v holds for every value ever stored.
//      mc_flatten_kernel    a launch of its own (the kernel boundary publishes the forest): parent[v] <- mc_root(v), by an atomic min,
//                           so the word still only goes down while other lanes walk through it.  labels[v] is then the smallest vertex
//                           index of v's component.
//   C2 mc_stats_init_kernel one lane per vertex: counts and area 0, lo / hi to the highest / lowest key.
//      mc_stats_vertices_kernel / mc_stats_faces_kernel   one lane per vertex / face.  When every live lane of a wave holds the same
//                           label (the common case: a mesh is mostly one large component, and extract() orders faces and vertices in
//                           space) the wave adds up its counts, quanta and box by shuffles and lane 0 issues ONE set of atomics;
//                           otherwise every lane issues its own.  All of them are integer atomics, so the sums do not depend on which
//                           way a wave went, on order or on the run.
#include "splat_device.h"
#include "meshclean_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;

unsigned blocks_for(long long n) { return splat::blocks_for(n, kBlock); }

__global__ void __launch_bounds__(kBlock) mc_init_kernel(int32_t *parent, int32_t V) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v < V) parent[v] = (int32_t)v;
}

__global__ void __launch_bounds__(kBlock) mc_link_kernel(const int32_t *faces, int32_t F, int32_t V, int32_t *parent) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= F) return;
    const int32_t f[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
    mc_link_face(parent, V, f);
}

__global__ void __launch_bounds__(kBlock) mc_flatten_kernel(int32_t *parent, int32_t V) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const int32_t r = mc_root(parent, (int32_t)v);
    if (r != (int32_t)v) mc_min(parent + v, r);
}

__global__ void __launch_bounds__(kBlock) mc_stats_init_kernel(int32_t V, int32_t *num_v, int32_t *num_f, int64_t *area_q, int32_t *lo,
                                                               int32_t *hi) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    num_v[v] = 0;
    num_f[v] = 0;
    area_q[v] = 0;
    for (int k = 0; k < 3; ++k) {
        lo[3 * v + k] = kMcKeyHighest;
        hi[3 * v + k] = kMcKeyLowest;
    }
}

// true when every live lane of the wave holds the label r0 (and one lane is live); every lane of the wave must call it
__device__ bool wave_shares_label(bool live, int32_t r, int32_t &r0) {
    const unsigned long long mask = __ballot(live);
    if (mask == 0ull) return false;
    r0 = __shfl(r, __ffsll((long long)mask) - 1, 64);
    return __all(!live || r == r0);
}

__global__ void __launch_bounds__(kBlock) mc_stats_vertices_kernel(const float *vertices, int32_t V, const int32_t *labels, int32_t *num_v,
                                                                   int32_t *lo, int32_t *hi) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    int32_t r = v < V ? labels[v] : -1;
    const bool live = r >= 0 && r < V;                                  // (labels are the caller's: one outside the arrays counts for nothing)
    int32_t r0 = -1;
    if (!wave_shares_label(live, r, r0)) {
        if (live) mc_count_vertex(vertices + 3 * v, r, num_v, lo, hi);
        return;
    }
    int32_t count = live ? 1 : 0, kmin[3], kmax[3];
    for (int k = 0; k < 3; ++k) {
        kmin[k] = live ? mc_float_key(vertices[3 * v + k]) : kMcKeyHighest;
        kmax[k] = live ? kmin[k] : kMcKeyLowest;
    }
    for (int h = 32; h >= 1; h >>= 1) {
        count += __shfl_down(count, h, 64);
        for (int k = 0; k < 3; ++k) {
            const int32_t a = __shfl_down(kmin[k], h, 64), b = __shfl_down(kmax[k], h, 64);
            kmin[k] = a < kmin[k] ? a : kmin[k];
            kmax[k] = b > kmax[k] ? b : kmax[k];
        }
    }
    if ((threadIdx.x & 63) != 0) return;
    mc_add(num_v + r0, count);
    for (int k = 0; k < 3; ++k) {
        mc_min(lo + 3 * (long long)r0 + k, kmin[k]);
        mc_max(hi + 3 * (long long)r0 + k, kmax[k]);
    }
}

__global__ void __launch_bounds__(kBlock) mc_stats_faces_kernel(const float *vertices, int32_t V, const int32_t *faces, int32_t F,
                                                                const int32_t *labels, int32_t *num_f, int64_t *area_q) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    int32_t r = -1;
    unsigned long long quanta = 0ull;
    if (i < F) {
        const int32_t f[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
        r = mc_face_label(labels, V, f);
        if (r >= 0 && r < V) quanta = (unsigned long long)mc_area_quanta(ms_face_area(vertices, V, f));
    }
    const bool live = r >= 0 && r < V;
    int32_t r0 = -1;
    if (!wave_shares_label(live, r, r0)) {
        if (live) mc_count_faces(r, 1, (int64_t)quanta, num_f, area_q);
        return;
    }
    int32_t count = live ? 1 : 0;
    for (int h = 32; h >= 1; h >>= 1) {
        count += __shfl_down(count, h, 64);
        quanta += __shfl_down(quanta, h, 64);                           // (unsigned: a sum beyond the range wraps as the atomic would)
    }
    if ((threadIdx.x & 63) == 0) mc_count_faces(r0, count, (int64_t)quanta, num_f, area_q);
}

}  // namespace

hipError_t launch_mesh_components(const int32_t *faces, int32_t F, int32_t V, int32_t *labels, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipLaunchKernelGGL(mc_init_kernel, dim3(blocks_for(V)), dim3(kBlock), 0, s, labels, V);
    if (F > 0) {
        hipLaunchKernelGGL(mc_link_kernel, dim3(blocks_for(F)), dim3(kBlock), 0, s, faces, F, V, labels);
        hipLaunchKernelGGL(mc_flatten_kernel, dim3(blocks_for(V)), dim3(kBlock), 0, s, labels, V);
    }
    return hipGetLastError();
}

hipError_t launch_mesh_component_stats(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const int32_t *labels, int32_t *num_v,
                                       int32_t *num_f, int64_t *area_q, int32_t *lo, int32_t *hi, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipLaunchKernelGGL(mc_stats_init_kernel, dim3(blocks_for(V)), dim3(kBlock), 0, s, V, num_v, num_f, area_q, lo, hi);
    hipLaunchKernelGGL(mc_stats_vertices_kernel, dim3(blocks_for(V)), dim3(kBlock), 0, s, vertices, V, labels, num_v, lo, hi);
    if (F > 0)
        hipLaunchKernelGGL(mc_stats_faces_kernel, dim3(blocks_for(F)), dim3(kBlock), 0, s, vertices, V, faces, F, labels, num_f, area_q);
    return hipGetLastError();
}

}  // namespace splat
