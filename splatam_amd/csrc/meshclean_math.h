// meshclean_math.h -- loop bodies of the mesh cleaning layer (meshclean.hip), written once as host/device inline functions: the kernels
// call them per lane, tests/test_meshclean_cpu.py compiles the very same header with g++ (tests/meshclean_math_shim.cpp) and checks it
// against the numpy restatement tests/meshclean_ref.py.
//
//   COMPONENTS  two vertices belong to one component when a chain of faces that share a vertex INDEX joins them.  A face with an index
//               outside 0..V-1 links nothing; a face with a repeated index links the vertices it names; a vertex no face names is a
//               component of its own.  The label of a component is its smallest vertex index.
//   FOREST      parent[v] = v at first.  mc_link(u, v) finds both roots and hooks the LARGER root under the smaller one with a
//               compare-and-swap on parent[larger]; mc_find halves the path it walks (parent[v] <- parent[parent[v]], by an atomic min).
//               A second launch flattens: parent[v] <- mc_root(v).
//   MEMORY      on the device every read of `parent` while links run is an agent-scope relaxed atomic load and every write an
//               agent-scope atomic (compare-and-swap, min): the per-XCD L2s are not coherent with each other and a CU's L1 is never
//               refreshed by another CU's stores, so a plain load may return a value of any age.  After a failed compare-and-swap the
//               walk goes on from the value it returned, which is the word's value at the point of coherence; nothing is re-read.  The
//               flatten pass is a launch of its own: the kernel boundary publishes the forest.  On the host the same functions are
//               plain loads and stores.
//   TERMINATION every value ever stored to parent[v] is <= v: the initial v; a hook stores the smaller root under the larger; halving
//               stores parent[parent[v]] <= parent[v] <= v, and by an atomic MIN, so a pointer only ever goes down.  A load, however
//               stale, returns a value that was stored once, so it is <= v too.  Hence (1) mc_find walks a strictly decreasing chain of
//               indices: each step either returns or moves to a smaller index, at most v steps; (2) in mc_link_roots every retry follows
//               a compare-and-swap that found parent[a] != a, i.e. < a, and continues from mc_find of that value: the larger candidate
//               strictly decreases while the smaller never grows, so a + b strictly decreases and the loop ends after at most a + b
//               rounds.  Neither loop spins on a value another lane has yet to write.
//   CORRECTNESS trees only ever merge, and an index is hooked only under an index of the tree it is being joined to.  A stale "root"
//               is still an ancestor in the same tree: if both walks return the same index the two vertices share a tree; otherwise the
//               compare-and-swap on the larger candidate either succeeds on a true root (the trees are joined) or fails and names its
//               current parent.  When every link has returned, every face's vertices share a tree, the root of a tree is <= all of its
//               indices, hence its minimum: labels are canonical -- the same bits on every run and for every face order.
//   STATISTICS  per root label: vertices and faces (integer adds), the area as a sum of per-face QUANTA of 2^-40 m^2 (mc_area_quanta of
//               ms_face_area's double: rint, ties to even; a 64-bit integer add, so the sum is exact in the quanta and independent of
//               order; it holds 2^63 quanta = 2^23 m^2, about 8.4e6 m^2 per component, and wraps beyond; a face whose area is not below
//               2^22 m^2 -- an infinite one included -- adds kMcAreaBad = 2^62 quanta, which callers test for; a NaN area is 0, as in
//               splat_mesh_areas), and the box as integer min / max of mc_float_key, an order-preserving map of the float's bits onto
//               int32 for both signs (-0 counts as +0; a NaN sorts beyond the infinity of its sign).  No float atomics anywhere.
#pragma once

#include <math.h>
#include <stdint.h>

#include "meshscore_math.h"

namespace splat {

constexpr double kMcAreaScale = 1099511627776.0;                        // 2^40 quanta per m^2
constexpr double kMcAreaQuantum = 1.0 / 1099511627776.0;
constexpr double kMcFaceAreaLimit = 4194304.0;                          // 2^22 m^2: a face at or beyond it is not summed
constexpr int64_t kMcAreaBad = (int64_t)1 << 62;
constexpr int32_t kMcKeyLowest = INT32_MIN, kMcKeyHighest = INT32_MAX;  // what hi / lo start from

// ---------------------------------------------------------------------------------------------------------------- the words of the forest
#if defined(__HIP_DEVICE_COMPILE__)
SPLAT_HD int32_t mc_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the word's value before the call: `expected` when the swap took place
SPLAT_HD int32_t mc_cas(int32_t *p, int32_t expected, int32_t desired) {
    __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;
}
SPLAT_HD void mc_min(int32_t *p, int32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
SPLAT_HD void mc_max(int32_t *p, int32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
SPLAT_HD void mc_add(int32_t *p, int32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
SPLAT_HD void mc_add64(int64_t *p, int64_t v) {                         // (two's complement: the unsigned add is the signed one)
    __hip_atomic_fetch_add((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
SPLAT_HD double mc_rint(double x) { return __builtin_rint(x); }
#else
SPLAT_HD int32_t mc_load(const int32_t *p) { return *p; }
SPLAT_HD int32_t mc_cas(int32_t *p, int32_t expected, int32_t desired) {
    const int32_t old = *p;
    if (old == expected) *p = desired;
    return old;
}
SPLAT_HD void mc_min(int32_t *p, int32_t v) { if (v < *p) *p = v; }
SPLAT_HD void mc_max(int32_t *p, int32_t v) { if (v > *p) *p = v; }
SPLAT_HD void mc_add(int32_t *p, int32_t v) { *p += v; }
SPLAT_HD void mc_add64(int64_t *p, int64_t v) { *p = (int64_t)((uint64_t)*p + (uint64_t)v); }
SPLAT_HD double mc_rint(double x) { return rint(x); }
#endif

// ---------------------------------------------------------------------------------------------------------------- C1: the forest
// the root of v's tree as far as this lane can see it, halving the path on the way (TERMINATION (1))
SPLAT_HD int32_t mc_find(int32_t *parent, int32_t v) {
    for (;;) {
        const int32_t p = mc_load(parent + v);
        if (p == v) return v;
        const int32_t g = mc_load(parent + p);
        if (g == p) return p;
        mc_min(parent + v, g);
        v = g;
    }
}

// join the trees of the candidate roots a and b (TERMINATION (2)); they need not be roots any more
SPLAT_HD void mc_link_roots(int32_t *parent, int32_t a, int32_t b) {
    while (a != b) {
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = mc_cas(parent + a, a, b);                   // hook the larger under the smaller
        if (old == a) return;
        a = mc_find(parent, old);                                       // a was no root: go on from its parent as the swap saw it
    }
}

SPLAT_HD void mc_link(int32_t *parent, int32_t u, int32_t v) {
    if (u == v) return;
    mc_link_roots(parent, mc_find(parent, u), mc_find(parent, v));
}

// one face: link(f0, f1), link(f1, f2); a face that names a vertex outside 0..V-1 links nothing
SPLAT_HD void mc_link_face(int32_t *parent, int32_t V, const int32_t *f) {
    if (!ms_face_valid(f, V)) return;
    mc_link(parent, f[0], f[1]);
    mc_link(parent, f[1], f[2]);
}

// the root of v without a write: the flatten pass stores it to parent[v] (other lanes' stores only shorten the chain it walks)
SPLAT_HD int32_t mc_root(const int32_t *parent, int32_t v) {
    for (;;) {
        const int32_t p = mc_load(parent + v);
        if (p == v) return v;
        v = p;
    }
}

// ---------------------------------------------------------------------------------------------------------------- C2: statistics
SPLAT_HD int32_t mc_float_key(float x) {
    union {
        float f;
        int32_t i;
    } u;
    u.f = x == 0.f ? 0.f : x;                                           // (-0 -> +0; a NaN compares unequal and keeps its bits)
    return u.i >= 0 ? u.i : (u.i ^ 0x7fffffff);
}
SPLAT_HD float mc_key_float(int32_t k) {                                // (the map is its own inverse)
    union {
        float f;
        int32_t i;
    } u;
    u.i = k >= 0 ? k : (k ^ 0x7fffffff);
    return u.f;
}

SPLAT_HD int64_t mc_area_quanta(double area) {
    if (!(area < kMcFaceAreaLimit)) return kMcAreaBad;                  // (ms_face_area gives no NaN and nothing negative)
    return (int64_t)mc_rint(ms_muld(area, kMcAreaScale));
}

// vertex v of a component with root label r
SPLAT_HD void mc_count_vertex(const float *p, int32_t r, int32_t *num_v, int32_t *lo, int32_t *hi) {
    mc_add(num_v + r, 1);
    for (int k = 0; k < 3; ++k) {
        const int32_t key = mc_float_key(p[k]);
        mc_min(lo + 3 * (int64_t)r + k, key);
        mc_max(hi + 3 * (int64_t)r + k, key);
    }
}

// the root label a face counts for (that of its first vertex), -1 for a face that names a vertex outside 0..V-1
SPLAT_HD int32_t mc_face_label(const int32_t *labels, int32_t V, const int32_t *f) { return ms_face_valid(f, V) ? labels[f[0]] : -1; }

SPLAT_HD void mc_count_faces(int32_t r, int32_t faces, int64_t quanta, int32_t *num_f, int64_t *area_q) {
    mc_add(num_f + r, faces);
    mc_add64(area_q + r, quanta);
}

}  // namespace splat
