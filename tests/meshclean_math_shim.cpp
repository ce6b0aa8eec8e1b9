// Host build of splatam_amd/csrc/meshclean_math.h for tests/test_meshclean_cpu.py: plain-loop models of the kernels of csrc/meshclean.hip
// that call nothing but the header's functions (on the host its atomics are plain loads and stores).  Built with -ffp-contract=off.
// With -DMESHCLEAN_SHIM_MAIN it is a stand-alone program for the sanitizers (main at the end).
#include <stdio.h>
#include <stdlib.h>

#include "../splatam_amd/csrc/meshclean_math.h"

using namespace splat;

extern "C" {

// 0 when parent[v] <= v (and >= 0) for every v
int mcs_invariant(const int32_t *parent, int32_t V) {
    for (int32_t v = 0; v < V; ++v)
        if (parent[v] > v || parent[v] < 0) return 1;
    return 0;
}

// C1's init and link launches, one face after the other; with `check` the invariant is tested after EVERY link.  Returns the number
// of violations seen (0), parent is left UNFLATTENED.
int mcs_link(const int32_t *faces, int32_t F, int32_t V, int32_t *parent, int check) {
    int bad = 0;
    for (int32_t v = 0; v < V; ++v) parent[v] = v;
    for (int32_t i = 0; i < F; ++i) {
        const int32_t *f = faces + 3 * (int64_t)i;
        if (!ms_face_valid(f, V)) {
            mc_link_face(parent, V, f);                                 // (must touch nothing)
            continue;
        }
        mc_link(parent, f[0], f[1]);
        if (check) bad += mcs_invariant(parent, V);
        mc_link(parent, f[1], f[2]);
        if (check) bad += mcs_invariant(parent, V);
    }
    return bad;
}

// C1's flatten launch
void mcs_flatten(int32_t *parent, int32_t V) {
    for (int32_t v = 0; v < V; ++v) {
        const int32_t r = mc_root(parent, v);
        if (r != v) mc_min(parent + v, r);
    }
}

// mc_link_roots from candidates that need not be roots: what a lane does whose finds returned stale answers
void mcs_link_roots(int32_t *parent, int32_t a, int32_t b) { mc_link_roots(parent, a, b); }
int32_t mcs_find(int32_t *parent, int32_t v) { return mc_find(parent, v); }

// C2: init, the vertex pass, the face pass, one element after the other
void mcs_stats(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const int32_t *labels, int32_t *num_v, int32_t *num_f,
               int64_t *area_q, int32_t *lo, int32_t *hi) {
    for (int32_t v = 0; v < V; ++v) {
        num_v[v] = num_f[v] = 0;
        area_q[v] = 0;
        for (int k = 0; k < 3; ++k) {
            lo[3 * (int64_t)v + k] = kMcKeyHighest;
            hi[3 * (int64_t)v + k] = kMcKeyLowest;
        }
    }
    for (int32_t v = 0; v < V; ++v) {
        const int32_t r = labels[v];
        if (r >= 0 && r < V) mc_count_vertex(vertices + 3 * (int64_t)v, r, num_v, lo, hi);
    }
    for (int32_t i = 0; i < F; ++i) {
        const int32_t *f = faces + 3 * (int64_t)i;
        const int32_t r = mc_face_label(labels, V, f);
        if (r >= 0 && r < V) mc_count_faces(r, 1, mc_area_quanta(ms_face_area(vertices, V, f)), num_f, area_q);
    }
}

int32_t mcs_float_key(float x) { return mc_float_key(x); }
float mcs_key_float(int32_t k) { return mc_key_float(k); }
int64_t mcs_area_quanta(double area) { return mc_area_quanta(area); }
double mcs_face_area(const float *vertices, int32_t V, const int32_t *f) { return ms_face_area(vertices, V, f); }
int64_t mcs_area_bad(void) { return kMcAreaBad; }

}

#ifdef MESHCLEAN_SHIM_MAIN
// Degenerate inputs through every function; a sanitizer report or a wrong answer is a non-zero exit.
static int fail(const char *what) {
    printf("meshclean_math: %s\n", what);
    return 1;
}

static int components(const int32_t *faces, int32_t F, int32_t V, int32_t *labels) {
    if (mcs_link(faces, F, V, labels, 1) != 0) return 1;
    mcs_flatten(labels, V);
    return mcs_invariant(labels, V);
}

int main() {
    // F = 0 and V = 0: nothing is touched
    if (components(nullptr, 0, 0, nullptr)) return fail("empty");
    int32_t four[4];
    if (components(nullptr, 0, 4, four) || four[0] != 0 || four[3] != 3) return fail("no faces");
    // repeated and out-of-range indices
    const int32_t faces[] = {5, 5, 5, 1, 1, 2, 3, 4, 9, -1, 0, 1, 4, 3, 3, 7, 2, 2, INT32_MAX, 0, 1, INT32_MIN, 2, 3};
    int32_t lab[8];
    if (components(faces, 8, 8, lab)) return fail("invariant");
    const int32_t want[8] = {0, 1, 1, 3, 3, 5, 6, 1};
    for (int v = 0; v < 8; ++v)
        if (lab[v] != want[v]) return fail("labels of the degenerate faces");
    // statistics of the same, with a vertex that is not a number, one at infinity and a -0
    const float vertices[24] = {0, 0, 0, 1, 0, 0, 0, 1, 0, -0.f, 0, 0, 1e-42f, -1e-42f, 0, NAN, 0, 0, INFINITY, 0, 0, -3e38f, 3e38f, 0};
    int32_t num_v[8], num_f[8], lo[24], hi[24];
    int64_t area_q[8];
    mcs_stats(vertices, 8, faces, 8, lab, num_v, num_f, area_q, lo, hi);
    if (num_v[1] != 3 || num_f[1] != 2 || num_v[3] != 2 || num_f[3] != 1 || num_f[5] != 1 || num_f[0] != 0 || num_v[6] != 1) return fail("counts");
    if (area_q[3] != 0 || area_q[5] != 0) return fail("area of faces with a repeated index");
    if (mcs_key_float(lo[3 * 3]) != 0.f || mcs_key_float(hi[3 * 3]) != 1e-42f || mcs_key_float(lo[3 * 3 + 1]) != -1e-42f) return fail("box");
    int32_t stray[8] = {0, 9, -4, INT32_MAX, INT32_MIN, 5, 6, 7};       // labels that are not the call's own: nothing outside the arrays is touched
    mcs_stats(vertices, 8, faces, 8, stray, num_v, num_f, area_q, lo, hi);
    mcs_stats(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    // an infinite, a huge and a NaN area
    if (mcs_area_quanta(INFINITY) != kMcAreaBad || mcs_area_quanta(4194304.0) != kMcAreaBad || mcs_area_quanta(0.0) != 0) return fail("quanta");
    if (mcs_area_quanta(4194303.0) != (int64_t)4194303 << 40) return fail("largest quanta");
    const float wide[9] = {-3e38f, -3e38f, 0, 3e38f, -3e38f, 0, 0, 3e38f, 0}, nan3[9] = {NAN, 0, 0, 1, 0, 0, 0, 1, 0};
    const int32_t tri[3] = {0, 1, 2};
    if (mcs_area_quanta(mcs_face_area(wide, 3, tri)) != kMcAreaBad || mcs_area_quanta(mcs_face_area(nan3, 3, tri)) != 0) return fail("wide faces");
    // one giant fan around vertex N - 1, rim ascending: the deepest chains hooking builds; then the same from stale candidates
    const int32_t N = 20000;
    int32_t *fan = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)(N - 2)), *parent = (int32_t *)malloc(sizeof(int32_t) * (size_t)N);
    for (int32_t i = 0; i < N - 2; ++i) {
        fan[3 * i] = N - 1;
        fan[3 * i + 1] = N - 2 - i;
        fan[3 * i + 2] = N - 3 - i;
    }
    if (mcs_link(fan, N - 2, N, parent, 0) != 0 || mcs_invariant(parent, N)) return fail("fan");
    mcs_flatten(parent, N);
    for (int32_t v = 0; v < N; ++v)
        if (parent[v] != 0) return fail("fan labels");
    for (int32_t v = 0; v < N; ++v) parent[v] = v > 0 ? v - 1 : 0;      // one chain N - 1 -> ... -> 0, then links between non-roots
    for (int32_t v = N - 1; v > 0; v -= 7) {
        mcs_link_roots(parent, v, v / 2);
        if (mcs_invariant(parent, N)) return fail("stale candidates");
    }
    mcs_flatten(parent, N);
    for (int32_t v = 0; v < N; ++v)
        if (parent[v] != 0) return fail("chain labels");
    free(fan);
    free(parent);
    printf("meshclean_math: ok\n");
    return 0;
}
#endif
