// Host build of splatam_amd/csrc/meshsimplify_math.h for tests/test_meshsimplify_cpu.py and tests/test_gpu_meshsimplify.py: plain-loop
// models of the kernels of csrc/meshsimplify.hip that call nothing but the header's functions (on the host its atomics are plain loads
// and stores).  Built with -ffp-contract=off.  With -DMESHSIMPLIFY_SHIM_MAIN it is a stand-alone program for the sanitizers (main at
// the end).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../splatam_amd/csrc/meshsimplify_math.h"

using namespace splat;

extern "C" {

// S0
void sqs_keys(const float *vertices, int32_t V, double cell, int64_t *keys) {
    for (int32_t v = 0; v < V; ++v) keys[v] = sq_key(vertices + 3 * (int64_t)v, cell);
}

// S1: adds to count [V] and sums [V][16], which the caller zeroed
void sqs_vertices(const float *vertices, const float *colors, int32_t V, const int32_t *cluster, double cell, int32_t *count, int64_t *sums) {
    for (int32_t v = 0; v < V; ++v) {
        const int32_t g = cluster[v];
        int64_t t[6];
        if (g < 0 || g >= V || !sq_vertex_terms(vertices + 3 * (int64_t)v, colors ? colors + 3 * (int64_t)v : nullptr, cell, t)) continue;
        mc_add(count + g, 1);
        for (int k = 0; k < 6; ++k) mc_add64(sums + (int64_t)kSqSums * g + k, t[k]);
    }
}

// S2: adds to sums; returns the largest |d| of any contribution; *contributions counts them, *refused is raised
double sqs_quadrics(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const int32_t *cluster, double cell, int64_t *sums,
                    int32_t *refused, int64_t *contributions) {
    double worst = 0.0;
    for (int32_t i = 0; i < F; ++i) {
        int32_t g[3];
        int64_t t[3][10];
        double d[3];
        sq_face_terms(vertices, V, faces + 3 * (int64_t)i, cluster, cell, g, t, d, refused);
        for (int s = 0; s < 3; ++s) {
            if (g[s] < 0) continue;
            for (int k = 0; k < 10; ++k) mc_add64(sums + (int64_t)kSqSums * g[s] + kSqA + k, t[s][k]);
            worst = fabs(d[s]) > worst ? fabs(d[s]) : worst;
            if (contributions) ++*contributions;
        }
    }
    return worst;
}

// S3
void sqs_place(const int32_t *count, const int64_t *sums, const int64_t *cell_keys, int32_t n, double cell, int quadric, float *positions,
               float *colors, int32_t *rank, int32_t *fallback, double *value) {
    for (int32_t c = 0; c < n; ++c)
        sq_place(count[c], sums + (int64_t)kSqSums * c, cell_keys[c], cell, quadric != 0, positions + 3 * (int64_t)c,
                 colors ? colors + 3 * (int64_t)c : nullptr, rank + c, fallback + c, value + c);
}

// ... and the points of S3 before they are rounded: p [n][3], local to each cell, in double (zeros for a cluster without a vertex)
void sqs_solve(const int32_t *count, const int64_t *sums, int32_t n, int quadric, double *p) {
    for (int32_t c = 0; c < n; ++c) {
        int32_t rank, fallback;
        double value;
        p[3 * (int64_t)c] = p[3 * (int64_t)c + 1] = p[3 * (int64_t)c + 2] = 0.0;
        if (count[c] > 0) sq_solve(count[c], sums + (int64_t)kSqSums * c, quadric != 0, p + 3 * (int64_t)c, nullptr, &rank, &fallback, &value);
    }
}

// S4
void sqs_faces(const int32_t *faces, int32_t F, int32_t V, const int32_t *cluster, int32_t *triples) {
    for (int32_t i = 0; i < F; ++i) sq_face_triple(faces + 3 * (int64_t)i, V, cluster, triples + 3 * (int64_t)i);
}

int sqs_num_sums(void) { return kSqSums; }

}

#ifdef MESHSIMPLIFY_SHIM_MAIN
// Degenerate inputs through every function; a sanitizer report or a wrong answer is a non-zero exit.
static int fail(const char *what) {
    printf("meshsimplify_math: %s\n", what);
    return 1;
}

// the clusters of `keys` as the caller makes them: ranks of the distinct keys >= 0
static void ranks(const int64_t *keys, int32_t V, int32_t *cluster, int64_t *cell_keys) {
    int32_t n = 0;
    for (int32_t v = 0; v < V; ++v) cell_keys[v] = -1;
    for (int32_t v = 0; v < V; ++v) {
        cluster[v] = -1;
        if (keys[v] < 0) continue;
        int32_t r = 0;
        bool seen = false;
        for (int32_t u = 0; u < V; ++u) {
            if (keys[u] < 0) continue;
            bool first = true;
            for (int32_t w = 0; w < u; ++w) first = first && keys[w] != keys[u];
            if (first && keys[u] < keys[v]) ++r;
            seen = seen || u == v;
        }
        cluster[v] = r;
        cell_keys[r] = keys[v];
        n = r + 1 > n ? r + 1 : n;
    }
    (void)n;
}

int main() {
    // V = 0 and F = 0: nothing is touched
    sqs_keys(nullptr, 0, 0.1, nullptr);
    sqs_vertices(nullptr, nullptr, 0, nullptr, 0.1, nullptr, nullptr);
    int32_t refused = 0;
    sqs_quadrics(nullptr, 0, nullptr, 0, nullptr, 0.1, nullptr, &refused, nullptr);
    sqs_place(nullptr, nullptr, nullptr, 0, 0.1, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
    sqs_faces(nullptr, 0, 0, nullptr, nullptr);
    // keys: negative coordinates, x = j cell, -0, denormals, values that are no numbers, the last index in range and the first beyond
    const double cell = 0.25;
    const float limit = 262144.f;                                       // 2^20 cells of 0.25
    const float probe[8 * 3] = {-0.f, 0.f, 1e-45f,   -1e-45f, 0.25f, -0.25f,   NAN, 0, 0,   0, INFINITY, 0,   0, 0, -INFINITY,
                                limit - 0.25f, -limit + 0.25f, 0,   limit, 0, 0,   0, -limit - 0.25f, 0};
    int64_t keys[8];
    sqs_keys(probe, 8, cell, keys);
    const int64_t L = 1 << 20;
    if (keys[0] != ((L << 42) | (L << 21) | L)) return fail("the key of the origin");
    if (keys[1] != ((L - 1) << 42 | (L + 1) << 21 | (L - 1))) return fail("floor of negative and exact coordinates");
    if (keys[2] != -1 || keys[3] != -1 || keys[4] != -1) return fail("vertices that are no numbers");
    if (keys[5] != ((L << 42) | ((int64_t)1 << 21) | (2 * L - 1))) return fail("the last index in range");
    if (keys[6] != -1 || keys[7] != -1) return fail("the first index beyond");
    // the edge semantics: a repeated index, indices out of range (INT32_MIN / INT32_MAX among them), a NaN vertex, a zero-area face
    // across three cells, an unreferenced vertex, a face of infinite area, clusters that are not the call's own
    const int32_t V = 10;
    float vertices[V * 3] = {0.1f, 0.1f, 0.1f,   1.1f, 0.1f, 0.1f,   0.1f, 1.1f, 0.1f,   NAN, 0.1f, 0.1f,   2.1f, 0.1f, 0.1f,   3.1f, 0.1f, 0.1f,
                             4.1f, 0.1f, 0.1f,   9.f, 9.f, 9.f,   -3e38f, -3e38f, 0,   3e38f, -3e38f, 0};
    const float colors[V * 3] = {1, 0, 0,   0, 1, 0,   0, 0, 1,   NAN, INFINITY, -INFINITY,   3e38f, -3e38f, 0.5f,   0, 0, 0,   1, 1, 1,   0, 0, 0,
                                 0, 0, 0,   0, 0, 0};
    const int32_t faces[] = {0, 1, 2,   0, 0, 1,   0, 1, 10,   -1, 0, 1,   INT32_MAX, 0, 1,   INT32_MIN, 1, 2,   0, 3, 1,   4, 5, 6,   1, 2, 0};
    const int32_t F = 9;
    int64_t k10[V], cell_keys[V], sums[V * 16];
    int32_t cluster[V], count[V], triples[F * 3];
    sqs_keys(vertices, V, 1.0, k10);
    if (k10[3] != -1 || k10[8] != -1 || k10[9] != -1) return fail("keys of the degenerate mesh");
    ranks(k10, V, cluster, cell_keys);
    memset(sums, 0, sizeof sums);
    memset(count, 0, sizeof count);
    sqs_vertices(vertices, colors, V, cluster, 1.0, count, sums);
    int64_t contributions = 0;
    const double worst = sqs_quadrics(vertices, V, faces, F, cluster, 1.0, sums, &refused, &contributions);
    if (refused) return fail("nothing here is beyond the range");
    if (contributions != 6) return fail("two faces across three cells add three times each, nothing else adds");
    if (!(worst <= 0.8660254037844387)) return fail("|d| <= sqrt(3) / 2");
    float positions[V * 3], mean_colors[V * 3];
    int32_t rank[V], fallback[V];
    double value[V];
    for (int quadric = 0; quadric < 2; ++quadric) {
        sqs_place(count, sums, cell_keys, V, 1.0, quadric, positions, mean_colors, rank, fallback, value);
        for (int32_t c = 0; c < V; ++c)
            for (int k = 0; k < 3; ++k)
                if (!(positions[3 * c + k] == positions[3 * c + k])) return fail("a position that is no number");
    }
    sqs_faces(faces, F, V, cluster, triples);
    if (triples[0] < 0 || triples[3] != -1 || triples[6] != -1 || triples[9] != -1 || triples[12] != -1 || triples[15] != -1 || triples[18] != -1)
        return fail("faces that go");
    if (triples[21] < 0 || triples[24] != triples[0] || triples[25] != triples[1] || triples[26] != triples[2]) return fail("rotation");
    // a face of infinite area raises the flag and adds nothing
    const int32_t wide[3] = {8, 9, 0};
    int32_t own[V];
    for (int32_t v = 0; v < V; ++v) own[v] = v;                         // (clusters that are not the call's own, but inside the arrays)
    memset(sums, 0, sizeof sums);
    sqs_quadrics(vertices, V, wide, 1, own, 1.0, sums, &refused, nullptr);
    if (!refused) return fail("a face beyond the range");
    for (int k = 0; k < V * 16; ++k)
        if (sums[k] != 0) return fail("a refused face added something");
    int32_t stray[V] = {0, 11, -4, INT32_MAX, INT32_MIN, 5, 6, 7, 8, 9}; // clusters outside the arrays: nothing outside is touched
    refused = 0;
    sqs_vertices(vertices, colors, V, stray, 1.0, count, sums);
    sqs_quadrics(vertices, V, faces, F, stray, 1.0, sums, &refused, nullptr);
    sqs_faces(faces, F, V, stray, triples);
    // placement from words that mean nothing: huge, negative, a count of zero, a key of -1
    int64_t wild[16];
    for (int k = 0; k < 16; ++k) wild[k] = (k % 2 ? INT64_MIN : INT64_MAX) / (k + 1);
    const int32_t one = 1, none = 0;
    const int64_t origin = (L << 42) | (L << 21) | L, nokey = -1;
    sqs_place(&one, wild, &origin, 1, 1e-300, 1, positions, mean_colors, rank, fallback, value);
    sqs_place(&one, wild, &origin, 1, 1e300, 1, positions, nullptr, rank, fallback, value);
    sqs_place(&none, wild, &origin, 1, 1.0, 1, positions, mean_colors, rank, fallback, value);
    sqs_place(&one, wild, &nokey, 1, 1.0, 1, positions, mean_colors, rank, fallback, value);
    if (positions[0] != 0.f || rank[0] != 0 || fallback[0] != 0) return fail("a cluster without a key");
    printf("meshsimplify_math: ok\n");
    return 0;
}
#endif
