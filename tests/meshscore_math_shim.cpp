// Host build of splatam_amd/csrc/meshscore_math.h for tests/test_meshscore_cpu.py (and, as the bit-exact reference of M0 / M1, for
// tests/test_gpu_meshscore.py): plain-loop models of the kernels of csrc/meshscore.hip that call nothing but the header's functions.
// Built with -ffp-contract=off: every float32 and double step of the header is then one operation, as on the device.
#include <algorithm>
#include <numeric>
#include <vector>

#include "../splatam_amd/csrc/meshscore_math.h"

using namespace splat;

namespace {
MsGrid grid(const float *lo, float cell, const int32_t *dims, int32_t count = 0) {
    MsGrid g;
    g.count = count;
    for (int k = 0; k < 3; ++k) { g.lo[k] = lo[k]; g.dims[k] = dims[k]; }
    g.cell = cell;
    return g;
}
}  // namespace

extern "C" {

void mm_uniform3(uint64_t seed, uint64_t first, long long n, float *u) {
    for (long long i = 0; i < n; ++i) ms_uniform3(seed, first + (uint64_t)i, u + 3 * i);
}
void mm_philox(uint64_t seed, uint64_t i, uint32_t *out) { ms_philox4x32_10(seed, i, out); }

// M0
void mm_areas(const float *vertices, int32_t V, const int32_t *faces, int32_t F, double *area) {
    for (int32_t f = 0; f < F; ++f) area[f] = ms_face_area(vertices, V, faces + 3 * (int64_t)f);
}

// M1 (prefix: the inclusive prefix sum the caller formed)
void mm_sample(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const double *prefix, uint64_t seed, long long n, float *points,
               int32_t *face) {
    for (long long i = 0; i < n; ++i) face[i] = ms_sample(vertices, V, faces, F, prefix, seed, (uint64_t)i, points + 3 * i);
}

// M2
int mm_cell_keys(const float *lo, float cell, const int32_t *dims, const float *points, long long n, int32_t *key) {
    const MsGrid g = grid(lo, cell, dims);
    if (!ms_grid_valid(g)) return -1;
    for (long long i = 0; i < n; ++i) {
        int32_t c[3];
        ms_cell(g, points + 3 * i, c);
        key[i] = ms_key(g, c);
    }
    return 0;
}

// M2 - M4 over `m` targets and `n` queries (queries in their given order: the result does not depend on it): dist2 / index [n], and the
// account [n][2] (candidates, shells) when not NULL
int mm_nearest(const float *lo, float cell, const int32_t *dims, const float *targets, int32_t m, const float *queries, long long n, float *dist2,
               int32_t *index, int32_t *account) {
    const MsGrid g = grid(lo, cell, dims, m);
    if (!ms_grid_valid(g)) return -1;
    const int32_t cells = ms_cells(g);
    std::vector<int32_t> key(m), order(m), start(cells + 1, 0);
    mm_cell_keys(lo, cell, dims, targets, m, key.data());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    std::vector<MsRecord> records(m);
    for (int32_t i = 0; i < m; ++i) {
        const int32_t src = order[i];
        records[i] = MsRecord{targets[3 * src], targets[3 * src + 1], targets[3 * src + 2], src};
        const int32_t k0 = i > 0 ? key[order[i - 1]] : -1, k1 = key[src];
        for (int32_t k = k0 + 1; k <= k1; ++k) start[k] = i;
        if (i == m - 1)
            for (int32_t k = k1 + 1; k <= cells; ++k) start[k] = m;
    }
    for (long long i = 0; i < n; ++i) {
        const MsWalk w = ms_nearest(g, records.data(), start.data(), queries + 3 * i, dist2[i], index[i]);
        if (account) {
            account[2 * i] = w.candidates;
            account[2 * i + 1] = w.shells;
        }
    }
    return 0;
}

double mm_ring_bound2(const float *lo, float cell, const int32_t *dims, const float *q, int r) {
    const MsGrid g = grid(lo, cell, dims);
    int32_t c[3];
    ms_cell(g, q, c);
    return ms_shells_cover(g, c, r) ? INFINITY : ms_ring_bound2(g, q, c, r);
}

int mm_max_cells(void) { return kMsMaxCells; }

}
