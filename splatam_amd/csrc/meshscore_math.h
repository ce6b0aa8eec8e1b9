// meshscore_math.h -- arithmetic of the mesh score layer (meshscore.hip), written once as host/device inline functions: the kernels
// call them per lane, tests/test_meshscore_cpu.py compiles the very same header with g++ (tests/meshscore_math_shim.cpp,
// -ffp-contract=off) and checks it against the numpy restatement tests/meshscore_ref.py.
//
//   GENERATOR  ms_uniform3(seed, i): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11;
//              TEN rounds, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85) of the counter
//              (i low, i high, 0, 0) under the key (seed low, seed high); words 0, 1, 2 of the output, each as (word >> 8) 2^-24:
//              three floats in [0, 1), exact.  No state: sample i is the same whatever the launch shape and whatever n.
//   AREA       of a triangle of float32 vertices, in double: e1 = b - a, e2 = c - a (the float32 values widened first),
//              n = e1 x e2 with each component one product minus one product, area = 0.5 sqrt((nx nx + ny ny) + nz nz).  A triangle
//              with an index outside 0..V-1 or an area that is not > 0 (NaN included) has area 0.
//   SAMPLE i   (u0, u1, u2) = ms_uniform3(seed, i).  t = (double)u0 * total, total the last element of the INCLUSIVE double prefix
//              sum of the areas; the triangle is the first whose prefix exceeds t (binary search; a zero-area triangle's prefix
//              equals its predecessor's, so it is never the first).  When u1 + u2 > 1 (float32 sum) both are folded: u1 = 1 - u1,
//              u2 = 1 - u2.  The point is, per coordinate and in float32, (a + u1 (b - a)) + u2 (c - a).
//   GRID       (lo[3], cell, dims[3]): the cell of p is floor((p - lo) / cell) per axis (float32 subtraction, float32 division),
//              clamped into 0..dims-1, so every point has a cell and the outermost cells reach to infinity.  key = (z dimy + y) dimx + x.
//   DISTANCE   d2 = (dx dx + dy dy) + dz dz in float32, d = q - p.  The nearest target is the one of least d2, the LOWEST ORIGINAL
//              INDEX among equals.
//   RING BOUND after the Chebyshev shells 0..r around the query's (clamped) cell c have been searched, every unsearched target has a
//              cell index <= c - r - 1 or >= c + r + 1 on some axis, so (the cell assignment being two float32 roundings of the true
//              quotient) it lies beyond the plane lo + k cell (1 -+ 4 2^-24), k = c - r resp. c + r + 1, of that axis.  Sides where the
//              shells have reached the grid's edge hold no unsearched target.  The bound b is the least of the query's distances to
//              the remaining planes, formed in double with the planes moved TOWARDS the query by the margin 4 2^-24 k cell, and 0
//              when one of them is negative (the query outside the box) or at most 1e-15 (below that a float32 square can underflow
//              to a tie at 0).  A float32 d2 of a target at true distance >= b is at least
//              b^2 (1 - 2^-20) (one rounding per difference, per square and per add is below 6 2^-24 relative): the search stops
//              only when best_d2 < b^2 (1 - 2^-20), a strict inequality, so an unsearched target can neither beat the best nor tie
//              with it at a lower index; or when the shells cover the grid.
//   REDUCE     a distance is sqrt((double)d2), correctly rounded.
//
// Every float32 step is an operation of its own (ms_add / _sub / _mul / _div, and their double forms: operators under
// `#pragma clang fp contract(off)` on the device, plain operators under -ffp-contract=off on the host), so a result does not depend on
// what a compiler contracts.
#pragma once

#include <math.h>
#include <stdint.h>

#include "splat_math.h"

namespace splat {

#if defined(__HIP_DEVICE_COMPILE__)
SPLAT_HD float ms_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
SPLAT_HD float ms_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
SPLAT_HD float ms_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
SPLAT_HD float ms_div(float a, float b) { return __fdiv_rn(a, b); }
SPLAT_HD double ms_addd(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
SPLAT_HD double ms_subd(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
SPLAT_HD double ms_muld(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
SPLAT_HD double ms_sqrtd(double a) { return __dsqrt_rn(a); }
#else
SPLAT_HD float ms_add(float a, float b) { return a + b; }
SPLAT_HD float ms_sub(float a, float b) { return a - b; }
SPLAT_HD float ms_mul(float a, float b) { return a * b; }
SPLAT_HD float ms_div(float a, float b) { return a / b; }
SPLAT_HD double ms_addd(double a, double b) { return a + b; }
SPLAT_HD double ms_subd(double a, double b) { return a - b; }
SPLAT_HD double ms_muld(double a, double b) { return a * b; }
SPLAT_HD double ms_sqrtd(double a) { return sqrt(a); }
#endif

constexpr int kMsMaxCells = 1 << 21;                        // a grid has at most this many cells: the walk of a stray query is bounded by it
constexpr double kMsPlaneMargin = 4.0 / 16777216.0;         // 4 2^-24, relative to k cell: the two roundings of the cell assignment, doubled
constexpr double kMsDistMargin = 1.0 / 1048576.0;           // 2^-20, relative to b^2: the roundings of a float32 d2, with room
constexpr double kMsMinBound = 1e-15;                       // a bound at or below this counts as 0: below it a float32 square may underflow

// ---------------------------------------------------------------------------------------------------------------- generator
SPLAT_HD void ms_philox4x32_10(uint64_t seed, uint64_t i, uint32_t out[4]) {
    uint32_t c0 = (uint32_t)i, c1 = (uint32_t)(i >> 32), c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

SPLAT_HD void ms_uniform3(uint64_t seed, uint64_t i, float u[3]) {
    uint32_t w[4];
    ms_philox4x32_10(seed, i, w);
    for (int c = 0; c < 3; ++c) u[c] = (float)(w[c] >> 8) * (1.0f / 16777216.0f);       // (24 bits times 2^-24: exact)
}

// ---------------------------------------------------------------------------------------------------------------- area, sample
SPLAT_HD bool ms_face_valid(const int32_t *f, int32_t V) {
    return f[0] >= 0 && f[0] < V && f[1] >= 0 && f[1] < V && f[2] >= 0 && f[2] < V;
}

SPLAT_HD double ms_triangle_area(const float *a, const float *b, const float *c) {
    double e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = ms_subd((double)b[k], (double)a[k]);
        e2[k] = ms_subd((double)c[k], (double)a[k]);
    }
    const double nx = ms_subd(ms_muld(e1[1], e2[2]), ms_muld(e1[2], e2[1]));
    const double ny = ms_subd(ms_muld(e1[2], e2[0]), ms_muld(e1[0], e2[2]));
    const double nz = ms_subd(ms_muld(e1[0], e2[1]), ms_muld(e1[1], e2[0]));
    const double area = ms_muld(0.5, ms_sqrtd(ms_addd(ms_addd(ms_muld(nx, nx), ms_muld(ny, ny)), ms_muld(nz, nz))));
    return area > 0.0 ? area : 0.0;
}

SPLAT_HD double ms_face_area(const float *vertices, int32_t V, const int32_t *f) {
    if (!ms_face_valid(f, V)) return 0.0;
    return ms_triangle_area(vertices + 3 * (int64_t)f[0], vertices + 3 * (int64_t)f[1], vertices + 3 * (int64_t)f[2]);
}

// the first of F prefix sums that exceeds t (F when none does)
SPLAT_HD int32_t ms_pick(const double *prefix, int32_t F, double t) {
    int32_t lo = 0, hi = F;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// sample i of the surface; returns the triangle, -1 (and the point 0) for a mesh without area or a triangle that names no vertex
SPLAT_HD int32_t ms_sample(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const double *prefix, uint64_t seed, uint64_t i,
                           float *p) {
    float u[3];
    ms_uniform3(seed, i, u);
    p[0] = p[1] = p[2] = 0.f;
    if (F <= 0) return -1;
    const int32_t f = ms_pick(prefix, F, ms_muld((double)u[0], prefix[F - 1]));
    if (f >= F || !ms_face_valid(faces + 3 * (int64_t)f, V)) return -1;
    float u1 = u[1], u2 = u[2];
    if (ms_add(u1, u2) > 1.0f) {
        u1 = ms_sub(1.0f, u1);
        u2 = ms_sub(1.0f, u2);
    }
    const float *a = vertices + 3 * (int64_t)faces[3 * (int64_t)f], *b = vertices + 3 * (int64_t)faces[3 * (int64_t)f + 1],
                *c = vertices + 3 * (int64_t)faces[3 * (int64_t)f + 2];
    for (int k = 0; k < 3; ++k) p[k] = ms_add(ms_add(a[k], ms_mul(u1, ms_sub(b[k], a[k]))), ms_mul(u2, ms_sub(c[k], a[k])));
    return f;
}

// ---------------------------------------------------------------------------------------------------------------- grid
struct MsGrid {
    float lo[3], cell;
    int32_t dims[3];
    int32_t count;                      // targets: no record is read at or beyond it, whatever the start table holds
};
struct alignas(16) MsRecord {          // a sorted target: one 16-byte load per candidate
    float x, y, z;
    int32_t index;                      // its original index
};

SPLAT_HD bool ms_grid_valid(const MsGrid &g) {
    if (!(g.cell > 0.f) || !(g.cell < INFINITY) || g.dims[0] <= 0 || g.dims[1] <= 0 || g.dims[2] <= 0) return false;
    if (!(g.lo[0] - g.lo[0] == 0.f) || !(g.lo[1] - g.lo[1] == 0.f) || !(g.lo[2] - g.lo[2] == 0.f)) return false;      // (finite)
    return (int64_t)g.dims[0] * g.dims[1] <= kMsMaxCells && (int64_t)g.dims[0] * g.dims[1] * (int64_t)g.dims[2] <= kMsMaxCells;
}
SPLAT_HD int32_t ms_cells(const MsGrid &g) { return g.dims[0] * g.dims[1] * g.dims[2]; }

SPLAT_HD void ms_cell(const MsGrid &g, const float *p, int32_t *c) {
    for (int k = 0; k < 3; ++k) {
        const float t = floorf(ms_div(ms_sub(p[k], g.lo[k]), g.cell));
        c[k] = !(t >= 0.f) ? 0 : (t >= (float)g.dims[k] ? g.dims[k] - 1 : (int32_t)t);          // (NaN: cell 0)
    }
}
SPLAT_HD int32_t ms_key(const MsGrid &g, const int32_t *c) { return (c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0]; }

SPLAT_HD float ms_dist2(const float *q, float x, float y, float z) {
    const float dx = ms_sub(q[0], x), dy = ms_sub(q[1], y), dz = ms_sub(q[2], z);
    return ms_add(ms_add(ms_mul(dx, dx), ms_mul(dy, dy)), ms_mul(dz, dz));
}

SPLAT_HD bool ms_shells_cover(const MsGrid &g, const int32_t *c, int r) {
    return c[0] - r <= 0 && c[0] + r >= g.dims[0] - 1 && c[1] - r <= 0 && c[1] + r >= g.dims[1] - 1 && c[2] - r <= 0 && c[2] + r >= g.dims[2] - 1;
}

// what a float32 d2 of any target outside the box of cells b0 .. b1 (inclusive, inside the grid) is at least (RING BOUND above, the box
// being any box that holds the query's cell); +inf when the box is the grid
SPLAT_HD double ms_box_bound2(const MsGrid &g, const float *q, const int32_t *b0, const int32_t *b1) {
    double b = INFINITY;
    for (int k = 0; k < 3; ++k) {
        const double lo = (double)g.lo[k], cell = (double)g.cell, x = (double)q[k];
        if (b0[k] > 0) {                                                // targets of cells <= b0 - 1 lie below this plane
            const double off = (double)b0[k] * cell;
            const double d = x - (lo + off + kMsPlaneMargin * off);
            b = d < b ? d : b;
        }
        if (b1[k] < g.dims[k] - 1) {                                    // targets of cells >= b1 + 1 lie at or above this one
            const double off = (double)(b1[k] + 1) * cell;
            const double d = (lo + off - kMsPlaneMargin * off) - x;
            b = d < b ? d : b;
        }
    }
    if (b == INFINITY) return INFINITY;
    if (!(b > kMsMinBound)) return 0.0;
    return b * b * (1.0 - kMsDistMargin);
}

// ... outside the shells 0..r around c
SPLAT_HD double ms_ring_bound2(const MsGrid &g, const float *q, const int32_t *c, int r) {
    int32_t b0[3], b1[3];
    for (int k = 0; k < 3; ++k) {
        b0[k] = c[k] - r < 0 ? 0 : c[k] - r;
        b1[k] = c[k] + r > g.dims[k] - 1 ? g.dims[k] - 1 : c[k] + r;
    }
    return ms_box_bound2(g, q, b0, b1);
}

struct MsWalk {                         // the account of one query's search
    int32_t candidates, shells;
};

SPLAT_HD void ms_scan(const MsRecord *records, int32_t count, int32_t begin, int32_t end, const float *q, float &best_d2, int32_t &best_index,
                      MsWalk &w) {
    begin = begin < 0 ? 0 : begin;
    end = end > count ? count : end;
    if (end <= begin) return;
    for (int32_t s = begin; s < end; ++s) {
        const MsRecord t = records[s];
        const float d2 = ms_dist2(q, t.x, t.y, t.z);
        if (d2 < best_d2 || (d2 == best_d2 && t.index < best_index)) {
            best_d2 = d2;
            best_index = t.index;
        }
    }
    w.candidates += end - begin;
}

// the nearest of the grid's targets to q: shells outward over the clipped grid; a row of a shell's faces along x is one contiguous
// range of the sorted records (x is the fastest axis of the key).  best_index stays -1 (best_d2 +inf) when no d2 compares (an empty
// grid, a NaN query).
SPLAT_HD MsWalk ms_nearest(const MsGrid &g, const MsRecord *records, const int32_t *start, const float *q, float &best_d2, int32_t &best_index) {
    int32_t c[3];
    ms_cell(g, q, c);
    best_d2 = INFINITY;
    best_index = -1;
    int32_t tie = INT32_MAX;            // (best_index for the comparison: any real index beats "none")
    MsWalk w = {0, 0};
    for (int r = 0;; ++r) {
        const int z0 = c[2] - r < 0 ? 0 : c[2] - r, z1 = c[2] + r > g.dims[2] - 1 ? g.dims[2] - 1 : c[2] + r;
        const int y0 = c[1] - r < 0 ? 0 : c[1] - r, y1 = c[1] + r > g.dims[1] - 1 ? g.dims[1] - 1 : c[1] + r;
        const int x0 = c[0] - r < 0 ? 0 : c[0] - r, x1 = c[0] + r > g.dims[0] - 1 ? g.dims[0] - 1 : c[0] + r;
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int32_t row = (z * g.dims[1] + y) * g.dims[0];
                if (z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r) {
                    ms_scan(records, g.count, start[row + x0], start[row + x1 + 1], q, best_d2, tie, w);
                } else {                                                // (r > 0 here: at r = 0 the one row is a face)
                    if (c[0] - r >= 0) ms_scan(records, g.count, start[row + c[0] - r], start[row + c[0] - r + 1], q, best_d2, tie, w);
                    if (c[0] + r <= g.dims[0] - 1) ms_scan(records, g.count, start[row + c[0] + r], start[row + c[0] + r + 1], q, best_d2, tie, w);
                }
            }
        w.shells = r + 1;
        if (ms_shells_cover(g, c, r)) break;
        if ((double)best_d2 < ms_ring_bound2(g, q, c, r)) break;
    }
    if (tie != INT32_MAX) best_index = tie;
    return w;
}

}  // namespace splat
