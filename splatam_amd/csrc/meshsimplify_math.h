// meshsimplify_math.h -- loop bodies of the mesh simplification layer (meshsimplify.hip), written once as host/device inline functions:
// the kernels call them per lane, tests/test_meshsimplify_cpu.py compiles the very same header with g++
// (tests/meshsimplify_math_shim.cpp, -ffp-contract=off) and checks it against the numpy restatement tests/meshsimplify_ref.py.
//
// Vertex clustering with quadric placement (P. Lindstrom, "Out-of-core simplification of large polygonal models", SIGGRAPH 2000): all
// vertices in one cell of a uniform grid anchored at the WORLD ORIGIN become one vertex, which sits where the summed plane quadrics of
// the faces around the cell are smallest.
//
//   S0 KEY     per coordinate i = floor((double)x / cell): floor, not truncation, so negative coordinates count and x = j cell exactly
//              belongs to cell j (-0 to cell 0, the smallest negative denormal to cell -1).  |i| < 2^20 is required.
//              key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20), an int64 >= 0; -1 for a vertex that is not finite or has an
//              index out of range.  Cluster ids are the ranks of the distinct keys in ascending order (made by the caller: a sort).
//   LOCAL      the cell's centre is (i + 0.5) cell; a vertex's local coordinate is p = ((double)x - centre) / cell, in [-1/2, 1/2) up
//              to one rounding.  Everything below lives in these units: the solve does not depend on where in the world the cell is.
//   S1 SUMS    per cluster, by integer adds: the count (int32) and kSqSums = 16 int64 words: [0..2] the sum of rint(p 2^32), [3..5]
//              the sum of rint(colour 2^32) (a colour that is no number or not below 2^20 in magnitude adds 0), and
//   S2         [6..11] A = sum area n n^T (xx xy xz yy yz zz), [12..14] b = sum area d n, [15] c = sum area d^2, each term as
//              rint(term 2^40): the quanta of meshclean's areas (2^-40 m^2).  Per face n = (b - a) x (c - a) in double as
//              ms_triangle_area forms it, len = |n|, n^ = n / len, area = len / 2.  A face adds nothing when it names a vertex outside
//              0..V-1 or one without a cluster, when len is not > 0, or when area is not below 2^22 m^2 (that raises the refusal flag).
//              For every DISTINCT cluster g among its three, d = n^ . p of the face's first corner in g (local to g's cell): the
//              signed distance, in cells, of the cell's centre from the face's plane, the corner lying on it.  |p_k| <= 1/2, so
//              |d| <= sqrt(3) / 2, every term is bounded by the face's area, and a word holds 2^23 m^2 of faces.  The sums are exact in
//              the quanta and independent of order.
//   S3 PLACE   m = sum p / count.  Eigenvalues l_i and eigenvectors v_i of A by icp_math.h's cyclic Jacobi sweeps; lmax = max |l_i|;
//              p = m + sum over l_i > tau lmax of v_i (v_i . (b - A m)) / l_i, tau = 1e-3: the minimiser of the quadric
//              Q(p) = p^T A p - 2 b^T p + c within the directions the faces constrain, nearest to the mean in the others -- a plane
//              keeps its vertices on it (rank 1), an edge on the edge (rank 2), a corner on the corner (rank 3).  lmax == 0 (no face
//              added anything) or |p_k| > 1/2 for some k (the point leaves its cell): p = m, flagged.  The vertex is
//              centre + p cell in double, rounded once to float32; the colour is the mean, rounded once.  Q(p) is written as it comes
//              out (it may be a few quanta below zero).
//   S4 FACES   g = cluster of the face's three; the face stays when all three exist and are pairwise distinct, renamed and rotated so
//              that the smallest id comes first (the winding is kept); otherwise (-1, -1, -1).
//
// Every double step is an operation of its own (ms_addd / _subd / _muld, icp_divd), so host and device give the same bits.
#pragma once

#include <math.h>
#include <stdint.h>

#include "icp_math.h"
#include "meshclean_math.h"

namespace splat {

constexpr int32_t kSqIndexLimit = 1 << 20;                              // |i| < 2^20 per axis
constexpr double kSqUnitScale = 4294967296.0, kSqUnitQuantum = 1.0 / 4294967296.0;      // 2^32 quanta per cell / per unit of colour
constexpr double kSqColourLimit = 1048576.0;
constexpr int kSqSums = 16, kSqP = 0, kSqColour = 3, kSqA = 6, kSqB = 12, kSqC = 15;
constexpr double kSqTau = 1e-3;

// ---------------------------------------------------------------------------------------------------------------- S0: keys
// the cell of coordinate x; false when x is not finite or the index is out of range
SPLAT_HD bool sq_cell_index(float x, double cell, int32_t &i) {
    const double q = floor(icp_divd((double)x, cell));
    if (!(q > -(double)kSqIndexLimit && q < (double)kSqIndexLimit)) return false;
    i = (int32_t)q;
    return true;
}

SPLAT_HD int64_t sq_key(const float *p, double cell) {
    int32_t i[3];
    for (int k = 0; k < 3; ++k)
        if (!sq_cell_index(p[k], cell, i[k])) return -1;
    return ((int64_t)(i[2] + kSqIndexLimit) << 42) | ((int64_t)(i[1] + kSqIndexLimit) << 21) | (int64_t)(i[0] + kSqIndexLimit);
}

SPLAT_HD int32_t sq_key_index(int64_t key, int k) { return (int32_t)((key >> (21 * k)) & 0x1fffff) - kSqIndexLimit; }

SPLAT_HD double sq_centre(int32_t i, double cell) { return ms_muld(ms_addd((double)i, 0.5), cell); }

// p of a vertex, local to its own cell; false for a vertex without a key
SPLAT_HD bool sq_local(const float *x, double cell, double *p) {
    for (int k = 0; k < 3; ++k) {
        int32_t i;
        if (!sq_cell_index(x[k], cell, i)) return false;
        p[k] = icp_divd(ms_subd((double)x[k], sq_centre(i, cell)), cell);
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- S1: vertex sums
SPLAT_HD int64_t sq_unit_quanta(double p) { return (int64_t)mc_rint(ms_muld(p, kSqUnitScale)); }
SPLAT_HD int64_t sq_colour_quanta(float c) {
    if (!(c > -(float)kSqColourLimit && c < (float)kSqColourLimit)) return 0;
    return sq_unit_quanta((double)c);
}

// the six words a vertex adds to its cluster ([kSqP .. kSqColour + 2]; colour may be NULL); false when it has no key
SPLAT_HD bool sq_vertex_terms(const float *x, const float *colour, double cell, int64_t *t) {
    double p[3];
    if (!sq_local(x, cell, p)) return false;
    for (int k = 0; k < 3; ++k) {
        t[kSqP + k] = sq_unit_quanta(p[k]);
        t[kSqColour + k] = colour ? sq_colour_quanta(colour[k]) : 0;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- S2: quadrics
SPLAT_HD int64_t sq_area_quanta(double x) { return (int64_t)mc_rint(ms_muld(x, kMcAreaScale)); }

// What face f adds: g[k] is the cluster slot k adds to and t[k] its ten words [kSqA .. kSqC]; g[k] = -1 for a slot that adds nothing
// (slot k is the face's corner k, live when its cluster differs from those of the corners before it).  d[k]: the distance used.
// Returns the number of live slots; *refused is set for a face whose area is beyond the range.
SPLAT_HD int sq_face_terms(const float *vertices, int32_t V, const int32_t *f, const int32_t *cluster, double cell, int32_t *g,
                           int64_t (*t)[10], double *d, int32_t *refused) {
    g[0] = g[1] = g[2] = -1;
    if (!ms_face_valid(f, V)) return 0;
    const int32_t c0 = cluster[f[0]], c1 = cluster[f[1]], c2 = cluster[f[2]];
    if (c0 < 0 || c0 >= V || c1 < 0 || c1 >= V || c2 < 0 || c2 >= V) return 0;
    const float *a = vertices + 3 * (int64_t)f[0], *b = vertices + 3 * (int64_t)f[1], *c = vertices + 3 * (int64_t)f[2];
    double e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = ms_subd((double)b[k], (double)a[k]);
        e2[k] = ms_subd((double)c[k], (double)a[k]);
    }
    double n[3];
    n[0] = ms_subd(ms_muld(e1[1], e2[2]), ms_muld(e1[2], e2[1]));
    n[1] = ms_subd(ms_muld(e1[2], e2[0]), ms_muld(e1[0], e2[2]));
    n[2] = ms_subd(ms_muld(e1[0], e2[1]), ms_muld(e1[1], e2[0]));
    const double len = ms_sqrtd(ms_addd(ms_addd(ms_muld(n[0], n[0]), ms_muld(n[1], n[1])), ms_muld(n[2], n[2])));
    if (!(len > 0.0)) return 0;
    const double area = ms_muld(0.5, len);
    if (!(area < kMcFaceAreaLimit)) {
        *refused = 1;
        return 0;
    }
    double w[3];
    for (int k = 0; k < 3; ++k) {
        n[k] = icp_divd(n[k], len);
        w[k] = ms_muld(area, n[k]);
    }
    const int32_t cs[3] = {c0, c1, c2};
    const bool live[3] = {true, c1 != c0, c2 != c0 && c2 != c1};
    int slots = 0;
    for (int k = 0; k < 3; ++k) {
        double p[3];
        if (!live[k] || !sq_local(vertices + 3 * (int64_t)f[k], cell, p)) continue;
        const double dk = ms_addd(ms_addd(ms_muld(n[0], p[0]), ms_muld(n[1], p[1])), ms_muld(n[2], p[2]));
        int64_t *q = t[k];
        q[0] = sq_area_quanta(ms_muld(w[0], n[0]));
        q[1] = sq_area_quanta(ms_muld(w[0], n[1]));
        q[2] = sq_area_quanta(ms_muld(w[0], n[2]));
        q[3] = sq_area_quanta(ms_muld(w[1], n[1]));
        q[4] = sq_area_quanta(ms_muld(w[1], n[2]));
        q[5] = sq_area_quanta(ms_muld(w[2], n[2]));
        for (int j = 0; j < 3; ++j) q[6 + j] = sq_area_quanta(ms_muld(w[j], dk));
        q[9] = sq_area_quanta(ms_muld(ms_muld(area, dk), dk));
        g[k] = cs[k];
        d[k] = dk;
        ++slots;
    }
    return slots;
}

// ---------------------------------------------------------------------------------------------------------------- S3: placement
// One cluster, from its count (> 0) and its kSqSums words: p [3], the point local to the cell (double); colour [3] (may be NULL); *rank
// (the directions the quadric fixed: 0 with the mean), *fallback (1 when the quadric was asked for and the mean was taken), *value (Q
// at the point).
SPLAT_HD void sq_solve(int32_t count, const int64_t *sums, bool quadric, double *p, float *colour, int32_t *rank, int32_t *fallback,
                       double *value) {
    *rank = *fallback = 0;
    *value = 0.0;
    const double n = (double)count;
    double m[3];
    for (int k = 0; k < 3; ++k) {
        m[k] = icp_divd(ms_muld((double)sums[kSqP + k], kSqUnitQuantum), n);
        p[k] = m[k];
        if (colour) colour[k] = (float)icp_divd(ms_muld((double)sums[kSqColour + k], kSqUnitQuantum), n);
    }
    if (quadric) {
        const double xx = ms_muld((double)sums[kSqA], kMcAreaQuantum), xy = ms_muld((double)sums[kSqA + 1], kMcAreaQuantum),
                     xz = ms_muld((double)sums[kSqA + 2], kMcAreaQuantum), yy = ms_muld((double)sums[kSqA + 3], kMcAreaQuantum),
                     yz = ms_muld((double)sums[kSqA + 4], kMcAreaQuantum), zz = ms_muld((double)sums[kSqA + 5], kMcAreaQuantum);
        const double A0[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}};
        double b[3], A[3][3], E[3][3];
        for (int i = 0; i < 3; ++i) {
            b[i] = ms_muld((double)sums[kSqB + i], kMcAreaQuantum);
            for (int j = 0; j < 3; ++j) A[i][j] = A0[i][j];
        }
        const double c = ms_muld((double)sums[kSqC], kMcAreaQuantum);
        icp_jacobi<3>(A, E);
        double lmax = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double l = A[i][i] < 0.0 ? -A[i][i] : A[i][i];
            lmax = l > lmax ? l : lmax;
        }
        if (!(lmax > 0.0)) {
            *fallback = 1;
        } else {
            double r[3];
            for (int i = 0; i < 3; ++i)
                r[i] = ms_subd(b[i], ms_addd(ms_addd(ms_muld(A0[i][0], m[0]), ms_muld(A0[i][1], m[1])), ms_muld(A0[i][2], m[2])));
            const double least = ms_muld(kSqTau, lmax);
            int used = 0;
            for (int i = 0; i < 3; ++i) {
                if (!(A[i][i] > least)) continue;
                const double dot = ms_addd(ms_addd(ms_muld(E[0][i], r[0]), ms_muld(E[1][i], r[1])), ms_muld(E[2][i], r[2]));
                const double s = icp_divd(dot, A[i][i]);
                for (int k = 0; k < 3; ++k) p[k] = ms_addd(p[k], ms_muld(E[k][i], s));
                ++used;
            }
            bool inside = true;
            for (int k = 0; k < 3; ++k) inside = inside && p[k] >= -0.5 && p[k] <= 0.5;
            if (inside) {
                *rank = used;
            } else {
                *fallback = 1;
                for (int k = 0; k < 3; ++k) p[k] = m[k];
            }
        }
        double Ap[3];
        for (int i = 0; i < 3; ++i) Ap[i] = ms_addd(ms_addd(ms_muld(A0[i][0], p[0]), ms_muld(A0[i][1], p[1])), ms_muld(A0[i][2], p[2]));
        const double pAp = ms_addd(ms_addd(ms_muld(p[0], Ap[0]), ms_muld(p[1], Ap[1])), ms_muld(p[2], Ap[2]));
        const double bp = ms_addd(ms_addd(ms_muld(b[0], p[0]), ms_muld(b[1], p[1])), ms_muld(b[2], p[2]));
        *value = ms_addd(ms_subd(pAp, ms_muld(2.0, bp)), c);
    }
}

// ... and its vertex: centre + p cell in double, rounded once.  A cluster without a vertex (count <= 0 or key < 0) gives zeros.
SPLAT_HD void sq_place(int32_t count, const int64_t *sums, int64_t key, double cell, bool quadric, float *position, float *colour, int32_t *rank,
                       int32_t *fallback, double *value) {
    if (count <= 0 || key < 0) {
        *rank = *fallback = 0;
        *value = 0.0;
        for (int k = 0; k < 3; ++k) {
            position[k] = 0.f;
            if (colour) colour[k] = 0.f;
        }
        return;
    }
    double p[3];
    sq_solve(count, sums, quadric, p, colour, rank, fallback, value);
    for (int k = 0; k < 3; ++k) position[k] = (float)ms_addd(sq_centre(sq_key_index(key, k), cell), ms_muld(p[k], cell));
}

// ---------------------------------------------------------------------------------------------------------------- S4: faces
SPLAT_HD bool sq_face_triple(const int32_t *f, int32_t V, const int32_t *cluster, int32_t *tri) {
    tri[0] = tri[1] = tri[2] = -1;
    if (!ms_face_valid(f, V)) return false;
    const int32_t a = cluster[f[0]], b = cluster[f[1]], c = cluster[f[2]];
    if (a < 0 || b < 0 || c < 0 || a == b || b == c || a == c) return false;
    if (a < b && a < c) {
        tri[0] = a; tri[1] = b; tri[2] = c;
    } else if (b < c) {
        tri[0] = b; tri[1] = c; tri[2] = a;
    } else {
        tri[0] = c; tri[1] = a; tri[2] = b;
    }
    return true;
}

}  // namespace splat
