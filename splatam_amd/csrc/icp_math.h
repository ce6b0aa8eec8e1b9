// icp_math.h -- arithmetic of the ICP layer (icp.hip), written once as host/device inline functions: the kernels call them per lane,
// tests/test_icp_cpu.py compiles the very same header with g++ (tests/icp_math_shim.cpp, -ffp-contract=off) and checks it against
// numpy.  Everything is double; every step is an operation of its own (ms_addd / _subd / _muld of meshscore_math.h), so a result does
// not depend on what a compiler contracts.
//
//   STATE      SPLAT_ICP_STATE doubles: T [16] row-major (bottom row 0 0 0 1), then kIcpIteration, kIcpStatus (0 running, 1 converged,
//              2 iteration limit, 3 fewer than three correspondences), kIcpFitness / kIcpRmse of the current evaluation,
//              kIcpPrevFitness / kIcpPrevRmse of the one before, kIcpCount (correspondences of the current evaluation), kIcpPoints (n).
//   MOVE       p' = R p + t per row as ((r0 x + r1 y) + r2 z) + t, the float32 point widened first.
//   SUMS       SPLAT_ICP_SUMS = 17 doubles over the correspondences: count, sum of d^2, sum of (p' - c) [3], sum of (q - c) [3], sum of
//              (p' - c)(q - c)^T [9] (row: the component of p', column: that of q).  c is an origin near the points: it only limits
//              cancellation, the solve does not depend on it beyond rounding.
//   SOLVE      from the sums: centroids a = Sp / N, b = Sq / N, cross-covariance M = Spq - Sp Sq^T / N; the proper rotation U that
//              maximises trace(U M) -- i.e. minimises sum |U (p' - a) - (q - b)|^2 -- by Horn's closed form (B. K. P. Horn, "Closed-form
//              solution of absolute orientation using unit quaternions", JOSA A 4(4), 1987): the unit eigenvector (w, x, y, z) of the
//              LARGEST eigenvalue of the symmetric
//                  [ Mxx+Myy+Mzz   Myz-Mzy       Mzx-Mxz       Mxy-Myx     ]
//                  [ .             Mxx-Myy-Mzz   Mxy+Myx       Mzx+Mxz     ]
//                  [ .             .            -Mxx+Myy-Mzz   Myz+Mzy     ]
//                  [ .             .             .            -Mxx-Myy+Mzz ]
//              found by cyclic Jacobi sweeps (rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), each annihilating one off-diagonal
//              element, until all are exactly zero or below 2^-200 of the matrix's scale squared; at most kIcpMaxSweeps).  A unit
//              quaternion is a proper rotation whatever the sums: planar, collinear and reflection-prone clouds need no determinant
//              fix (a collinear cloud's two largest eigenvalues are equal: any vector of their plane is a minimiser, Jacobi returns
//              one).  Among equal eigenvalues the first column wins, so M = 0 gives the identity.  The translation is
//              (c + b) - U (c + a).
//   UPDATE     T <- U T: the rotation block U R, the translation U t + u.
#pragma once

#include <math.h>
#include <stdint.h>

#include "meshscore_math.h"

namespace splat {

constexpr int kIcpIteration = 16, kIcpStatus = 17, kIcpFitness = 18, kIcpRmse = 19, kIcpPrevFitness = 20, kIcpPrevRmse = 21, kIcpCount = 22,
              kIcpPoints = 23;
constexpr int kIcpSums = 17;
constexpr int kIcpMaxSweeps = 60;

#if defined(__HIP_DEVICE_COMPILE__)
SPLAT_HD double icp_divd(double a, double b) { return __ddiv_rn(a, b); }
#else
SPLAT_HD double icp_divd(double a, double b) { return a / b; }
#endif

// R p + t of row-major T [16] (its first three rows), the point widened to double first
SPLAT_HD void icp_move(const double *T, const float *p, double *out) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    for (int r = 0; r < 3; ++r)
        out[r] = ms_addd(ms_addd(ms_addd(ms_muld(T[4 * r], x), ms_muld(T[4 * r + 1], y)), ms_muld(T[4 * r + 2], z)), T[4 * r + 3]);
}

// a correspondence's contribution to the 17 sums: p' (double), its target q (float32), d2 the float32 squared distance of the search
SPLAT_HD void icp_add_terms(double *acc, const double *pm, const float *q, float d2, const double *c) {
    double a[3], b[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = ms_subd(pm[k], c[k]);
        b[k] = ms_subd((double)q[k], c[k]);
    }
    acc[0] = ms_addd(acc[0], 1.0);
    acc[1] = ms_addd(acc[1], (double)d2);
    for (int k = 0; k < 3; ++k) {
        acc[2 + k] = ms_addd(acc[2 + k], a[k]);
        acc[5 + k] = ms_addd(acc[5 + k], b[k]);
    }
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) acc[8 + 3 * r + k] = ms_addd(acc[8 + 3 * r + k], ms_muld(a[r], b[k]));
}

// eigenvalues (the diagonal of A afterwards) and eigenvectors (the columns of V) of the symmetric N x N A, by cyclic Jacobi sweeps
// (the 4 x 4 of Horn's form here, the 3 x 3 of a cluster's quadric in meshsimplify_math.h)
template <int N>
SPLAT_HD void icp_jacobi(double (*A)[N], double (*V)[N]) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    double scale = 0.0;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) scale = ms_addd(scale, ms_muld(A[i][j], A[i][j]));
    const double tiny = ms_muld(scale, 6.223015277861142e-61);          // 2^-200 of the squared Frobenius norm
    for (int sweep = 0; sweep < kIcpMaxSweeps; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < N; ++i)
            for (int j = i + 1; j < N; ++j) off = ms_addd(off, ms_muld(A[i][j], A[i][j]));
        if (!(off > tiny)) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                // t = tan of the rotation angle, the smaller root of t^2 + 2 theta t - 1 = 0, theta = (aqq - app) / (2 apq)
                const double theta = icp_divd(ms_subd(A[q][q], A[p][p]), ms_muld(2.0, apq));
                const double root = ms_sqrtd(ms_addd(ms_muld(theta, theta), 1.0));
                const double t = theta >= 0.0 ? icp_divd(1.0, ms_addd(theta, root)) : icp_divd(-1.0, ms_subd(root, theta));
                const double cs = icp_divd(1.0, ms_sqrtd(ms_addd(ms_muld(t, t), 1.0))), sn = ms_muld(t, cs);
                for (int k = 0; k < N; ++k) {                           // A <- A J (columns p, q)
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = ms_subd(ms_muld(cs, akp), ms_muld(sn, akq));
                    A[k][q] = ms_addd(ms_muld(sn, akp), ms_muld(cs, akq));
                }
                for (int k = 0; k < N; ++k) {                           // A <- J^T A (rows p, q)
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = ms_subd(ms_muld(cs, apk), ms_muld(sn, aqk));
                    A[q][k] = ms_addd(ms_muld(sn, apk), ms_muld(cs, aqk));
                }
                A[p][q] = A[q][p] = 0.0;
                for (int k = 0; k < N; ++k) {                           // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = ms_subd(ms_muld(cs, vkp), ms_muld(sn, vkq));
                    V[k][q] = ms_addd(ms_muld(sn, vkp), ms_muld(cs, vkq));
                }
            }
    }
}

SPLAT_HD void icp_jacobi4(double A[4][4], double V[4][4]) { icp_jacobi<4>(A, V); }

// the proper rotation U [9] row-major that maximises trace(U M), M [9] row-major = sum (p - a)(q - b)^T
SPLAT_HD void icp_horn(const double *M, double *U) {
    const double xx = M[0], xy = M[1], xz = M[2], yx = M[3], yy = M[4], yz = M[5], zx = M[6], zy = M[7], zz = M[8];
    double A[4][4], V[4][4];
    A[0][0] = ms_addd(ms_addd(xx, yy), zz);
    A[1][1] = ms_subd(ms_subd(xx, yy), zz);
    A[2][2] = ms_subd(ms_subd(yy, xx), zz);
    A[3][3] = ms_subd(ms_subd(zz, xx), yy);
    A[0][1] = A[1][0] = ms_subd(yz, zy);
    A[0][2] = A[2][0] = ms_subd(zx, xz);
    A[0][3] = A[3][0] = ms_subd(xy, yx);
    A[1][2] = A[2][1] = ms_addd(xy, yx);
    A[1][3] = A[3][1] = ms_addd(zx, xz);
    A[2][3] = A[3][2] = ms_addd(yz, zy);
    icp_jacobi4(A, V);
    int best = 0;
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > A[best][best]) best = k;
    double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
    const double norm = ms_sqrtd(ms_addd(ms_addd(ms_addd(ms_muld(w, w), ms_muld(x, x)), ms_muld(y, y)), ms_muld(z, z)));
    if (!(norm > 0.0) || !(norm < INFINITY)) {                          // (sums that are not numbers: leave the pose where it is)
        w = 1.0; x = y = z = 0.0;
    } else {
        w = icp_divd(w, norm); x = icp_divd(x, norm); y = icp_divd(y, norm); z = icp_divd(z, norm);
    }
    const double ww = ms_muld(w, w), xx2 = ms_muld(x, x), yy2 = ms_muld(y, y), zz2 = ms_muld(z, z);
    const double wx = ms_muld(w, x), wy = ms_muld(w, y), wz = ms_muld(w, z), xy2 = ms_muld(x, y), xz2 = ms_muld(x, z), yz2 = ms_muld(y, z);
    U[0] = ms_subd(ms_subd(ms_addd(ww, xx2), yy2), zz2);
    U[1] = ms_muld(2.0, ms_subd(xy2, wz));
    U[2] = ms_muld(2.0, ms_addd(xz2, wy));
    U[3] = ms_muld(2.0, ms_addd(xy2, wz));
    U[4] = ms_subd(ms_addd(ms_subd(ww, xx2), yy2), zz2);
    U[5] = ms_muld(2.0, ms_subd(yz2, wx));
    U[6] = ms_muld(2.0, ms_subd(xz2, wy));
    U[7] = ms_muld(2.0, ms_addd(yz2, wx));
    U[8] = ms_addd(ms_subd(ms_subd(ww, xx2), yy2), zz2);
}

// the rigid motion (U [9], u [3]) that best takes the correspondences' p' onto their q, from the 17 sums about the origin c (count >= 1)
SPLAT_HD void icp_solve_sums(const double *sums, const double *c, double *U, double *u) {
    const double n = sums[0];
    double a[3], b[3], M[9];
    for (int k = 0; k < 3; ++k) {
        a[k] = icp_divd(sums[2 + k], n);
        b[k] = icp_divd(sums[5 + k], n);
    }
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) M[3 * r + k] = ms_subd(sums[8 + 3 * r + k], ms_muld(sums[2 + r], b[k]));
    icp_horn(M, U);
    for (int r = 0; r < 3; ++r) {
        const double pa[3] = {ms_addd(c[0], a[0]), ms_addd(c[1], a[1]), ms_addd(c[2], a[2])};
        const double moved = ms_addd(ms_addd(ms_muld(U[3 * r], pa[0]), ms_muld(U[3 * r + 1], pa[1])), ms_muld(U[3 * r + 2], pa[2]));
        u[r] = ms_subd(ms_addd(c[r], b[r]), moved);
    }
}

// T <- (U, u) T
SPLAT_HD void icp_compose(double *T, const double *U, const double *u) {
    double out[12];
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 4; ++k)
            out[4 * r + k] = ms_addd(ms_addd(ms_muld(U[3 * r], T[k]), ms_muld(U[3 * r + 1], T[4 + k])), ms_muld(U[3 * r + 2], T[8 + k]));
        out[4 * r + 3] = ms_addd(out[4 * r + 3], u[r]);
    }
    for (int k = 0; k < 12; ++k) T[k] = out[k];
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

// one evaluation of the loop from the 17 sums of iteration state[kIcpIteration] over n points: fitness, inlier RMSE, the history row,
// the stop (Open3D's: both changed by less than the relative_* since the evaluation before), and -- while running -- the update.
// history may be NULL.  Does nothing once the status is set: T is frozen.
SPLAT_HD void icp_step(double *state, const double *sums, long long n, int32_t max_iterations, double relative_fitness, double relative_rmse,
                       const double *c, double *history) {
    if (state[kIcpStatus] != 0.0) return;
    const double count = sums[0];
    const double fitness = count > 0.0 && n > 0 ? icp_divd(count, (double)n) : 0.0;
    const double rmse = count > 0.0 ? ms_sqrtd(icp_divd(sums[1], count)) : 0.0;
    const double it = state[kIcpIteration];
    double status = 0.0;
    const double df = ms_subd(fitness, state[kIcpPrevFitness]), dr = ms_subd(rmse, state[kIcpPrevRmse]);
    if (it > 0.0 && (df < 0.0 ? -df : df) < relative_fitness && (dr < 0.0 ? -dr : dr) < relative_rmse) status = 1.0;
    else if (!(it < (double)max_iterations)) status = 2.0;
    else if (count < 3.0) status = 3.0;
    state[kIcpFitness] = fitness;
    state[kIcpRmse] = rmse;
    state[kIcpCount] = count;
    state[kIcpPoints] = (double)n;
    state[kIcpStatus] = status;
    if (history && it >= 0.0 && it <= (double)max_iterations) {
        double *row = history + 4 * (long long)it;
        row[0] = count; row[1] = fitness; row[2] = rmse; row[3] = status;
    }
    if (status != 0.0) return;
    double U[9], u[3];
    icp_solve_sums(sums, c, U, u);
    icp_compose(state, U, u);
    state[kIcpPrevFitness] = fitness;
    state[kIcpPrevRmse] = rmse;
    state[kIcpIteration] = ms_addd(it, 1.0);
}

}  // namespace splat
