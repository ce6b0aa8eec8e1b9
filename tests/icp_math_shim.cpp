// Host build of splatam_amd/csrc/icp_math.h for tests/test_icp_cpu.py: plain-loop models of the kernels of csrc/icp.hip that call nothing
// but the header's functions.  Built with -ffp-contract=off: every double step of the header is then one operation, as on the device.
// With -DICP_SHIM_MAIN it is a stand-alone program for the sanitizers (main at the end).
#include <stdio.h>

#include "../splatam_amd/csrc/icp_math.h"

using namespace splat;

extern "C" {

// the proper rotation U [9] that maximises trace(U M), M [9] = sum (p - a)(q - b)^T
void im_horn(const double *M, double *U) { icp_horn(M, U); }

// I1
void im_transform(const double *T, const float *source, long long n, float *moved) {
    for (long long i = 0; i < n; ++i) {
        double out[3];
        icp_move(T, source + 3 * i, out);
        for (int k = 0; k < 3; ++k) moved[3 * i + k] = (float)out[k];
    }
}

// I2 in one row: the 17 sums over the correspondences, in the points' order
void im_accumulate(const double *T, const float *source, const float *targets, long long num_targets, const float *dist2, const int32_t *index,
                   long long n, double threshold, const double *origin, double *sums) {
    for (int k = 0; k < kIcpSums; ++k) sums[k] = 0.0;
    for (long long i = 0; i < n; ++i) {
        const long long j = index[i];
        if (j < 0 || j >= num_targets || !(ms_sqrtd((double)dist2[i]) < threshold)) continue;
        double pm[3];
        icp_move(T, source + 3 * i, pm);
        icp_add_terms(sums, pm, targets + 3 * j, dist2[i], origin);
    }
}

// the rigid motion of the 17 sums
void im_solve_sums(const double *sums, const double *origin, double *U, double *u) { icp_solve_sums(sums, origin, U, u); }

// I3's lane 0
void im_step(double *state, const double *sums, long long n, int32_t max_iterations, double relative_fitness, double relative_rmse,
             const double *origin, double *history) {
    icp_step(state, sums, n, max_iterations, relative_fitness, relative_rmse, origin, history);
}

int im_sums(void) { return kIcpSums; }
int im_state_slot(int which) {
    const int slots[] = {kIcpIteration, kIcpStatus, kIcpFitness, kIcpRmse, kIcpPrevFitness, kIcpPrevRmse, kIcpCount, kIcpPoints};
    return which >= 0 && which < 8 ? slots[which] : -1;
}

}

#ifdef ICP_SHIM_MAIN
// Edge inputs through every function; a sanitizer report or a wrong answer is a non-zero exit.
static int proper(const double *U) {
    const double det = U[0] * (U[4] * U[8] - U[5] * U[7]) - U[1] * (U[3] * U[8] - U[5] * U[6]) + U[2] * (U[3] * U[7] - U[4] * U[6]);
    return fabs(det - 1.0) <= 1e-12;
}

int main() {
    const double nan = NAN, inf = INFINITY;
    const double Ms[][9] = {{0, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 1, 0, 0, 0, -1}, {-1, 0, 0, 0, -1, 0, 0, 0, -1}, {1e300, 0, 0, 0, 1e300, 0, 0, 0, 1e300},
                            {1e-320, 0, 0, 0, 0, 0, 0, 0, 0}, {nan, 0, 0, 0, 1, 0, 0, 0, 1}, {inf, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 1, 0, -1, 0, 0, 0, 0, 1}};
    for (const auto &M : Ms) {
        double U[9];
        im_horn(M, U);
        if (!proper(U)) { printf("improper rotation\n"); return 1; }
    }
    // three points, indices in and out of range, a NaN and an infinite distance; then the loop to its limit and beyond
    const float source[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, targets[9] = {0.01f, 0, 0, 1.01f, 0, 0, 0.01f, 1, 0};
    const float dist2[4] = {1e-4f, 1e-4f, NAN, INFINITY};
    const int32_t index[4] = {0, 1, 2, 7};
    const double origin[3] = {0.3, 0.3, 0.0};
    double state[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, history[3 * 4] = {0}, sums[kIcpSums];
    for (int k = 0; k < 6; ++k) {
        float moved[12];
        im_transform(state, source, 4, moved);
        im_accumulate(state, source, targets, 3, dist2, index, 4, 0.1, origin, sums);
        if (sums[0] != 2.0) { printf("count %g\n", sums[0]); return 1; }
        im_step(state, sums, 4, 2, 0.0, 0.0, origin, history);
    }
    if (state[kIcpStatus] != 3.0 || state[kIcpIteration] != 0.0) { printf("status %g at %g\n", state[kIcpStatus], state[kIcpIteration]); return 1; }
    double full[kIcpSums] = {3, 3e-4, 1, 1, 0, 1.03, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0};
    double run[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int k = 0; k < 6; ++k) {
        full[1] *= 0.5;                                                  // (the RMSE keeps changing: only the limit can stop it)
        im_step(run, full, 3, 2, 0.0, 0.0, origin, history);
    }
    if (run[kIcpStatus] != 2.0 || run[kIcpIteration] != 2.0 || history[11] != 2.0) { printf("limit: status %g\n", run[kIcpStatus]); return 1; }
    im_accumulate(state, nullptr, nullptr, 0, nullptr, nullptr, 0, 0.1, origin, sums);
    if (sums[0] != 0.0) return 1;
    printf("icp_math: ok\n");
    return 0;
}
#endif
