// icp.hip -- the ICP layer: point-to-point registration of a source cloud onto the targets of a nearest-neighbour grid (meshscore.hip's
// splat_nn_query finds the correspondences).  The arithmetic is icp_math.h's; everything is double.
//
//   I1 icp_transform_kernel   one lane per source point: moved = float32(R p + t), T read from the state row ON THE DEVICE, so a block of
//                             iterations is enqueued without a host read in between.
//   I2 icp_accumulate_kernel  SPLAT_ICP_ROWS workgroups at most; lane l of workgroup b takes point b 256 + l, then strides by the whole
//                             launch: a fixed assignment.  Point i is a correspondence when 0 <= index[i] < num_targets and
//                             sqrt((double)dist2[i]) < threshold; its 17 terms (icp_add_terms) are added to the lane's running sums
//                             with p' = R p + t formed in double again.  Then each of the 17 sums goes down the wave (lane l += lane
//                             l + h, h = 32 .. 1, by __shfl_down: a fixed order), lane 0 of each of the four waves stores to LDS and
//                             lanes 0..16 add the four in wave order: one row of partials per workgroup.  No atomics.
//   I3 icp_solve_kernel       one workgroup.  status != 0: return (T is frozen).  Otherwise every lane fetches partials into LDS,
//                             lanes 0..16 add the rows in workgroup order, lane 0 runs icp_step: fitness, RMSE, the history row, the
//                             stop, and -- while running -- Horn's solve and T <- U T.
#include "splat_device.h"
#include "icp_math.h"

namespace splat {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct IcpOrigin {
    double c[3];
};

__global__ void __launch_bounds__(kBlock) icp_transform_kernel(const float *source, long long n, const double *state, float *moved) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = state[k];
    const float p[3] = {source[3 * i], source[3 * i + 1], source[3 * i + 2]};
    double out[3];
    icp_move(T, p, out);
    moved[3 * i] = (float)out[0];
    moved[3 * i + 1] = (float)out[1];
    moved[3 * i + 2] = (float)out[2];
}

__global__ void __launch_bounds__(kBlock) icp_accumulate_kernel(const float *source, const float *targets, long long num_targets,
                                                                const float *dist2, const int32_t *index, long long n, double threshold,
                                                                IcpOrigin origin, const double *state, double *partials) {
    __shared__ double s_wave[kWaves][kIcpSums];
    double T[12], acc[kIcpSums];
    for (int k = 0; k < 12; ++k) T[k] = state[k];
    for (int k = 0; k < kIcpSums; ++k) acc[k] = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const long long j = index[i];
        if (j < 0 || j >= num_targets) continue;
        const float d2 = dist2[i];
        if (!(ms_sqrtd((double)d2) < threshold)) continue;
        const float p[3] = {source[3 * i], source[3 * i + 1], source[3 * i + 2]};
        const float q[3] = {targets[3 * j], targets[3 * j + 1], targets[3 * j + 2]};
        double pm[3];
        icp_move(T, p, pm);
        icp_add_terms(acc, pm, q, d2, origin.c);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < kIcpSums; ++k) {
        double v = acc[k];
        for (int h = 32; h >= 1; h >>= 1) v = ms_addd(v, __shfl_down(v, h, 64));
        if (lane == 0) s_wave[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kIcpSums) {
        double v = s_wave[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) v = ms_addd(v, s_wave[w][threadIdx.x]);
        partials[(long long)blockIdx.x * kIcpSums + threadIdx.x] = v;
    }
}

__global__ void __launch_bounds__(kBlock) icp_solve_kernel(const double *partials, int rows, long long n, int32_t max_iterations,
                                                           double relative_fitness, double relative_rmse, IcpOrigin origin, double *state,
                                                           double *history) {
    __shared__ double s_part[SPLAT_ICP_ROWS * kIcpSums];
    __shared__ double s_sums[kIcpSums];
    if (state[kIcpStatus] != 0.0) return;                               // (the same answer for every lane: nothing below has run yet)
    for (int k = threadIdx.x; k < rows * kIcpSums; k += kBlock) s_part[k] = partials[k];
    __syncthreads();
    if (threadIdx.x < kIcpSums) {
        double v = 0.0;
        for (int b = 0; b < rows; ++b) v = ms_addd(v, s_part[b * kIcpSums + threadIdx.x]);
        s_sums[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double st[SPLAT_ICP_STATE], sums[kIcpSums];
    for (int k = 0; k < SPLAT_ICP_STATE; ++k) st[k] = state[k];
    for (int k = 0; k < kIcpSums; ++k) sums[k] = s_sums[k];
    icp_step(st, sums, n, max_iterations, relative_fitness, relative_rmse, origin.c, history);
    for (int k = 0; k < SPLAT_ICP_STATE; ++k) state[k] = st[k];
}

int rows_for(long long n) {
    const long long rows = (n + kBlock - 1) / kBlock;
    return (int)(rows < 1 ? 1 : (rows > SPLAT_ICP_ROWS ? SPLAT_ICP_ROWS : rows));
}

}  // namespace

hipError_t launch_icp_transform(const float *source, long long n, const double *state, float *moved, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(icp_transform_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, source, n, state, moved);
    return hipGetLastError();
}

hipError_t launch_icp_accumulate(const float *source, const float *targets, long long num_targets, const float *dist2, const int32_t *index,
                                 long long n, double threshold, const double *origin, const double *state, double *partials, hipStream_t s) {
    const IcpOrigin o = {{origin[0], origin[1], origin[2]}};
    hipLaunchKernelGGL(icp_accumulate_kernel, dim3((unsigned)rows_for(n)), dim3(kBlock), 0, s, source, targets, num_targets, dist2, index, n,
                       threshold, o, state, partials);
    return hipGetLastError();
}

hipError_t launch_icp_solve(const double *partials, long long n, int32_t max_iterations, double relative_fitness, double relative_rmse,
                            const double *origin, double *state, double *history, hipStream_t s) {
    const IcpOrigin o = {{origin[0], origin[1], origin[2]}};
    hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(kBlock), 0, s, partials, rows_for(n), n, max_iterations, relative_fitness, relative_rmse,
                       o, state, history);
    return hipGetLastError();
}

}  // namespace splat
