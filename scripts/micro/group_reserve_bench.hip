// Microbenchmark: the slot reservation of group binning alone (splat_device.h, file_group_records): W workgroups of 512 threads, each lane
// adds a non-zero count to the counter of group g = tid, tid + 512, ... of G = 836 groups with a RETURNING integer atomicAdd and uses the
// result.  Varies how far apart the counters lie (one per 128-byte line as the library had them, four or sixteen words apart, sixteen
// per upper half line as group_counter() places them, and relatives of that), the share of non-empty groups (61 % / 85 %: 512 / 1 024 random Gaussians per
// workgroup at workload B) and the number of workgroups.  Prints us per launch by HIP events (20 launches after 3 of warm-up, three
// repeats: lowest / median / highest) next to an empty launch of the same grid.
// Build: hipcc --offload-arch=gfx950 -O3 group_reserve_bench.hip -o group_reserve_bench ; run on the GPU box.  Developer tool.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#define CK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); exit(1); } } while (0)

constexpr int kBlock = 512, kGroups = 836, kLine = 32;

__device__ __forceinline__ unsigned hash(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

// PLACE 0: counter g at word g * stride; PLACE 1: `stride & 0xFF` (n = 16, 8, 4) consecutive groups in the upper 64 bytes of line
// (g / n) * (stride >> 8) -- every line exists while (kGroups / n) * (stride >> 8) < kGroups
template <int PLACE>
__device__ __forceinline__ size_t counter_word(int g, int stride) {
    const int n = stride & 0xFF, every = stride >> 8;
    return PLACE == 0 ? (size_t)g * stride : (size_t)(g / n) * every * kLine + 16 + (g % n);
}

template <int PLACE>
__global__ __launch_bounds__(kBlock) void reserve_kernel(unsigned *counters, unsigned *out, int stride, unsigned percent, int atomics) {
    unsigned acc = 0u;
    for (int g = (int)threadIdx.x; g < kGroups; g += kBlock) {
        const unsigned h = hash((unsigned)blockIdx.x * 9973u + (unsigned)g);
        if (h % 100u < percent && atomics) acc += atomicAdd(&counters[counter_word<PLACE>(g, stride)], 1u + (h >> 28));
    }
    out[blockIdx.x * kBlock + threadIdx.x] = acc;            // (the result is used: a returning atomic)
}

template <int PLACE>
static float timed(unsigned *counters, unsigned *out, int W, int stride, unsigned percent, int atomics) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) reserve_kernel<PLACE><<<W, kBlock>>>(counters, out, stride, percent, atomics);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(a));
    for (int i = 0; i < 20; ++i) reserve_kernel<PLACE><<<W, kBlock>>>(counters, out, stride, percent, atomics);
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, a, b));
    CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
    return ms * 1000.f / 20.f;
}

template <int PLACE>
static void row(unsigned *counters, unsigned *out, int W, int stride, unsigned percent, int atomics, const char *name) {
    float t[3];
    for (float &x : t) x = timed<PLACE>(counters, out, W, stride, percent, atomics);
    std::sort(t, t + 3);
    printf("%-28s W=%4d active=%2u%%  %7.2f %7.2f %7.2f us per launch (lowest, median, highest)\n", name, W, percent, t[0], t[1], t[2]);
}

int main() {
    unsigned *counters, *out;
    CK(hipMalloc(&counters, sizeof(unsigned) * kGroups * kLine));
    CK(hipMalloc(&out, sizeof(unsigned) * 586 * kBlock));
    CK(hipMemset(counters, 0, sizeof(unsigned) * kGroups * kLine));
    const int Ws[3] = {586, 293, 147};
    const unsigned percents[2] = {61u, 85u};
    for (int W : Ws) {
        row<0>(counters, out, W, 32, 61u, 0, "no atomics (launch floor)");
        for (unsigned p : percents) {
            row<0>(counters, out, W, 32, p, 1, "stride 32 (one per line)");
            row<0>(counters, out, W, 16, p, 1, "stride 16 (one per 64 B)");
            row<0>(counters, out, W, 4, p, 1, "stride 4");
            row<0>(counters, out, W, 1, p, 1, "stride 1");
            row<1>(counters, out, W, 16 | 1 << 8, p, 1, "16 per upper half line");
            row<1>(counters, out, W, 16 | 4 << 8, p, 1, "16 per half, every 4th line");
            row<1>(counters, out, W, 16 | 15 << 8, p, 1, "16 per half, every 15th line");
            row<1>(counters, out, W, 8 | 1 << 8, p, 1, "8 per upper half line");
            row<1>(counters, out, W, 4 | 1 << 8, p, 1, "4 per upper half line");
        }
    }
    CK(hipDeviceSynchronize());
    CK(hipFree(counters)); CK(hipFree(out));
    return 0;
}
