// Host build of the marching-cubes part of splatam_amd/csrc/tsdf_math.h for tests/test_tsdf_cubes_cpu.py and
// tests/test_gpu_mesh_cubes.py: plain-loop models of the cubes pass of csrc/tsdf.hip that call nothing but the header's functions, so
// that the table and the pass are checked against the restatement of the rule (tests/tsdf_cubes_ref.py) without a GPU.
//
// With -DTSDF_CUBES_MAIN the file is a program of its own (built with -fsanitize=address,undefined by the test and run, never loaded
// into Python): all 256 masks, a volume with no surface, a 2 x 2 x 2 volume and a noise volume through the same functions, with the
// directed-edge balance of the noise mesh checked on the way.
#include "../splatam_amd/csrc/tsdf_math.h"

#include <map>
#include <utility>
#include <vector>

using namespace splat;

namespace {
TsdfGrid grid(int nx, int ny, int nz, const float *origin, float voxel) {
    TsdfGrid g;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2]; g.voxel = voxel;
    return g;
}
}  // namespace

extern "C" {

// the header's table, [256][16]
void tc_table(int8_t *out) {
    for (int m = 0; m < 256; ++m)
        for (int n = 0; n < 16; ++n) out[16 * m + n] = kTsdfCubesCases[m][n];
}

// corners (lower, upper) of edge e
void tc_edge(int e, int *corners) {
    corners[0] = tsdf_cubes_edge_corner(e);
    corners[1] = corners[0] | (1 << (e >> 2));
}

// the triangles of ONE cell (a 2 x 2 x 2 grid) with the given inside mask: keys [5][3]; returns their number, or -1 when the host
// model's emit, the count and the kernels' row path (tsdf_cubes_row / tsdf_cubes_store) do not say the same
int tc_cell_pattern(int mask, int64_t *keys) {
    const float origin[3] = {0.f, 0.f, 0.f};
    const TsdfGrid g = grid(2, 2, 2, origin, 1.f);
    const int n = tsdf_cubes_emit(g, 0, 0, 0, mask, keys);
    int64_t other[15];
    for (int q = 0; q < 15; ++q) other[q] = -1;
    if (n != tsdf_cubes_triangles(mask) || n != tsdf_cubes_store(g, 0, 0, 0, tsdf_cubes_row(mask), 0, 5, other)) return -1;
    for (int q = 0; q < 15; ++q)
        if (other[q] != (q < 3 * n ? keys[q] : -1)) return -1;
    return n;
}

// the cubes pass over every cell, in cell order, by the kernels' row path: keys [capacity][3]; returns the number of triangles wanted
long long tc_triangles(int nx, int ny, int nz, const float *origin, float voxel, const float *tsdf, const float *weight, float min_weight,
                       int64_t *keys, long long capacity) {
    const TsdfGrid g = grid(nx, ny, nz, origin, voxel);
    long long n = 0;
    for (int k = 0; k + 1 < nz; ++k)
        for (int j = 0; j + 1 < ny; ++j)
            for (int i = 0; i + 1 < nx; ++i) {
                float f8[8];
                bool seen = true;
                for (int c = 0; c < 8; ++c) {
                    const int64_t o = tsdf_linear(g, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1));
                    f8[c] = tsdf[o];
                    seen = seen && weight[o] >= min_weight;
                }
                if (!seen) continue;
                n += tsdf_cubes_store(g, i, j, k, tsdf_cubes_row(tsdf_cell_mask(f8)), (unsigned long long)n, (unsigned long long)capacity, keys);
            }
    return n;
}

// vertices / colors [n][3] of n keys (T3, unchanged)
void tc_vertices(int nx, int ny, int nz, const float *origin, float voxel, const float *tsdf, const float *r, const float *g, const float *b,
                 const int64_t *keys, long long n, float *vertices, float *colors) {
    const TsdfGrid gr = grid(nx, ny, nz, origin, voxel);
    for (long long v = 0; v < n; ++v) tsdf_vertex(gr, keys[v], tsdf, r, g, b, vertices + 3 * v, colors + 3 * v);
}

}

#ifdef TSDF_CUBES_MAIN
#include <stdio.h>

namespace {
// every directed edge as often as its reverse
bool balanced(const std::vector<int64_t> &keys) {
    std::map<std::pair<int64_t, int64_t>, int> d;
    for (size_t t = 0; t + 2 < keys.size(); t += 3)
        for (int e = 0; e < 3; ++e) ++d[{keys[t + e], keys[t + (e + 1) % 3]}];
    for (const auto &it : d) {
        const auto back = d.find({it.first.second, it.first.first});
        if (back == d.end() || back->second != it.second) return false;
    }
    return true;
}
long long run(int nx, int ny, int nz, const std::vector<float> &tsdf, std::vector<int64_t> &keys) {
    const float origin[3] = {-0.3f, 0.1f, 0.2f};
    const std::vector<float> weight(tsdf.size(), 1.f);
    const long long n = tc_triangles(nx, ny, nz, origin, 0.05f, tsdf.data(), weight.data(), 1.f, nullptr, 0);
    keys.assign(3 * n, -1);                                 // (exactly the need: one slot more would be out of bounds)
    if (tc_triangles(nx, ny, nz, origin, 0.05f, tsdf.data(), weight.data(), 1.f, keys.data(), n) != n) return -1;
    std::vector<float> pos(keys.size() * 3), col(keys.size() * 3);
    tc_vertices(nx, ny, nz, origin, 0.05f, tsdf.data(), tsdf.data(), tsdf.data(), tsdf.data(), keys.data(), (long long)keys.size(), pos.data(), col.data());
    return n;
}
}  // namespace

int main() {
    int64_t cell[15];
    int total = 0;
    for (int mask = 0; mask < 256; ++mask) {
        const int n = tc_cell_pattern(mask, cell);
        if (n < 0 || n > 5) return printf("mask %d: %d\n", mask, n), 1;
        total += n;
    }
    if (total != 820) return printf("%d triangles over the table\n", total), 1;
    std::vector<int64_t> keys;
    if (run(7, 6, 5, std::vector<float>(7 * 6 * 5, 1.f), keys) != 0) return printf("a volume without a surface emits\n"), 1;
    std::vector<float> one(8, 1.f);
    one[5] = -1.f;
    if (run(2, 2, 2, one, keys) != 1) return printf("2 x 2 x 2\n"), 1;
    const int nx = 14, ny = 13, nz = 12;                    // sign noise with an outside shell
    std::vector<float> noise(nx * ny * nz);
    uint32_t s = 12345u;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                s = s * 1664525u + 1013904223u;
                const bool shell = i == 0 || j == 0 || k == 0 || i == nx - 1 || j == ny - 1 || k == nz - 1;
                noise[(k * ny + j) * nx + i] = shell ? 1.f : ((float)(s >> 8) / 8388608.f - 1.f);
            }
    const long long n = run(nx, ny, nz, noise, keys);
    if (n <= 0 || !balanced(keys)) return printf("noise: %lld triangles, not balanced\n", n), 1;
    printf("ok: 820 table triangles, %lld noise triangles\n", n);
    return 0;
}
#endif
