// Host build of splatam_amd/csrc/tsdf_math.h for tests/test_tsdf_math_cpu.py and tests/test_mesh_cpu.py: plain-loop models of the
// kernels of csrc/tsdf.hip that call nothing but the header's per-point, per-cell and per-vertex functions, so that the mesh layer is
// checked against the float64 restatement (tests/tsdf_ref.py) without a GPU.  Built with -ffp-contract=off: every float32 step of the
// header is then one operation, as the device's round-to-nearest intrinsics make it there.
#include "../splatam_amd/csrc/tsdf_math.h"

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

// T1 over every grid point; vol: tsdf, weight, r, g, b, each [nz][ny][nx]; intr: fx, fy, cx, cy; w2c: 16 floats row-major.  Returns the
// number of points updated.
long long tm_integrate(int nx, int ny, int nz, const float *origin, float voxel, float trunc, float *tsdf, float *weight, float *r, float *g,
                       float *b, int W, int H, const float *out6, const float *intr, float sil_thres, float depth_max, float weight_max,
                       const float *w2c) {
    const TsdfGrid gr = grid(nx, ny, nz, origin, voxel);
    TsdfCamera c;
    c.W = W; c.H = H;
    c.fx = intr[0]; c.fy = intr[1]; c.cx = intr[2]; c.cy = intr[3];
    c.trunc = trunc; c.sil_thres = sil_thres; c.depth_max = depth_max; c.weight_max = weight_max;
    for (int q = 0; q < 12; ++q) c.m[q] = w2c[q];
    long long updated = 0;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                float p[3];
                tsdf_point(gr, i, j, k, p);
                const int64_t o = tsdf_linear(gr, i, j, k);
                updated += tsdf_update(c, out6, p, tsdf[o], weight[o], r[o], g[o], b[o]) ? 1 : 0;
            }
    return updated;
}

// the triangles of ONE cell (a 2 x 2 x 2 grid) with the given inside mask: keys [12][3]; returns their number
int tm_cell_pattern(int mask, int64_t *keys) {
    const float origin[3] = {0.f, 0.f, 0.f};
    const TsdfGrid g = grid(2, 2, 2, origin, 1.f);
    const int n = tsdf_cell_emit(g, 0, 0, 0, mask, keys);
    return n == tsdf_cell_triangles(mask) ? n : -1;
}

// T2 over every cell, in cell order: keys [capacity][3]; returns the number of triangles wanted
long long tm_triangles(int nx, int ny, int nz, const float *origin, float voxel, const float *tsdf, const float *weight, float min_weight,
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
                int64_t tri[36];
                const int m = tsdf_cell_emit(g, i, j, k, tsdf_cell_mask(f8), tri);
                for (int t = 0; t < m; ++t, ++n)
                    if (n < capacity)
                        for (int e = 0; e < 3; ++e) keys[3 * n + e] = tri[3 * t + e];
            }
    return n;
}

// T3: vertices / colors [n][3] of n keys
void tm_vertices(int nx, int ny, int nz, const float *origin, float voxel, const float *tsdf, const float *r, const float *g, const float *b,
                 const int64_t *keys, long long n, float *vertices, float *colors) {
    const TsdfGrid gr = grid(nx, ny, nz, origin, voxel);
    for (long long v = 0; v < n; ++v) tsdf_vertex(gr, keys[v], tsdf, r, g, b, vertices + 3 * v, colors + 3 * v);
}

// key of the edge from corner ca to corner cb of cell (i, j, k), and the grid point a linear index names
int64_t tm_edge_key(int nx, int ny, int nz, int i, int j, int k, int ca, int cb) {
    const float origin[3] = {0.f, 0.f, 0.f};
    return tsdf_edge_key(grid(nx, ny, nz, origin, 1.f), i, j, k, ca, cb);
}
void tm_unlinear(int nx, int ny, int nz, int64_t linear, int *ijk) {
    const float origin[3] = {0.f, 0.f, 0.f};
    tsdf_unlinear(grid(nx, ny, nz, origin, 1.f), linear, ijk[0], ijk[1], ijk[2]);
}
int64_t tm_max_points(void) { return kTsdfMaxPoints; }

}
