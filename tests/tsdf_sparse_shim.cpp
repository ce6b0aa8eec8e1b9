// Host build of the sparse-volume part of splatam_amd/csrc/tsdf_math.h for tests/test_tsdf_sparse_cpu.py: plain-loop models of the
// kernels of csrc/tsdf_sparse.hip (S1 mark, S2 integrate, S3 triangles, S4 vertices) that call nothing but the header's functions, and
// the dense model's f < 0 set to hold the mark against.  Built with -ffp-contract=off, like tests/tsdf_math_shim.cpp, whose dense
// models (tm_integrate, tm_triangles, tm_vertices) are the other side of every comparison.
#include "../splatam_amd/csrc/tsdf_math.h"

using namespace splat;

namespace {
TsdfGrid grid(const int *dims, const float *origin, float voxel) {
    TsdfGrid g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2]; g.voxel = voxel;
    return g;
}
// cam: W, H, fx, fy, cx, cy, trunc, sil_thres, depth_max, weight_max (floats), then w2c
TsdfCamera camera(const float *cam, const float *w2c) {
    TsdfCamera c;
    c.W = (int)cam[0]; c.H = (int)cam[1];
    c.fx = cam[2]; c.fy = cam[3]; c.cx = cam[4]; c.cy = cam[5];
    c.trunc = cam[6]; c.sil_thres = cam[7]; c.depth_max = cam[8]; c.weight_max = cam[9];
    for (int q = 0; q < 12; ++q) c.m[q] = w2c[q];
    return c;
}
// the pool offset of grid point (i, j, k), -1 where its brick has no slot
long long offset_of(const TsdfBricks &b, const int32_t *directory, int i, int j, int k) {
    const int32_t s = directory[tsdf_brick_of(b, i, j, k)];
    return s < 0 ? -1 : (long long)s * kTsdfBrickPoints + tsdf_brick_local(b, i, j, k);
}
}  // namespace

extern "C" {

// brick geometry of one grid point: out = brick, local, and the point recovered from them (3); per = bricks per axis (3)
void ts_geometry(const int *dims, const int *lg, int i, int j, int k, long long *out, int *per) {
    const float origin[3] = {0.f, 0.f, 0.f};
    const TsdfBricks b = tsdf_bricks(grid(dims, origin, 1.f), lg[0], lg[1], lg[2]);
    per[0] = b.bx; per[1] = b.by; per[2] = b.bz;
    out[0] = tsdf_brick_of(b, i, j, k);
    out[1] = tsdf_brick_local(b, i, j, k);
    int i0, j0, k0, li, lj, lk;
    tsdf_brick_origin(b, out[0], i0, j0, k0);
    tsdf_brick_unlocal(b, (int)out[1], li, lj, lk);
    out[2] = i0 + li; out[3] = j0 + lj; out[4] = k0 + lk;
}

// S1: every pixel's tsdf_mark_box into flags [bricks]; returns the number of pixels that marked
long long ts_mark(const int *dims, const float *origin, float voxel, const int *lg, const float *cam, const float *w2c, const float *out6,
                  int32_t *flags) {
    const TsdfGrid g = grid(dims, origin, voxel);
    const TsdfBricks b = tsdf_bricks(g, lg[0], lg[1], lg[2]);
    const TsdfCamera c = camera(cam, w2c);
    const size_t plane = (size_t)c.W * c.H;
    long long marking = 0;
    for (int v = 0; v < c.H; ++v)
        for (int u = 0; u < c.W; ++u) {
            int lo[3], hi[3];
            const size_t px = (size_t)v * c.W + u;
            if (!tsdf_mark_box(g, c, u, v, out6[4 * plane + px], out6[3 * plane + px], lo, hi)) continue;
            ++marking;
            for (int bk = lo[2] >> b.lz; bk <= hi[2] >> b.lz; ++bk)
                for (int bj = lo[1] >> b.ly; bj <= hi[1] >> b.ly; ++bj)
                    for (int bi = lo[0] >> b.lx; bi <= hi[0] >> b.lx; ++bi) flags[((long long)bk * b.by + bj) * b.bx + bi] = 1;
        }
    return marking;
}

// the dense model's decisions: negative[o] = 1 where the view updates grid point o with f < 0
long long ts_negative(const int *dims, const float *origin, float voxel, const float *cam, const float *w2c, const float *out6, uint8_t *negative) {
    const TsdfGrid g = grid(dims, origin, voxel);
    const TsdfCamera c = camera(cam, w2c);
    long long n = 0;
    for (int k = 0; k < g.nz; ++k)
        for (int j = 0; j < g.ny; ++j)
            for (int i = 0; i < g.nx; ++i) {
                float p[3], f, rgb[3];
                tsdf_point(g, i, j, k, p);
                if (tsdf_observe(c, out6, p, f, rgb) && f < 0.f) {
                    negative[tsdf_linear(g, i, j, k)] = 1;
                    ++n;
                }
            }
    return n;
}

// S2: one view into every grid point of every slot's brick; pool: tsdf, weight, r, g, b, each [slots][2048]
long long ts_integrate(const int *dims, const float *origin, float voxel, const int *lg, const float *cam, const float *w2c, const float *out6,
                       int slots, const int32_t *brick_of_slot, float *tsdf, float *weight, float *r, float *gg, float *bb) {
    const TsdfGrid g = grid(dims, origin, voxel);
    const TsdfBricks b = tsdf_bricks(g, lg[0], lg[1], lg[2]);
    const TsdfCamera c = camera(cam, w2c);
    long long updated = 0;
    for (int s = 0; s < slots; ++s) {
        int i0, j0, k0;
        tsdf_brick_origin(b, brick_of_slot[s], i0, j0, k0);
        for (int local = 0; local < kTsdfBrickPoints; ++local) {
            int li, lj, lk;
            tsdf_brick_unlocal(b, local, li, lj, lk);
            const int i = i0 + li, j = j0 + lj, k = k0 + lk;
            if (i >= g.nx || j >= g.ny || k >= g.nz) continue;
            float p[3];
            tsdf_point(g, i, j, k, p);
            const size_t o = (size_t)s * kTsdfBrickPoints + local;
            updated += tsdf_update(c, out6, p, tsdf[o], weight[o], r[o], gg[o], bb[o]) ? 1 : 0;
        }
    }
    return updated;
}

// S3: the cells of every slot's brick, corners through the directory; keys [capacity][3]; returns the number of triangles wanted
long long ts_triangles(const int *dims, const float *origin, float voxel, const int *lg, int slots, const int32_t *brick_of_slot,
                       const int32_t *directory, const float *tsdf, const float *weight, float min_weight, int64_t *keys, long long capacity) {
    const TsdfGrid g = grid(dims, origin, voxel);
    const TsdfBricks b = tsdf_bricks(g, lg[0], lg[1], lg[2]);
    long long n = 0;
    for (int s = 0; s < slots; ++s) {
        int i0, j0, k0;
        tsdf_brick_origin(b, brick_of_slot[s], i0, j0, k0);
        for (int local = 0; local < kTsdfBrickPoints; ++local) {
            int li, lj, lk;
            tsdf_brick_unlocal(b, local, li, lj, lk);
            const int i = i0 + li, j = j0 + lj, k = k0 + lk;
            if (i >= g.nx - 1 || j >= g.ny - 1 || k >= g.nz - 1) continue;
            float f8[8];
            bool seen = true;
            for (int c = 0; c < 8 && seen; ++c) {
                const long long o = offset_of(b, directory, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1));
                seen = o >= 0 && weight[o] >= min_weight;
                if (seen) f8[c] = tsdf[o];
            }
            if (!seen) continue;
            int64_t tri[36];
            const int m = tsdf_cell_emit(g, i, j, k, tsdf_cell_mask(f8), tri);
            for (int t = 0; t < m; ++t, ++n)
                if (n < capacity)
                    for (int e = 0; e < 3; ++e) keys[3 * n + e] = tri[3 * t + e];
        }
    }
    return n;
}

// S4: vertices / colors [n][3] of n keys, the two grid points of each through the directory; returns the keys with a point that has no brick
long long ts_vertices(const int *dims, const float *origin, float voxel, const int *lg, const int32_t *directory, const float *tsdf,
                      const float *weight, const float *r, const float *gg, const float *bb, const int64_t *keys, long long n, float *vertices,
                      float *colors) {
    const TsdfGrid g = grid(dims, origin, voxel);
    const TsdfBricks b = tsdf_bricks(g, lg[0], lg[1], lg[2]);
    long long missing = 0;
    for (long long v = 0; v < n; ++v) {
        const int dir = (int)(keys[v] & 7);
        int i, j, k;
        tsdf_unlinear(g, keys[v] >> 3, i, j, k);
        const long long oa = offset_of(b, directory, i, j, k), ob = offset_of(b, directory, i + (dir & 1), j + ((dir >> 1) & 1), k + ((dir >> 2) & 1));
        if (oa < 0 || ob < 0) {
            ++missing;
            continue;
        }
        const float va[5] = {tsdf[oa], weight[oa], r[oa], gg[oa], bb[oa]}, vb[5] = {tsdf[ob], weight[ob], r[ob], gg[ob], bb[ob]};
        tsdf_vertex_values(g, keys[v], va, vb, vertices + 3 * v, colors + 3 * v);
    }
    return missing;
}

}
