// tsdf_device.h -- what the dense volume's kernels (tsdf.hip) and the sparse volume's (tsdf_sparse.hip) share, one definition each, so
// that "the dense volume's mesh bit for bit" is held by the source and not by two copies kept in step: the view kernels' gate and
// camera, the frustum test of a brick, the lane body of integrate, the emission tail of the triangles pass, and the host side's grid
// and camera.  The arithmetic per grid point, cell and vertex is tsdf_math.h's.  What differs stays in its file: how a lane finds
// its grid points and where they lie in memory.
#pragma once

#include "splat_device.h"
#include "tsdf_math.h"

namespace splat {

constexpr long long kTsdfMaxGrid = 1ll << 30;
inline unsigned tsdf_grid_for(long long blocks) { return (unsigned)(blocks < 1 ? 1 : (blocks > kTsdfMaxGrid ? kTsdfMaxGrid : blocks)); }

struct TsdfArrays {
    float *tsdf, *weight, *r, *g, *b;
};

// SplatTsdfVolume and SplatTsdfSparse name these fields alike
template <typename Volume>
TsdfGrid tsdf_grid_of(const Volume &v) {
    TsdfGrid g;
    g.nx = v.nx; g.ny = v.ny; g.nz = v.nz;
    g.ox = v.origin[0]; g.oy = v.origin[1]; g.oz = v.origin[2]; g.voxel = v.voxel;
    return g;
}
template <typename Volume>
TsdfArrays tsdf_arrays_of(const Volume &v) { return TsdfArrays{v.tsdf, v.weight, v.r, v.g, v.b}; }
template <typename Volume>
TsdfCamera tsdf_camera_of(const Volume &v, const SplatTsdfView &w) {
    TsdfCamera c;
    c.W = w.width; c.H = w.height;
    c.fx = w.fx; c.fy = w.fy; c.cx = w.cx; c.cy = w.cy;
    c.trunc = v.trunc; c.sil_thres = w.sil_thres; c.depth_max = w.depth_max; c.weight_max = w.weight_max;
    for (int q = 0; q < 12; ++q) c.m[q] = 0.f;              // (filled in the kernel, from w2c)
    return c;
}

// ---------------------------------------------------------------------------------------------------------------- gate and camera
// A view kernel opens with these two.  `skip` (device, the view camera's truncation status) non-zero: the view's lists did not fit,
// its planes are incomplete; the launch returns before it reads them, and block 0 lane 0 has counted it in `skipped`.
__device__ __forceinline__ bool tsdf_view_skipped(const int32_t *skip, int32_t *skipped) {
    if (!(skip && *skip != 0)) return false;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(skipped, 1);
    return true;
}
__device__ __forceinline__ TsdfCamera tsdf_view_camera(const TsdfCamera &args, const float *w2c) {
    TsdfCamera cam = args;
#pragma unroll
    for (int q = 0; q < 12; ++q) cam.m[q] = w2c[q];
    return cam;
}

// ---------------------------------------------------------------------------------------------------------------- frustum test
// The brick's index box (i0..i1, j0..j1, k0..k1, clipped to the grid), pushed out by half a voxel, against the planes every updated
// point satisfies: z > 0; 0 <= u + 0.5 < W and 0 <= v + 0.5 < H, which for z > 0 are fx x + (cx + 0.5) z >= 0 and
// fx x + (cx + 0.5 - W) z < 0 (y likewise); z <= depth_max + trunc.  Each is linear in p, so a box whose eight corners all fail one of
// them holds no point that passes.  Plain float arithmetic: the half voxel of margin is orders of magnitude beyond its rounding.  Lane
// l of a wave projects corner l mod 8 and six ballots combine them (EVERY lane of the workgroup must be here: the callers' brick
// loops have uniform bounds), so the test costs a wave one corner, not eight.
__device__ __forceinline__ bool tsdf_brick_outside(const TsdfGrid &g, const TsdfCamera &cam, int i0, int i1, int j0, int j1, int k0, int k1) {
    const int c = threadIdx.x & 7;
    const float p[3] = {g.ox + g.voxel * ((c & 1) ? (float)i1 + 0.5f : (float)i0 - 0.5f),
                        g.oy + g.voxel * ((c & 2) ? (float)j1 + 0.5f : (float)j0 - 0.5f),
                        g.oz + g.voxel * ((c & 4) ? (float)k1 + 0.5f : (float)k0 - 0.5f)};
    const float *m = cam.m;
    const float ax = cam.cx + 0.5f, ay = cam.cy + 0.5f, far_z = cam.depth_max + cam.trunc;
    const float x = m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3];
    const float y = m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7];
    const float z = m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11];
    // a plane is failed by the brick when the ballot of its eight corners (lanes 0..7; the other lanes repeat them) is full
    bool outside = (__builtin_amdgcn_ballot_w64(!(z > 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fx * x + ax * z >= 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fx * x + (ax - (float)cam.W) * z < 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fy * y + ay * z >= 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(!(cam.fy * y + (ay - (float)cam.H) * z < 0.f)) & 0xffull) == 0xffull;
    outside |= (__builtin_amdgcn_ballot_w64(cam.depth_max > 0.f && z > far_z) & 0xffull) == 0xffull;
    return outside;
}

// ---------------------------------------------------------------------------------------------------------------- integrate, a lane
// One view into the V grid points (i .. i + V - 1, j, k) of a lane, which lie at offset o .. o + V - 1 of the five arrays ((i, j, k)
// inside the grid; V = 4: o a multiple of 4 and the arrays on 16 bytes, 16-byte accesses).  A point at or beyond nx is never hit:
// the sparse volume's last brick of a row needs that; the dense kernel takes V = 4 only where nx is a multiple of 4, where it is
// always inside, and carries the test all the same -- one body, and no way to call it that writes past a row.
// Three rounds of independent loads (a chain of dependent gathers per point is what the kernels would otherwise wait for): pixel
// offsets; silhouette and depth of all V; colours and the volume where a point is hit -- the volume is touched only then.
template <int V>
__device__ __forceinline__ void tsdf_integrate_lane(const TsdfGrid &g, const TsdfCamera &cam, const float *out6, const TsdfArrays &vol, int i, int j, int k,
                                                    size_t o) {
    const size_t plane = (size_t)cam.W * cam.H;
    struct Point {                  // (one struct per point, not one array per field: arrays of floats indexed in a loop are turned
        float z, s, dep, f, rgb[3]; //  into vectors before the loops are unrolled, and the kernels then carry the moves that keep them up)
        size_t px;
        bool hit;
    } pt[V];
    bool any = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float p[3];
        tsdf_point(g, i + v, j, k, p);
        pt[v].hit = i + v < g.nx && tsdf_project(cam, p, pt[v].z, pt[v].px);
        if (!pt[v].hit) pt[v].px = 0;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        pt[v].s = pt[v].hit ? out6[4 * plane + pt[v].px] : 0.f;
        pt[v].dep = pt[v].hit ? out6[3 * plane + pt[v].px] : 0.f;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        pt[v].hit = pt[v].hit && tsdf_measure(cam, pt[v].s, pt[v].dep, pt[v].z, pt[v].f);
        any |= pt[v].hit;
    }
    if (!any) return;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int c = 0; c < 3; ++c) pt[v].rgb[c] = pt[v].hit ? tsdf_colour(out6[c * plane + pt[v].px], pt[v].s) : 0.f;
    if constexpr (V == 4) {
        float4 q[5] = {*reinterpret_cast<const float4 *>(vol.tsdf + o), *reinterpret_cast<const float4 *>(vol.weight + o),
                       *reinterpret_cast<const float4 *>(vol.r + o), *reinterpret_cast<const float4 *>(vol.g + o),
                       *reinterpret_cast<const float4 *>(vol.b + o)};
        float *t = &q[0].x, *w = &q[1].x, *r = &q[2].x, *gg = &q[3].x, *b = &q[4].x;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (pt[v].hit) tsdf_blend(pt[v].f, pt[v].rgb, cam.weight_max, t[v], w[v], r[v], gg[v], b[v]);
        *reinterpret_cast<float4 *>(vol.tsdf + o) = q[0];
        *reinterpret_cast<float4 *>(vol.weight + o) = q[1];
        *reinterpret_cast<float4 *>(vol.r + o) = q[2];
        *reinterpret_cast<float4 *>(vol.g + o) = q[3];
        *reinterpret_cast<float4 *>(vol.b + o) = q[4];
    } else {
        float t = vol.tsdf[o], w = vol.weight[o], r = vol.r[o], gg = vol.g[o], b = vol.b[o];
        tsdf_blend(pt[0].f, pt[0].rgb, cam.weight_max, t, w, r, gg, b);
        vol.tsdf[o] = t; vol.weight[o] = w; vol.r[o] = r; vol.g[o] = gg; vol.b[o] = b;
    }
}

// ---------------------------------------------------------------------------------------------------------------- triangles, the tail
// From a lane's cell (i, j, k) and its sign pattern `mask` (0 for a lane without a cell, or an unseen one) to the stored keys: 0..12
// triangles by marching tetrahedra, or (kCubes) 0..5 from the lane's 16-byte row of the cubes table, held in four registers, the five
// slots unrolled and predicated on the count.  A wave reserves the slots of all its lanes with ONE returning atomic (prefix sum over
// the lanes' counts, the last lane adds the total, every lane reads the base): the group-binning reservation's idiom.  count[0] gets
// what is wanted; nothing is written at or beyond `capacity`.  EVERY lane of the wave must reach this call -- the scan and the
// readlanes are wave-wide -- so the loops it is called from have uniform bounds and idle lanes come with mask 0.
template <bool kCubes>
__device__ __forceinline__ void tsdf_emit_cell(const TsdfGrid &g, int i, int j, int k, int mask, int64_t *keys, unsigned long long capacity,
                                               unsigned long long *count) {
    TsdfCubesRow cubes;                                                     // (row 0 of the table is empty: an idle lane's)
    if constexpr (kCubes) cubes = tsdf_cubes_row(mask);
    const unsigned n = kCubes ? (unsigned)tsdf_cubes_row_entry(cubes, 0) : (unsigned)tsdf_cell_triangles(mask);
    if (__builtin_amdgcn_ballot_w64(n != 0) == 0ull) return;                // (wave-uniform)
    const unsigned incl = wave_scan_incl_u32(n);
    unsigned long long base = 0;
    if (lane_id() == kWave - 1) base = atomicAdd(count, (unsigned long long)incl);
    base = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(base >> 32), kWave - 1) << 32)
           | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)base, kWave - 1);
    if (n == 0) return;
    unsigned long long slot = base + (incl - n);
    if constexpr (kCubes) {
        tsdf_cubes_store(g, i, j, k, cubes, slot, capacity, keys);
        return;
    }
#pragma unroll 1
    for (int q = 0; q < 6; ++q) {
        const int8_t *row = kTsdfTetCases[tsdf_tet_mask(mask, q)];
        for (int t = 0; t < row[0]; ++t, ++slot) {
            if (slot >= capacity) continue;
            int64_t key[3];
            tsdf_tet_triangle(g, i, j, k, q, row, t, key);
            keys[3 * slot] = key[0];
            keys[3 * slot + 1] = key[1];
            keys[3 * slot + 2] = key[2];
        }
    }
}

}  // namespace splat
