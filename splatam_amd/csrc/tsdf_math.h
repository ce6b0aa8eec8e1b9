// tsdf_math.h -- arithmetic of the mesh layer (tsdf.hip), written once as host/device inline functions: the kernels call them per lane,
// tests/test_tsdf_math_cpu.py compiles the very same header with g++ (tests/tsdf_math_shim.cpp, -ffp-contract=off) and checks it
// against the float64 numpy form of the same definitions (tests/tsdf_ref.py).  The sparse volume's part (bricks, the mark; at the end)
// is held to the dense part of this same header by tests/test_tsdf_sparse_cpu.py through tests/tsdf_sparse_shim.cpp.
//
//   VOLUME   grid points p(i, j, k) = origin + voxel (i, j, k), nx ny nz of them, x fastest; five float32 arrays of that many:
//            tsdf (reset 1), weight (reset 0), r, g, b (reset 0).
//   UPDATE   of one grid point by one view (the six planes of a composite, its w2c, its pinhole):  pc = w2c p, skip unless pc.z > 0;
//            u = fx pc.x / pc.z + cx, v likewise; the pixel is (floor(u + 0.5), floor(v + 0.5)), skip outside the image;
//            s = silhouette there, skip unless s > sil_thres; d = depth / s (the depth plane is sum w_i z_i: without the division a
//            pixel at s = 0.99 sits 1 % short), skip unless d > 0 (NaN fails) and, with depth_max > 0, d <= depth_max;
//            sdf = d - pc.z, skip when sdf < -trunc; f = min(1, sdf / trunc); W' = W + 1; tsdf = (tsdf W + f) / W'; colour the same
//            running mean of clamp(rgb / s, 0, 1); then W = min(W', weight_max) when weight_max > 0.
//   SURFACE  marching tetrahedra on Kuhn's split of a cell: the six tetrahedra are the paths c -> c + e_a -> c + e_a + e_b ->
//            c + (1, 1, 1) over the permutations (a, b, c) of the axes.  The split is translation invariant, so neighbouring cells
//            agree on their shared faces and the surface is closed.  A corner is inside when tsdf < 0 (zero is outside).  A vertex
//            lies on a grid edge from corner a to a + dir, dir in {0, 1}^3 \ 0, and is NAMED by key = linear(a) 8 + (dx + 2 dy + 4 dz);
//            its position is p(a) + t (p(b) - p(a)), t = f_a / (f_a - f_b) (opposite signs: no cancellation), colour likewise.
//            The orientation of a triangle comes from the sign pattern alone (kTsdfTetCases, mirrored for the three tetrahedra of
//            odd permutations), with the normal towards positive tsdf -- never from computed positions, which lose their meaning
//            at corners that are exactly zero; the zero-area triangles such corners give are kept (dropping them opens the mesh).
//            Two corners inside, two outside: the quadrilateral (ac, ad, bd, bc) of inside a < b and outside c < d (positions along
//            the path) is split along ac - bd.
//   SURFACE, cubes   the second extractor: marching cubes, vertices on the twelve AXIS edges of a cell only (keys with dir in {1, 2, 4},
//            the same keys, positions and colours the tetrahedra give there), at most 5 triangles per cell.  The case table
//            (tsdf_cubes_table.h) follows from a rule that reads sign patterns alone.  Edge e = 0..11 is (c, c | 1 << a), axis-major
//            (a = 0, 1, 2), c ascending within an axis.  Take each face of the cell with its four corners counter-clockwise seen from
//            OUTSIDE the cell and walk that cycle: every maximal run of inside corners gives one directed SEGMENT, from the crossing
//            where the walk enters the run to the crossing where it leaves.  A face with two crossings has one segment; a face whose
//            inside corners are diagonal has two -- each inside corner is cut off on its own and the outside connects through the
//            face: the one disambiguation, used everywhere.  Every crossed edge then has one outgoing and one incoming segment, so
//            the segments chain into closed loops; a loop starts at its lowest edge, loops go by ascending start, and each is
//            fan-triangulated from its start: (l0, li, li+1).  One corner inside: the loop x -> y -> z edge of that corner, normal
//            away from it -- towards positive tsdf, like the tetrahedra.
//            CLOSED: the segments on a face depend on that face's four signs only.  The neighbouring cell sees the same four signs on
//            the same four grid points, walks them the other way round (its outside is this cell's inside of the face) and so puts
//            the same segments there, reversed; inside a cell a fan's diagonals occur once in each direction.  Every directed edge
//            of the mesh is therefore matched by its reverse wherever both cells are seen.
//            NOT here: the asymptotic decider and interior ambiguity tests (MC33), parity with any library's table, dual contouring.
//            KNOWN: a fan diagonal can join two crossings that lie on one ambiguous face, and the neighbour's fan can join the same
//            two; on adversarial sign noise a few edges are then shared by four triangles (still a closed oriented cycle: each
//            direction as often as its reverse).  Smooth surfaces do not do this.
//
// Every float32 step is an operation of its own (tsdf_add / _sub / _mul / _div: operators the device compiler may not contract, plain
// operators under -ffp-contract=off on the host), so a decision does not depend on what a compiler contracts.
#pragma once

#include <math.h>
#include <stdint.h>

#include "splat_math.h"

namespace splat {

#if defined(__HIP_DEVICE_COMPILE__)
// (the pragma keeps the `contract` flag off the instruction itself, so that it stays one operation wherever it is inlined: the
//  runtime's __fmul_rn / __fadd_rn are plain operators the device compiler is free to fuse)
SPLAT_HD float tsdf_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
SPLAT_HD float tsdf_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
SPLAT_HD float tsdf_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
SPLAT_HD float tsdf_div(float a, float b) { return __fdiv_rn(a, b); }
#else
SPLAT_HD float tsdf_add(float a, float b) { return a + b; }
SPLAT_HD float tsdf_sub(float a, float b) { return a - b; }
SPLAT_HD float tsdf_mul(float a, float b) { return a * b; }
SPLAT_HD float tsdf_div(float a, float b) { return a / b; }
#endif

constexpr int64_t kTsdfMaxPoints = (int64_t)1 << 40;        // nx ny nz below this: a key (linear 8 + dir) stays far inside int64

struct TsdfGrid {
    int nx, ny, nz;
    float ox, oy, oz, voxel;
};

SPLAT_HD int64_t tsdf_linear(const TsdfGrid &g, int i, int j, int k) { return ((int64_t)k * g.ny + j) * g.nx + i; }
SPLAT_HD void tsdf_unlinear(const TsdfGrid &g, int64_t l, int &i, int &j, int &k) {
    i = (int)(l % g.nx);
    const int64_t r = l / g.nx;
    j = (int)(r % g.ny);
    k = (int)(r / g.ny);
}
// p(i, j, k): one multiplication and one addition per coordinate
SPLAT_HD void tsdf_point(const TsdfGrid &g, int i, int j, int k, float *p) {
    p[0] = tsdf_add(g.ox, tsdf_mul(g.voxel, (float)i));
    p[1] = tsdf_add(g.oy, tsdf_mul(g.voxel, (float)j));
    p[2] = tsdf_add(g.oz, tsdf_mul(g.voxel, (float)k));
}

// ---------------------------------------------------------------------------------------------------------------- update
struct TsdfCamera {
    int W, H;
    float fx, fy, cx, cy;
    float trunc, sil_thres, depth_max, weight_max;
    float m[12];                    // rows 0..2 of the view's w2c (row-major)
};

// row r of w2c applied to p: ((m0 x + m1 y) + m2 z) + m3
SPLAT_HD float tsdf_cam_coord(const float *row, const float *p) {
    return tsdf_add(tsdf_add(tsdf_add(tsdf_mul(row[0], p[0]), tsdf_mul(row[1], p[1])), tsdf_mul(row[2], p[2])), row[3]);
}
SPLAT_HD float tsdf_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// The update in three steps, so that a kernel can have the loads of several grid points in flight at once:
// 1. where the view sees grid point p: false = behind the camera or outside the image; else z = pc.z and o, the pixel's offset in a plane
SPLAT_HD bool tsdf_project(const TsdfCamera &c, const float *p, float &z, size_t &o) {
    z = tsdf_cam_coord(c.m + 8, p);
    if (!(z > 0.f)) return false;
    const float x = tsdf_cam_coord(c.m, p), y = tsdf_cam_coord(c.m + 4, p);
    const float u = tsdf_add(tsdf_div(tsdf_mul(c.fx, x), z), c.cx), v = tsdf_add(tsdf_div(tsdf_mul(c.fy, y), z), c.cy);
    const float uf = floorf(tsdf_add(u, 0.5f)), vf = floorf(tsdf_add(v, 0.5f));
    if (!(uf >= 0.f && uf < (float)c.W && vf >= 0.f && vf < (float)c.H)) return false;       // (NaN and +-inf fail here, before the cast)
    o = (size_t)(int)vf * c.W + (int)uf;
    return true;
}
// 2. what the pixel's silhouette s and depth-plane value say about a point at depth z: false = no update; else f, the truncated
//    distance over trunc, at most 1
SPLAT_HD bool tsdf_measure(const TsdfCamera &c, float s, float depth, float z, float &f) {
    if (!(s > c.sil_thres)) return false;
    const float d = tsdf_div(depth, s);
    if (!(d > 0.f)) return false;
    if (c.depth_max > 0.f && !(d <= c.depth_max)) return false;
    const float sdf = tsdf_sub(d, z);
    if (sdf < -c.trunc) return false;
    f = fminf(1.f, tsdf_div(sdf, c.trunc));
    return true;
}
// 3. the pixel's colour channel: the composite's sum over the silhouette, clamped
SPLAT_HD float tsdf_colour(float v, float s) { return tsdf_clamp01(tsdf_div(v, s)); }

// ... and in one piece: out6 is [>= 5][H][W] (r, g, b, depth, silhouette)
SPLAT_HD bool tsdf_observe(const TsdfCamera &c, const float *out6, const float *p, float &f, float *rgb) {
    float z;
    size_t o;
    if (!tsdf_project(c, p, z, o)) return false;
    const size_t plane = (size_t)c.W * c.H;
    const float s = out6[4 * plane + o];
    if (!tsdf_measure(c, s, out6[3 * plane + o], z, f)) return false;
    for (int k = 0; k < 3; ++k) rgb[k] = tsdf_colour(out6[k * plane + o], s);
    return true;
}

// the running means; vals: tsdf, r, g, b of the grid point
SPLAT_HD void tsdf_blend(float f, const float *rgb, float weight_max, float &tsdf, float &w, float &r, float &g, float &b) {
    const float w1 = tsdf_add(w, 1.f);
    tsdf = tsdf_div(tsdf_add(tsdf_mul(tsdf, w), f), w1);
    r = tsdf_div(tsdf_add(tsdf_mul(r, w), rgb[0]), w1);
    g = tsdf_div(tsdf_add(tsdf_mul(g, w), rgb[1]), w1);
    b = tsdf_div(tsdf_add(tsdf_mul(b, w), rgb[2]), w1);
    w = weight_max > 0.f ? fminf(w1, weight_max) : w1;
}

// one grid point by one view, for the host model (the kernel loads the volume only where tsdf_observe says yes)
SPLAT_HD bool tsdf_update(const TsdfCamera &c, const float *out6, const float *p, float &tsdf, float &w, float &r, float &g, float &b) {
    float f, rgb[3];
    if (!tsdf_observe(c, out6, p, f, rgb)) return false;
    tsdf_blend(f, rgb, c.weight_max, tsdf, w, r, g, b);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- surface
// A cell's corners are numbered dx + 2 dy + 4 dz.  Tetrahedron q = 0..5 of Kuhn's split walks the axes in the order kTsdfPerm[q]; its
// vertices 0..3 are the cell's corners 0, 1 << a, (1 << a) | (1 << b), 7.  Even permutations give positively oriented tetrahedra
// (det [v1 - v0, v2 - v0, v3 - v0] = det [e_a, e_b, e_c] > 0), odd ones their mirror images.
constexpr int8_t kTsdfPerm[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};     // three even, three odd
SPLAT_HD int tsdf_tet_corner(int q, int v) {
    const int a = 1 << kTsdfPerm[q][0], b = 1 << kTsdfPerm[q][1];
    return v == 0 ? 0 : (v == 1 ? a : (v == 2 ? (a | b) : 7));
}
SPLAT_HD bool tsdf_tet_odd(int q) { return q >= 3; }

// the six edges of a tetrahedron, (lower vertex, upper vertex) along the path
constexpr int8_t kTsdfTetEdges[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// case table of a POSITIVELY oriented tetrahedron: row = inside mask (bit v: vertex v has tsdf < 0), entry 0 the number of triangles, then
// three edges per triangle, wound so that the normal points towards positive tsdf.  One vertex inside (mask 1): the triangle on edges
// 01, 02, 03 has n . (v1 - v0) = t2 t3 det > 0, away from the inside vertex; every other row follows by relabelling, and a mask's
// complement is the same surface with the winding reversed.
constexpr int8_t kTsdfTetCases[16][7] = {
    {0, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 2, 0, 0, 0}, {1, 0, 4, 3, 0, 0, 0}, {2, 1, 2, 4, 1, 4, 3},
    {1, 1, 3, 5, 0, 0, 0}, {2, 0, 5, 2, 0, 3, 5}, {2, 0, 4, 5, 0, 5, 1}, {1, 2, 4, 5, 0, 0, 0},
    {1, 2, 5, 4, 0, 0, 0}, {2, 0, 1, 5, 0, 5, 4}, {2, 0, 5, 3, 0, 2, 5}, {1, 1, 5, 3, 0, 0, 0},
    {2, 1, 3, 4, 1, 4, 2}, {1, 0, 3, 4, 0, 0, 0}, {1, 0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}};

// inside mask of a cell from its eight corner values (corner order dx + 2 dy + 4 dz)
SPLAT_HD int tsdf_cell_mask(const float *f8) {
    int m = 0;
    for (int c = 0; c < 8; ++c) m |= (f8[c] < 0.f ? 1 : 0) << c;
    return m;
}
SPLAT_HD int tsdf_tet_mask(int cell_mask, int q) {
    int m = 0;
    for (int v = 0; v < 4; ++v) m |= ((cell_mask >> tsdf_tet_corner(q, v)) & 1) << v;
    return m;
}
// triangles a cell's sign pattern asks for (0..12)
SPLAT_HD int tsdf_cell_triangles(int cell_mask) {
    if (cell_mask == 0 || cell_mask == 255) return 0;
    int n = 0;
    for (int q = 0; q < 6; ++q) n += kTsdfTetCases[tsdf_tet_mask(cell_mask, q)][0];
    return n;
}
// key of the vertex on the cell's edge between corners ca and cb (ca a subset of cb's bits); cell = (i, j, k) of corner 0
SPLAT_HD int64_t tsdf_edge_key(const TsdfGrid &g, int i, int j, int k, int ca, int cb) {
    return tsdf_linear(g, i + (ca & 1), j + ((ca >> 1) & 1), k + ((ca >> 2) & 1)) * 8 + (cb & ~ca);
}
// triangle t of tetrahedron q of cell (i, j, k) under the table's row `row` (of the tetrahedron's mask): its three keys, wound
SPLAT_HD void tsdf_tet_triangle(const TsdfGrid &g, int i, int j, int k, int q, const int8_t *row, int t, int64_t *key) {
    int64_t e3[3];
    for (int e = 0; e < 3; ++e) {
        const int8_t *ed = kTsdfTetEdges[row[1 + 3 * t + e]];
        e3[e] = tsdf_edge_key(g, i, j, k, tsdf_tet_corner(q, ed[0]), tsdf_tet_corner(q, ed[1]));
    }
    const bool odd = tsdf_tet_odd(q);
    key[0] = e3[0];
    key[1] = odd ? e3[2] : e3[1];
    key[2] = odd ? e3[1] : e3[2];
}
// the triangles of cell (i, j, k) with sign pattern cell_mask, three keys each, to out[3 n]; returns n (the host model's loop; the
// kernel walks the same two loops and stores each triangle where its slot is)
SPLAT_HD int tsdf_cell_emit(const TsdfGrid &g, int i, int j, int k, int cell_mask, int64_t *out) {
    int n = 0;
    if (cell_mask == 0 || cell_mask == 255) return 0;
    for (int q = 0; q < 6; ++q) {
        const int8_t *row = kTsdfTetCases[tsdf_tet_mask(cell_mask, q)];
        for (int t = 0; t < row[0]; ++t, ++n) tsdf_tet_triangle(g, i, j, k, q, row, t, out + 3 * n);
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------- surface, cubes
#include "tsdf_cubes_table.h"

// triangles a cell's sign pattern asks for (0..5)
SPLAT_HD int tsdf_cubes_triangles(int cell_mask) { return kTsdfCubesCases[cell_mask][0]; }
// lower corner of edge e = 4 a + n: n with a zero bit inserted at position a (the upper corner is that | 1 << a)
SPLAT_HD int tsdf_cubes_edge_corner(int e) {
    const int a = e >> 2, n = e & 3, low = (1 << a) - 1;
    return (n & low) | ((n & ~low) << 1);
}
// key of the vertex on edge e of cell (i, j, k): an ordinary edge key with dir = 1 << axis
SPLAT_HD int64_t tsdf_cubes_edge_key(const TsdfGrid &g, int i, int j, int k, int e) {
    const int c = tsdf_cubes_edge_corner(e);
    return tsdf_edge_key(g, i, j, k, c, c | (1 << (e >> 2)));
}
// triangle t of cell (i, j, k) under the table's row `row` (of the cell's mask): its three keys, wound
SPLAT_HD void tsdf_cubes_triangle(const TsdfGrid &g, int i, int j, int k, const int8_t *row, int t, int64_t *key) {
    for (int e = 0; e < 3; ++e) key[e] = tsdf_cubes_edge_key(g, i, j, k, row[1 + 3 * t + e]);
}
// the triangles of cell (i, j, k) with sign pattern cell_mask, three keys each, to out[3 n]; returns n (the host model's loop)
SPLAT_HD int tsdf_cubes_emit(const TsdfGrid &g, int i, int j, int k, int cell_mask, int64_t *out) {
    const int8_t *row = kTsdfCubesCases[cell_mask];
    for (int t = 0; t < row[0]; ++t) tsdf_cubes_triangle(g, i, j, k, row, t, out + 3 * t);
    return row[0];
}

// A row as the kernels hold it: four registers, fetched with one 16-byte load (each lane its own row: the table is 4 KiB and stays in
// the vector cache), entries picked out by shifts at compile-time positions -- the triangle loop is unrolled over the row's five slots
// and predicated on the count, so no lane indexes memory by a value it computed and the wave does not loop to its longest row.
struct TsdfCubesRow {
    uint32_t w[4];
};
SPLAT_HD TsdfCubesRow tsdf_cubes_row(int cell_mask) {
    TsdfCubesRow r;
    __builtin_memcpy(r.w, kTsdfCubesCases[cell_mask], 16);
    return r;
}
SPLAT_HD int tsdf_cubes_row_entry(const TsdfCubesRow &r, int n) { return (int)((r.w[n >> 2] >> (8 * (n & 3))) & 0xffu); }
// the row's triangles into keys[3 slot ...], those at or beyond `capacity` left out; returns their number
SPLAT_HD int tsdf_cubes_store(const TsdfGrid &g, int i, int j, int k, const TsdfCubesRow &r, unsigned long long slot, unsigned long long capacity,
                              int64_t *keys) {
    const int n = tsdf_cubes_row_entry(r, 0);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 5; ++t) {
        if (t >= n || slot + t >= capacity) continue;
        for (int e = 0; e < 3; ++e) keys[3 * (slot + t) + e] = tsdf_cubes_edge_key(g, i, j, k, tsdf_cubes_row_entry(r, 1 + 3 * t + e));
    }
    return n;
}

// position and colour of the vertex a key names, from the values of its edge's two grid points: va, vb = tsdf, weight, r, g, b (the
// volume's array order; the weight is not used) at corner a and at corner a + dir
SPLAT_HD void tsdf_vertex_values(const TsdfGrid &g, int64_t key, const float *va, const float *vb, float *pos, float *col) {
    const int dir = (int)(key & 7);
    int i, j, k;
    tsdf_unlinear(g, key >> 3, i, j, k);
    const float fa = va[0], fb = vb[0];
    const float t = tsdf_div(fa, tsdf_sub(fa, fb));
    float pa[3], pb[3];
    tsdf_point(g, i, j, k, pa);
    tsdf_point(g, i + (dir & 1), j + ((dir >> 1) & 1), k + ((dir >> 2) & 1), pb);
    for (int c = 0; c < 3; ++c) pos[c] = tsdf_add(pa[c], tsdf_mul(t, tsdf_sub(pb[c], pa[c])));
    for (int c = 0; c < 3; ++c) col[c] = tsdf_add(va[2 + c], tsdf_mul(t, tsdf_sub(vb[2 + c], va[2 + c])));
}

// ... and with the two grid points read from the volume's five arrays
SPLAT_HD void tsdf_vertex(const TsdfGrid &g, int64_t key, const float *tsdf, const float *r, const float *gr, const float *b, float *pos,
                          float *col) {
    const int64_t la = key >> 3;
    const int dir = (int)(key & 7);
    int i, j, k;
    tsdf_unlinear(g, la, i, j, k);
    const int64_t lb = tsdf_linear(g, i + (dir & 1), j + ((dir >> 1) & 1), k + ((dir >> 2) & 1));
    const float va[5] = {tsdf[la], 0.f, r[la], gr[la], b[la]}, vb[5] = {tsdf[lb], 0.f, r[lb], gr[lb], b[lb]};
    tsdf_vertex_values(g, key, va, vb, pos, col);
}

// ---------------------------------------------------------------------------------------------------------------- sparse volume
// A SPARSE volume (tsdf_sparse.hip) keeps the same virtual grid and stores only BRICKS of it: boxes of 2^lx x 2^ly x 2^lz = 2048 grid
// points, x fastest inside the brick, each 8 KiB contiguous per array in a pool; a directory over all bricks of the grid (x fastest)
// holds a brick's slot in the pool or -1.  Which bricks: a grid point's tsdf is a running convex mean, from 1, of the f it received,
// so tsdf < 0 needs one update with f < 0 -- the point lay in the band d < z <= d + trunc behind the surface of some view --, and a
// cell emits triangles only with a negative corner and all eight seen: every emitting cell lies in the 3 x 3 x 3 index neighbourhood
// of a grid point some view updated with f < 0.  tsdf_mark_box is a conservative index box around the grid points ONE PIXEL of one
// view can update so, neighbourhood included; the bricks meeting the boxes of every pixel of every view are allocated, and when each
// of them then receives every update of every view, every corner of every emitting cell holds the dense volume's bits.
constexpr int kTsdfBrickPoints = 2048, kTsdfBrickLog2 = 11;

struct TsdfBricks {
    int lx, ly, lz;                 // log2 of the brick's points per axis; lx + ly + lz = 11, lx >= 2 (a row is a multiple of 4 points)
    int bx, by, bz;                 // bricks per axis: the grid's points, rounded up
};
SPLAT_HD TsdfBricks tsdf_bricks(const TsdfGrid &g, int lx, int ly, int lz) {
    TsdfBricks b;
    b.lx = lx; b.ly = ly; b.lz = lz;
    b.bx = (g.nx + (1 << lx) - 1) >> lx; b.by = (g.ny + (1 << ly) - 1) >> ly; b.bz = (g.nz + (1 << lz) - 1) >> lz;
    return b;
}
SPLAT_HD int64_t tsdf_brick_count(const TsdfBricks &b) { return (int64_t)b.bx * b.by * b.bz; }
// the brick of grid point (i, j, k), and the point's offset inside it
SPLAT_HD int64_t tsdf_brick_of(const TsdfBricks &b, int i, int j, int k) { return ((int64_t)(k >> b.lz) * b.by + (j >> b.ly)) * b.bx + (i >> b.lx); }
SPLAT_HD int tsdf_brick_local(const TsdfBricks &b, int i, int j, int k) {
    return ((((k & ((1 << b.lz) - 1)) << b.ly) | (j & ((1 << b.ly) - 1))) << b.lx) | (i & ((1 << b.lx) - 1));
}
// ... and back: the first grid point of a brick, and the grid point at a local offset from it
SPLAT_HD void tsdf_brick_origin(const TsdfBricks &b, int64_t brick, int &i0, int &j0, int &k0) {
    i0 = (int)(brick % b.bx) << b.lx;
    const int64_t r = brick / b.bx;
    j0 = (int)(r % b.by) << b.ly;
    k0 = (int)(r / b.by) << b.lz;
}
SPLAT_HD void tsdf_brick_unlocal(const TsdfBricks &b, int local, int &li, int &lj, int &lk) {
    li = local & ((1 << b.lx) - 1);
    lj = (local >> b.lx) & ((1 << b.ly) - 1);
    lk = local >> (b.lx + b.ly);
}

// lower / upper clipped index of a box coordinate; written so that a NaN (a depth beyond float range) gives the whole axis
SPLAT_HD int tsdf_index_lo(float a, int n) { return !(a > 0.f) ? 0 : (a < (float)n ? (int)a : n); }
SPLAT_HD int tsdf_index_hi(float a, int n) { return !(a < (float)(n - 1)) ? n - 1 : (a >= 0.f ? (int)a : -1); }

// The index box [lo, hi] (inclusive, clipped to the grid; empty when lo > hi on an axis) of pixel (u, v) of a view whose silhouette
// and depth-plane value there are s and depth: false when the pixel can give no grid point an f < 0.  The gates are tsdf_measure's,
// the depth limit widened to depth_max + trunc.  A grid point the pixel updates with f < 0 projects into [u - 0.5, u + 0.5) x
// [v - 0.5, v + 0.5) at a depth in (d, d + trunc]: inside the frustum segment whose eight corners are the rays through
// (u +- 0.5, v +- 0.5) at depths d and d + trunc.  The corners go to world space by the rigid inverse of w2c (R^T (pc - t)); their
// axis-aligned box, widened by half a voxel against the rounding of all this (float32 at 100 m: 1e-5 m; a voxel is a millimetre at
// least) and by one index for the cell neighbourhood, is [ceil((lo - o) / voxel - 0.5) - 1, floor((hi - o) / voxel + 0.5) + 1].
SPLAT_HD bool tsdf_mark_box(const TsdfGrid &g, const TsdfCamera &c, int u, int v, float s, float depth, int *lo, int *hi) {
    if (!(s > c.sil_thres)) return false;
    const float d = tsdf_div(depth, s);
    if (!(d > 0.f) || !(d <= 3.0e38f)) return false;                 // (an infinite d gives sdf = inf and f = 1 wherever it is seen)
    if (c.depth_max > 0.f && !(d <= tsdf_add(c.depth_max, c.trunc))) return false;
    float wlo[3] = {INFINITY, INFINITY, INFINITY}, whi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool finite = true;
    for (int q = 0; q < 8; ++q) {
        const float z = (q & 4) ? tsdf_add(d, c.trunc) : d;
        const float uf = tsdf_add((float)u, (q & 1) ? 0.5f : -0.5f), vf = tsdf_add((float)v, (q & 2) ? 0.5f : -0.5f);
        // the camera-space corner less the translation
        const float pc[3] = {tsdf_sub(tsdf_mul(tsdf_div(tsdf_sub(uf, c.cx), c.fx), z), c.m[3]),
                             tsdf_sub(tsdf_mul(tsdf_div(tsdf_sub(vf, c.cy), c.fy), z), c.m[7]), tsdf_sub(z, c.m[11])};
        for (int a = 0; a < 3; ++a) {
            const float w = tsdf_add(tsdf_add(tsdf_mul(c.m[a], pc[0]), tsdf_mul(c.m[4 + a], pc[1])), tsdf_mul(c.m[8 + a], pc[2]));
            finite = finite && w >= -3.0e38f && w <= 3.0e38f;
            wlo[a] = fminf(wlo[a], w);
            whi[a] = fmaxf(whi[a], w);
        }
    }
    const float o[3] = {g.ox, g.oy, g.oz};
    const int n[3] = {g.nx, g.ny, g.nz};
    for (int a = 0; a < 3; ++a) {
        const float fl = finite ? tsdf_sub(ceilf(tsdf_sub(tsdf_div(tsdf_sub(wlo[a], o[a]), g.voxel), 0.5f)), 1.f) : NAN;
        const float fh = finite ? tsdf_add(floorf(tsdf_add(tsdf_div(tsdf_sub(whi[a], o[a]), g.voxel), 0.5f)), 1.f) : NAN;
        lo[a] = tsdf_index_lo(fl, n[a]);
        hi[a] = tsdf_index_hi(fh, n[a]);
    }
    return lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
}

}  // namespace splat
