// meshrender_math.h -- arithmetic of the mesh render layer (meshrender.hip), written once as host/device inline functions: the kernels
// call them per lane, tests/test_meshrender_cpu.py compiles the very same header with g++ (tests/meshrender_math_shim.cpp,
// -ffp-contract=off) and checks it against the float64 numpy restatement tests/meshrender_ref.py.
//
//   CAMERA     pc = w2c p per row as ((m0 x + m1 y) + m2 z) + m3 (w2c: 16 floats, row-major).  Pixel (i, j) looks along
//              d = ((i - cx) / fx, (j - cy) / fy, 1); a point lands on pixel (floor(fx x / z + cx + 0.5), floor(fy y / z + cy + 0.5)):
//              the convention of tsdf_math.h.
//   EDGE       of a triangle's camera-space vertices a, b (vertex indices ia, ib): the plane through the camera centre and both,
//              e = a x b, each component one product minus one product.  It is ALWAYS formed from the endpoint of lower index first
//              and negated when the triangle names them the other way round: the two triangles that share an edge then hold vectors
//              that are exact negatives (or exact copies) of each other, which `fma(x, y, -z w)` against its swapped form would not give.
//              E(d) = (dx e0 + dy e1) + e2.
//   COVERAGE   pixel (i, j) is covered by the triangle when E_ab, E_bc, E_ca are all >= 0 or all <= 0 (zero included, both faces count).
//              With the exact antisymmetry above, a ray through a shared edge is turned away by at most one of its two triangles on
//              account of that edge: a closed mesh has no pinholes along its edges.
//   HIT        z = (n . a) / (n . d), n = (b - a) x (c - a) in camera space, n . d = (dx n0 + dy n1) + n2.  The hit counts when
//              near <= z < +inf.  No near-plane clipping: a triangle behind the camera gives z < near, one that crosses z = 0 is
//              handled by the same three signs, one that contains the camera centre gives z = 0 or NaN.
//   BOX        of a triangle whose three vertices have z > near: pixels ceil(umin - 0.5) .. floor(umax + 0.5) (v alike) of the projected
//              vertices, clipped to the image -- half a pixel more than the hull on every side, far beyond the projection's rounding.
//              A triangle with a vertex at z <= near counts as LARGE and takes the box of its part at z >= near -- its vertices there
//              and the points where its edges meet the plane z = near, each a + t (b - a) with t = (near - az) / (bz - az) -- grown
//              by 1 + 2^-16 max|u| pixels for the rounding of those points (their error, about 2^-22 of the coordinates' size, is
//              multiplied by f / near); a projection that is not a number takes the whole image; a triangle with all three
//              z < near, an index outside the vertices or a non-finite coordinate takes nothing.  The box decides only WHICH pixels
//              are tested, never what a test says: the plane is a minimum over hits and does not depend on boxes, lanes or order.
//   SEEN       vertex p is seen by a view when z > 0, its pixel (i, j) has edge <= i <= W - 1 - edge and edge <= j <= H - 1 - edge,
//              and, with a depth plane, d = depth[j][i] > 0 and z <= d + eps (one float32 addition).
//
// Every float32 step is an operation of its own (mr_add / _sub / _mul / _div: operators under `#pragma clang fp contract(off)` on the
// device, plain operators under -ffp-contract=off on the host), so host and device give the same bits.
#pragma once

#include <math.h>
#include <stdint.h>

#include "splat_math.h"

namespace splat {

#if defined(__HIP_DEVICE_COMPILE__)
SPLAT_HD float mr_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
SPLAT_HD float mr_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
SPLAT_HD float mr_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
SPLAT_HD float mr_div(float a, float b) { return __fdiv_rn(a, b); }
#else
SPLAT_HD float mr_add(float a, float b) { return a + b; }
SPLAT_HD float mr_sub(float a, float b) { return a - b; }
SPLAT_HD float mr_mul(float a, float b) { return a * b; }
SPLAT_HD float mr_div(float a, float b) { return a / b; }
#endif

constexpr int kMrSplit = 16;            // a box of more pixels than this is spread over a wave: measured against 1 .. 256 (profiles/mesh_render.md 2)
constexpr int kMrNothing = 0, kMrSmall = 1, kMrLarge = 2;
constexpr float kMrClipMargin = 1.0f / 65536.0f;   // a near-clipped box grows by 1 + 2^-16 |u| pixels: the rounding of the points on the plane

struct MrPinhole {
    int W, H;
    float fx, fy, cx, cy;
};

// k4: (fx, fy, cx, cy)
SPLAT_HD MrPinhole mr_pinhole(int W, int H, const float *k4) {
    MrPinhole c;
    c.W = W; c.H = H;
    c.fx = k4[0]; c.fy = k4[1]; c.cx = k4[2]; c.cy = k4[3];
    return c;
}

struct MrFace {
    float e[3][3];                      // edge planes ab, bc, ca
    float n[3], na;                     // normal and n . a
    int i0, i1, j0, j1;                 // the box, inclusive, inside the image
    int kind;                           // kMrNothing / kMrSmall / kMrLarge
};

SPLAT_HD bool mr_finite(float x) { return mr_sub(x, x) == 0.f; }

// row of w2c applied to p: ((m0 x + m1 y) + m2 z) + m3
SPLAT_HD float mr_cam_coord(const float *row, const float *p) {
    return mr_add(mr_add(mr_add(mr_mul(row[0], p[0]), mr_mul(row[1], p[1])), mr_mul(row[2], p[2])), row[3]);
}
SPLAT_HD void mr_to_camera(const float *m, const float *p, float *pc) {
    pc[0] = mr_cam_coord(m, p);
    pc[1] = mr_cam_coord(m + 4, p);
    pc[2] = mr_cam_coord(m + 8, p);
}

SPLAT_HD void mr_cross(const float *a, const float *b, float *c) {
    c[0] = mr_sub(mr_mul(a[1], b[2]), mr_mul(a[2], b[1]));
    c[1] = mr_sub(mr_mul(a[2], b[0]), mr_mul(a[0], b[2]));
    c[2] = mr_sub(mr_mul(a[0], b[1]), mr_mul(a[1], b[0]));
}

// a x b, formed from the endpoint of lower index first
SPLAT_HD void mr_edge(const float *a, int32_t ia, const float *b, int32_t ib, float *e) {
    if (ia <= ib) {
        mr_cross(a, b, e);
    } else {
        mr_cross(b, a, e);
        e[0] = -e[0]; e[1] = -e[1]; e[2] = -e[2];
    }
}

// the ray of pixel column i / row j
SPLAT_HD float mr_ray_x(const MrPinhole &c, int i) { return mr_div(mr_sub((float)i, c.cx), c.fx); }
SPLAT_HD float mr_ray_y(const MrPinhole &c, int j) { return mr_div(mr_sub((float)j, c.cy), c.fy); }

SPLAT_HD float mr_plane(const float *e, float dx, float dy) { return mr_add(mr_add(mr_mul(dx, e[0]), mr_mul(dy, e[1])), e[2]); }

// the clipped pixel range of projected coordinates lo .. hi along an axis of `size` pixels; false when it is empty
SPLAT_HD bool mr_range(float lo, float hi, int size, int &p0, int &p1) {
    const float a = ceilf(mr_sub(lo, 0.5f)), b = floorf(mr_add(hi, 0.5f));
    if (!(b >= 0.f) || !(a <= (float)(size - 1))) return false;
    p0 = a > 0.f ? (int)a : 0;
    p1 = b < (float)(size - 1) ? (int)b : size - 1;
    return p0 <= p1;
}

// everything the per-pixel test needs of face f (three indices) seen through w2c rows m[12]; `split`: the largest box of a small face
SPLAT_HD void mr_face_setup(const MrPinhole &c, float near_z, const float *m, const float *vertices, int32_t V, const int32_t *f, int split,
                            MrFace &out) {
    out.kind = kMrNothing;
    out.i0 = out.j0 = 0;
    out.i1 = out.j1 = -1;
    if (!(f[0] >= 0 && f[0] < V && f[1] >= 0 && f[1] < V && f[2] >= 0 && f[2] < V)) return;
    float p[3][3];
    for (int k = 0; k < 3; ++k) {
        const float *w = vertices + 3 * (int64_t)f[k];
        if (!(mr_finite(w[0]) && mr_finite(w[1]) && mr_finite(w[2]))) return;
        mr_to_camera(m, w, p[k]);
    }
    if (p[0][2] < near_z && p[1][2] < near_z && p[2][2] < near_z) return;          // (a hit lies between the vertices' depths)
    mr_edge(p[0], f[0], p[1], f[1], out.e[0]);
    mr_edge(p[1], f[1], p[2], f[2], out.e[1]);
    mr_edge(p[2], f[2], p[0], f[0], out.e[2]);
    float ab[3], ac[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = mr_sub(p[1][k], p[0][k]);
        ac[k] = mr_sub(p[2][k], p[0][k]);
    }
    mr_cross(ab, ac, out.n);
    out.na = mr_add(mr_add(mr_mul(out.n[0], p[0][0]), mr_mul(out.n[1], p[0][1])), mr_mul(out.n[2], p[0][2]));
    out.i0 = 0; out.i1 = c.W - 1; out.j0 = 0; out.j1 = c.H - 1;
    out.kind = kMrLarge;
    const bool crossing = !(p[0][2] > near_z && p[1][2] > near_z && p[2][2] > near_z);
    float ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    for (int k = 0; k < 3; ++k) {
        const int l = k == 2 ? 0 : k + 1;
        float q[2][3];
        int count = 0;
        if (!crossing || p[k][2] >= near_z) {
            q[0][0] = p[k][0]; q[0][1] = p[k][1]; q[0][2] = p[k][2];
            count = 1;
        }
        if (crossing && (p[k][2] < near_z) != (p[l][2] < near_z)) {    // the edge meets the plane z = near
            const float t = mr_div(mr_sub(near_z, p[k][2]), mr_sub(p[l][2], p[k][2]));
            q[count][0] = mr_add(p[k][0], mr_mul(t, mr_sub(p[l][0], p[k][0])));
            q[count][1] = mr_add(p[k][1], mr_mul(t, mr_sub(p[l][1], p[k][1])));
            q[count][2] = near_z;
            ++count;
        }
        for (int a = 0; a < count; ++a) {
            const float u = mr_add(mr_div(mr_mul(c.fx, q[a][0]), q[a][2]), c.cx), v = mr_add(mr_div(mr_mul(c.fy, q[a][1]), q[a][2]), c.cy);
            if (!(mr_finite(u) && mr_finite(v))) return;                 // the box is unknown: the whole image
            ulo = fminf(ulo, u); uhi = fmaxf(uhi, u);
            vlo = fminf(vlo, v); vhi = fmaxf(vhi, v);
        }
    }
    if (!(ulo <= uhi)) return;                                           // (a vertex that is not a number: the whole image, where every test fails)
    if (crossing) {                                                      // the points on the plane carry the rounding of the intersection
        const float mu = mr_add(1.f, mr_mul(kMrClipMargin, fmaxf(fabsf(ulo), fabsf(uhi)))), mv = mr_add(1.f, mr_mul(kMrClipMargin, fmaxf(fabsf(vlo), fabsf(vhi))));
        ulo = mr_sub(ulo, mu); uhi = mr_add(uhi, mu);
        vlo = mr_sub(vlo, mv); vhi = mr_add(vhi, mv);
    }
    if (!mr_range(ulo, uhi, c.W, out.i0, out.i1) || !mr_range(vlo, vhi, c.H, out.j0, out.j1)) {
        out.kind = kMrNothing;
        return;
    }
    const int64_t area = (int64_t)(out.i1 - out.i0 + 1) * (out.j1 - out.j0 + 1);
    out.kind = !crossing && area <= (int64_t)split ? kMrSmall : kMrLarge;
}

// the depth at which the ray (dx, dy, 1) meets the face; false when it does not, or not at near <= z < +inf
SPLAT_HD bool mr_hit(const MrFace &f, float near_z, float dx, float dy, float &z) {
    const float e0 = mr_plane(f.e[0], dx, dy), e1 = mr_plane(f.e[1], dx, dy), e2 = mr_plane(f.e[2], dx, dy);
    if (!((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f))) return false;
    z = mr_div(f.na, mr_plane(f.n, dx, dy));
    return z >= near_z && z < INFINITY;
}

// One walker alone over a face's own box, row by row: sink(offset, z) for every pixel the face hits, offset = j W + i (it fits 32
// bits: a view has fewer than 2^30 pixels).  Returns the pixel tests made: the box's area, at most width x height.  The one-lane
// branch of the device walk (mesh_device.h) and the host models of the depth and the key plane are this loop.
template <typename Sink>
SPLAT_HD long long mr_walk_box(const MrPinhole &c, const MrFace &f, float near_z, Sink sink) {
    long long tests = 0;
    for (int j = f.j0; j <= f.j1; ++j) {
        const float dy = mr_ray_y(c, j);
        for (int i = f.i0; i <= f.i1; ++i) {
            float z;
            ++tests;
            if (mr_hit(f, near_z, mr_ray_x(c, i), dy, z)) sink((uint32_t)j * c.W + i, z);
        }
    }
    return tests;
}

// whether the view with w2c rows m[12] sees p; `depth` (or NULL): the view's plane
SPLAT_HD bool mr_seen(const MrPinhole &c, const float *m, const float *p, int edge, const float *depth, float eps) {
    const float z = mr_cam_coord(m + 8, p);
    if (!(z > 0.f)) return false;
    const float x = mr_cam_coord(m, p), y = mr_cam_coord(m + 4, p);
    const float u = mr_add(mr_div(mr_mul(c.fx, x), z), c.cx), v = mr_add(mr_div(mr_mul(c.fy, y), z), c.cy);
    const float uf = floorf(mr_add(u, 0.5f)), vf = floorf(mr_add(v, 0.5f));
    if (!(uf >= (float)edge && uf <= (float)(c.W - 1 - edge) && vf >= (float)edge && vf <= (float)(c.H - 1 - edge))) return false;
    if (!depth) return true;
    const float d = depth[(size_t)(int)vf * c.W + (int)uf];
    return d > 0.f && z <= mr_add(d, eps);
}

}  // namespace splat
