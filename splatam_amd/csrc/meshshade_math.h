// meshshade_math.h -- arithmetic of the mesh shade layer (meshshade.hip), written once as host/device inline functions: the kernels
// call them per lane, tests/test_meshshade_cpu.py compiles the very same header with g++ (tests/meshshade_math_shim.cpp,
// -ffp-contract=off) and checks it against the float64 numpy restatement tests/meshshade_ref.py.  The camera, the edge planes, the
// coverage test and the hit are meshrender_math.h's, unchanged (MrPinhole, MrFace, mr_face_setup, mr_hit, mr_ray_x / _y).
//
//   NORMALS    area-weighted vertex normals.  A face adds n = (b - a) x (c - a), formed in DOUBLE from the float32 vertices (one
//              operation per step), to its three vertices as QUANTA: q_k = rint(n_k 2^40), ties to even -- the quanta of meshclean's
//              areas (SPLAT_MESH_AREA_BITS) -- by 64-bit integer adds, which are exact and independent of order.  A face with an index
//              outside the vertices, a non-finite vertex or a component with |n_k| >= 2^22 m^2 adds NOTHING; a face with a repeated
//              index has n = 0 and adds nothing either.  A vertex holds 2^23 m^2 per component and wraps beyond.  The normal of a
//              vertex is (x, y, z) / s, s = sqrt((x^2 + y^2) + z^2) on the integer sums converted to double, each component rounded
//              ONCE to float32; s == 0 (a vertex no face names, or faces that cancel) gives (0, 0, 0).  sqrt(x x) = |x| in binary
//              floating point, so a vertex whose faces are coplanar with an axis plane gets EXACTLY +-1 and two zeros.
//   KEY        of a hit: ((uint64)bits(z) << 32) | face index.  z >= near > 0, so the bits order as the values and an unsigned 64-bit
//              minimum keeps the nearest hit and, among faces that hit at the same z bits (every pixel on a shared edge), the LOWEST
//              face index.  A plane of keys is cleared to all ones; its high words are what the depth plane holds before +inf -> 0.
//   SAMPLE     one sub-pixel of the key plane.  A key of all ones, a face index >= F and a face mr_face_setup turns away (an index
//              outside the vertices, a non-finite vertex, all of it nearer than near_z, a box outside the image: never the winner of
//              a pixel) are BACKGROUND.  Otherwise the edge planes of
//              the winning face at the sub-pixel's ray d give perspective-correct barycentrics without a division by w -- they are
//              homogeneous in camera space --: S = (E_ab + E_bc) + E_ca, l_a = E_bc / S, l_b = E_ca / S, l_c = E_ab / S; S == 0: thirds.
//              An attribute is (l_a x_a + l_b x_b) + l_c x_c.  The colour is the interpolated vertex colour, `albedo` without colours.
//              The normal is the interpolated vertex normal divided by its length sqrt((x^2 + y^2) + z^2); where that length is 0 or
//              not finite, with smooth == 0 or without normals it is the face's own (b - a) x (c - a) from the WORLD-frame vertices in
//              float32, normalised alike ((0, 0, 0) for a face without area).  The stored z is the key's high word, never recomputed.
//   LIGHT      a head light, two-sided: L = ambient + (1 - ambient) |n . w| / |w|, w = R^T d the ray in the mesh's frame
//              (w_k = (m[k] dx + m[4 + k] dy) + m[8 + k]).  Winding never blackens a picture.
//   MODES      COLOR: the colour.  SHADED: albedo L.  SHADED_COLOR: colour L.  NORMAL: (n + 1) / 2, n in the mesh's frame
//              (normal_frame 0) or in the camera's, n_c = R n, negated where n_c . d > 0 so that it faces the viewer (1).  DEPTH: the
//              row view_depth_index(z, vmin, vmax) of `lut`, each byte / 255 -- view_pixel_bytes' bytes once view_byte has rounded.
//              Background is `bg` in every mode.
//   PIXEL      an OUTPUT pixel (i, j) sums the channel values of its samples x samples sub-pixels (i s + a, j s + b) in row order in
//              float32, multiplies by 1 / s^2 (one division, one product), clamps to 0..1 and rounds with view_byte.
//
// Every float32 step is an operation of its own (mr_add / _sub / _mul / _div, msh_sqrt), every double step likewise (ms_subd / _muld /
// _addd / _sqrtd, msh_divd): host and device give the same bits.
#pragma once

#include <math.h>
#include <stdint.h>

#include "meshrender_math.h"
#include "meshclean_math.h"
#include "view_math.h"

namespace splat {

#if defined(__HIP_DEVICE_COMPILE__)
// (through double: the correctly rounded float32 root whatever the compiler makes of a float sqrt -- 53 >= 2 x 24 + 2 bits, so the
// second rounding changes nothing; __fsqrt_rn is the hardware's approximate root here and was 2 ulps off the host's)
SPLAT_HD float msh_sqrt(float a) { return (float)__dsqrt_rn((double)a); }
SPLAT_HD double msh_divd(double a, double b) { return __ddiv_rn(a, b); }
SPLAT_HD uint32_t msh_bits(float z) { return __float_as_uint(z); }
SPLAT_HD float msh_float(uint32_t b) { return __uint_as_float(b); }
#else
SPLAT_HD float msh_sqrt(float a) { return sqrtf(a); }
SPLAT_HD double msh_divd(double a, double b) { return a / b; }
SPLAT_HD uint32_t msh_bits(float z) {
    union {
        float f;
        uint32_t u;
    } v;
    v.f = z;
    return v.u;
}
SPLAT_HD float msh_float(uint32_t b) {
    union {
        float f;
        uint32_t u;
    } v;
    v.u = b;
    return v.f;
}
#endif

constexpr uint64_t kMshNoKey = ~(uint64_t)0;
constexpr int kMshColor = 0, kMshShaded = 1, kMshShadedColor = 2, kMshNormal = 3, kMshDepth = 4;     // SPLAT_MESH_SHADE_*
constexpr int kMshMaxSamples = 4;

// ---------------------------------------------------------------------------------------------------------------- normals
// the quanta face f adds to each of its three vertices; false: it adds nothing
SPLAT_HD bool msh_face_quanta(const float *vertices, int32_t V, const int32_t *f, int64_t *q) {
    if (!ms_face_valid(f, V)) return false;
    const float *a = vertices + 3 * (int64_t)f[0], *b = vertices + 3 * (int64_t)f[1], *c = vertices + 3 * (int64_t)f[2];
    for (int k = 0; k < 3; ++k)
        if (!(mr_finite(a[k]) && mr_finite(b[k]) && mr_finite(c[k]))) return false;
    double ab[3], ac[3], n[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = ms_subd((double)b[k], (double)a[k]);
        ac[k] = ms_subd((double)c[k], (double)a[k]);
    }
    n[0] = ms_subd(ms_muld(ab[1], ac[2]), ms_muld(ab[2], ac[1]));
    n[1] = ms_subd(ms_muld(ab[2], ac[0]), ms_muld(ab[0], ac[2]));
    n[2] = ms_subd(ms_muld(ab[0], ac[1]), ms_muld(ab[1], ac[0]));
    for (int k = 0; k < 3; ++k)
        if (!(fabs(n[k]) < kMcFaceAreaLimit)) return false;
    for (int k = 0; k < 3; ++k) q[k] = (int64_t)mc_rint(ms_muld(n[k], kMcAreaScale));
    return (q[0] | q[1] | q[2]) != 0;
}

// one face: its quanta to accum [V][3] (64-bit integer adds)
SPLAT_HD void msh_add_face(const float *vertices, int32_t V, const int32_t *f, int64_t *accum) {
    int64_t q[3];
    if (!msh_face_quanta(vertices, V, f, q)) return;
    for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k)
            if (q[k] != 0) mc_add64(accum + 3 * (int64_t)f[v] + k, q[k]);
}

// one vertex: its three sums to a unit normal, or zeros
SPLAT_HD void msh_vertex_normal(const int64_t *acc, float *n) {
    const double x = (double)acc[0], y = (double)acc[1], z = (double)acc[2];
    const double s = ms_sqrtd(ms_addd(ms_addd(ms_muld(x, x), ms_muld(y, y)), ms_muld(z, z)));
    if (!(s > 0.0)) {
        n[0] = n[1] = n[2] = 0.f;
        return;
    }
    n[0] = (float)msh_divd(x, s);
    n[1] = (float)msh_divd(y, s);
    n[2] = (float)msh_divd(z, s);
}

// ---------------------------------------------------------------------------------------------------------------- keys
SPLAT_HD uint64_t msh_key(float z, uint32_t face) { return ((uint64_t)msh_bits(z) << 32) | (uint64_t)face; }

// ---------------------------------------------------------------------------------------------------------------- shading
struct MshShade {                       // SplatMeshShade's fields
    int mode, samples, smooth, normal_frame;
    float bg[3], albedo[3], ambient, vmin, vmax;
    const uint8_t *lut;
};

struct MshSample {
    float rgb[3];                       // channel values in 0..1 (before the clamp)
    float n[3];                         // the shading normal in the mesh's frame; zeros on the background
    float z;                            // the key's depth; 0 on the background
    int32_t face;                       // -1 on the background
};

SPLAT_HD float msh_dot(const float *a, const float *b) { return mr_add(mr_add(mr_mul(a[0], b[0]), mr_mul(a[1], b[1])), mr_mul(a[2], b[2])); }
SPLAT_HD float msh_mix(const float *l, float xa, float xb, float xc) { return mr_add(mr_add(mr_mul(l[0], xa), mr_mul(l[1], xb)), mr_mul(l[2], xc)); }

// v / |v| into out; false (out untouched) when the length is 0 or not finite
SPLAT_HD bool msh_unit(const float *v, float *out) {
    const float len = msh_sqrt(msh_dot(v, v));
    if (!(len > 0.f) || !mr_finite(len)) return false;
    out[0] = mr_div(v[0], len); out[1] = mr_div(v[1], len); out[2] = mr_div(v[2], len);
    return true;
}

// the barycentrics (of a, b, c) of face g at the ray (dx, dy, 1)
SPLAT_HD void msh_barycentrics(const MrFace &g, float dx, float dy, float *l) {
    const float eab = mr_plane(g.e[0], dx, dy), ebc = mr_plane(g.e[1], dx, dy), eca = mr_plane(g.e[2], dx, dy);
    const float S = mr_add(mr_add(eab, ebc), eca);
    if (S == 0.f) {
        l[0] = l[1] = l[2] = 1.f / 3.f;
        return;
    }
    l[0] = mr_div(ebc, S); l[1] = mr_div(eca, S); l[2] = mr_div(eab, S);
}

// sub-pixel (i, j) of the key plane that `cam` describes; m: the 12 floats of w2c's first three rows
SPLAT_HD void msh_sample(const MrPinhole &cam, float near_z, const float *m, const float *vertices, int32_t V, const int32_t *faces, int32_t F,
                         const float *colors, const float *normals, const MshShade &a, uint64_t key, int i, int j, MshSample &o) {
    o.rgb[0] = a.bg[0]; o.rgb[1] = a.bg[1]; o.rgb[2] = a.bg[2];
    o.n[0] = o.n[1] = o.n[2] = 0.f;
    o.z = 0.f;
    o.face = -1;
    const uint32_t id = (uint32_t)(key & 0xffffffffu);
    if (key == kMshNoKey || F <= 0 || id >= (uint32_t)F) return;
    const int32_t idx[3] = {faces[3 * (int64_t)id], faces[3 * (int64_t)id + 1], faces[3 * (int64_t)id + 2]};
    MrFace g;
    mr_face_setup(cam, near_z, m, vertices, V, idx, kMrSplit, g);       // (checks the three indices before it loads a vertex)
    if (g.kind == kMrNothing) return;                                   // (its planes may not have been formed)
    const float *pa = vertices + 3 * (int64_t)idx[0], *pb = vertices + 3 * (int64_t)idx[1], *pc = vertices + 3 * (int64_t)idx[2];
    const float dx = mr_ray_x(cam, i), dy = mr_ray_y(cam, j);
    float l[3];
    msh_barycentrics(g, dx, dy, l);
    o.face = (int32_t)id;
    o.z = msh_float((uint32_t)(key >> 32));
    float colour[3];
    for (int c = 0; c < 3; ++c)
        colour[c] = colors ? msh_mix(l, colors[3 * (int64_t)idx[0] + c], colors[3 * (int64_t)idx[1] + c], colors[3 * (int64_t)idx[2] + c]) : a.albedo[c];
    bool have = false;
    if (a.smooth && normals) {
        float s[3];
        for (int c = 0; c < 3; ++c) s[c] = msh_mix(l, normals[3 * (int64_t)idx[0] + c], normals[3 * (int64_t)idx[1] + c], normals[3 * (int64_t)idx[2] + c]);
        have = msh_unit(s, o.n);
    }
    if (!have) {
        float ab[3], ac[3], fn[3];
        for (int k = 0; k < 3; ++k) {
            ab[k] = mr_sub(pb[k], pa[k]);
            ac[k] = mr_sub(pc[k], pa[k]);
        }
        mr_cross(ab, ac, fn);
        msh_unit(fn, o.n);                                              // (no area: the zeros stay)
    }
    if (a.mode == kMshColor) {
        for (int c = 0; c < 3; ++c) o.rgb[c] = colour[c];
    } else if (a.mode == kMshShaded || a.mode == kMshShadedColor) {
        const float w[3] = {mr_add(mr_add(mr_mul(m[0], dx), mr_mul(m[4], dy)), m[8]), mr_add(mr_add(mr_mul(m[1], dx), mr_mul(m[5], dy)), m[9]),
                            mr_add(mr_add(mr_mul(m[2], dx), mr_mul(m[6], dy)), m[10])};
        const float t = mr_div(fabsf(msh_dot(o.n, w)), msh_sqrt(msh_dot(w, w)));
        const float L = mr_add(a.ambient, mr_mul(mr_sub(1.f, a.ambient), t));
        for (int c = 0; c < 3; ++c) o.rgb[c] = mr_mul(a.mode == kMshShaded ? a.albedo[c] : colour[c], L);
    } else if (a.mode == kMshNormal) {
        float n[3] = {o.n[0], o.n[1], o.n[2]};
        if (a.normal_frame) {
            for (int r = 0; r < 3; ++r) n[r] = msh_dot(m + 4 * r, o.n);
            if (mr_plane(n, dx, dy) > 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        }
        for (int c = 0; c < 3; ++c) o.rgb[c] = mr_mul(mr_add(n[c], 1.f), 0.5f);
    } else {
        const uint8_t *row = a.lut + 3 * view_depth_index(o.z, a.vmin, a.vmax);
        for (int c = 0; c < 3; ++c) o.rgb[c] = mr_div((float)row[c], 255.f);
    }
}

// OUTPUT pixel (i, j): rgb8[3]; with samples == 1 also the sample itself (planes)
SPLAT_HD void msh_pixel(const MrPinhole &cam, float near_z, const float *m, const float *vertices, int32_t V, const int32_t *faces, int32_t F,
                        const float *colors, const float *normals, const MshShade &a, const uint64_t *keys, int i, int j, uint8_t *rgb8,
                        MshSample &last) {
    const int s = a.samples;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int b = 0; b < s; ++b)
        for (int c = 0; c < s; ++c) {
            const int si = i * s + c, sj = j * s + b;
            msh_sample(cam, near_z, m, vertices, V, faces, F, colors, normals, a, keys[(size_t)sj * cam.W + si], si, sj, last);
            for (int k = 0; k < 3; ++k) acc[k] = mr_add(acc[k], last.rgb[k]);
        }
    const float inv = mr_div(1.f, (float)(s * s));
    for (int k = 0; k < 3; ++k) rgb8[k] = view_byte(view_clamp01(mr_mul(acc[k], inv)));
}

}  // namespace splat
