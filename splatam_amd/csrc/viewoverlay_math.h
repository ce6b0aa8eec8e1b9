// viewoverlay_math.h -- arithmetic of the view overlay (viewoverlay.hip): the cameras of a run as line segments, Gaussian centres as
// points, both in ONE depth-tested key plane, and the pass that puts the winners' bytes into a picture.  Written once as host/device
// inline functions: the kernels call them per lane, tests/test_viewoverlay_cpu.py compiles the very same header with g++
// (tests/viewoverlay_math_shim.cpp, -ffp-contract=off) and checks it against the float64 numpy form of the same definitions
// (tests/viewoverlay_ref.py).
//
//   KEY      (bits(z) << 32) | id, entered by unsigned 64-bit minimum into a plane cleared to all ones (meshshade_math.h's msh_key and
//            kMshNoKey).  z: float32 camera-space depth, positive, so its bits order like the floats.  id: bit 31 set = a segment, the
//            other bits its index in the segment array; bit 31 clear = a row of the map.  Equal depth bits resolve to the lowest id:
//            points win over segments.  A minimum: the same bits on every run and for every order of the launches.
//   RUN      frame t of a run -> nine segments.  The pose is view_math.h's (first_w2c . rel_w2c[t] from the map's pose parameters, or
//            a given w2c), c2w its rigid inverse.  FRUSTUM: apex at the camera centre, corners c2w (K^-1 (u, v, 1) scale) for
//            (u, v) = (0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1); segments apex-corner x 4, then the rectangle 1-2, 2-3, 3-4, 4-1.
//            This is a STATED definition (Open3D's create_camera_visualization as recalled; Open3D is not available to compare with,
//            no parity is claimed).  TRAJECTORY: centre t - 1 -> centre t, t > 0.  Colours: cool(x), x = 0.5 t / n for frustum t,
//            x = 0.5 j / (n - 1) + 0.5 for trajectory segment j = t - 1 (n frames).  cool: matplotlib's 256-entry map, entry
//            i = (i / 255, 1 - i / 255, 1), index min(int(256 x), 255), as the bytes round(255 v) = (i, 255 - i, 255) -- rounded to
//            nearest as view_byte rounds every colour of the view layer (matplotlib's own `bytes=True` truncates, and its table sits
//            an ulp below i / 255 in places: 62 of its bytes are one lower).  Layout of a block:
//            trajectory segments [0, n - 1), then eight per frame from n - 1 in frame order -- a prefix of each part is "the run up
//            to t".  Evaluated in double, every endpoint rounded once.
//   POINT    pc = w2c p as the mesh layers form it (meshrender_math.h mr_cam_coord); skipped unless pc.z > near; pixel
//            (floor(fx x / z + cx + 0.5), floor(fy y / z + cy + 0.5)); footprint: the square of `size` pixels from pixel - (size - 1) / 2
//            (integer division), clipped to the image.
//   SEGMENT  endpoints ordered (lexicographically, by their float32 world coordinates: a segment and its reverse are the SAME input from
//            here on), to the camera in double, clipped to z >= near, projected (u = fx x / z + cx), clipped to the rectangle
//            [-0.5, W - 0.5] x [-0.5, H - 0.5] of the pixels' squares (Liang-Barsky), turned so that the walk starts at the smaller
//            major-axis coordinate (major: the axis of the larger extent, x on a tie).  The steps are the pixel centres the clipped span
//            covers along the major axis, m = ceil(major0) .. floor(major1): the clip's edges lie half a pixel from every centre, so a
//            clipped end never sits on a rounding boundary, and consecutive segments of a polyline share no step.  A span that covers
//            no centre (a zero-length segment among them) gets ONE step at floor(major0 + 0.5).  At most max(W, H) + 1 steps after the
//            clip, and clamped to that.  The
//            step's parameter s = clamp((m - major0) / (major1 - major0), 0, 1) gives the minor pixel floor(minor(s) + 0.5) and the
//            depth 1 / (w0 + s (w1 - w0)) with w = 1 / z (linear in screen space), rounded to float32 once.  Width: `width` pixels
//            along the minor axis from minor - (width - 1) / 2.  A non-finite endpoint or a segment wholly behind `near` gives no
//            step; a zero-length segment one.
//   RESOLVE  a pixel whose key is not all ones: z its high word, d the scene's depth there (none: 0); the primitive's bytes replace
//            the pixel's iff occlusion is off, or d <= 0, or z <= d.  A point's bytes: view_byte(view_clamp01(rgb_colors[row][c]));
//            a segment's: its stored colour.
//
// Every function with arithmetic in it is compiled without contraction (VO_EXACT on the device, -ffp-contract=off on the host), and the
// double divisions are msh_divd's, so host and device walk the same pixels and form the same keys.
#pragma once

#include <math.h>
#include <stdint.h>

#include "meshshade_math.h"

#if defined(__clang__)
#define VO_EXACT _Pragma("clang fp contract(off)")
#else
#define VO_EXACT
#endif

namespace splat {

constexpr uint32_t kVoSegmentBit = 0x80000000u;
constexpr int kVoFrustumSegments = 8;
constexpr int kVoMaxPointSize = 8, kVoMaxLineWidth = 4;

SPLAT_HD bool vo_finite(double x) {
    VO_EXACT
    return x - x == 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- RUN
// entry min(int(256 x), 255) of matplotlib's `cool`, (i / 255, 1 - i / 255, 1), as bytes rounded to nearest
SPLAT_HD void vo_cool(double x, uint8_t *rgb) {
    VO_EXACT
    int i = x >= 1.0 ? 255 : (x > 0.0 ? (int)(256.0 * x) : 0);      // (NaN -> 0)
    if (i > 255) i = 255;
    rgb[0] = (uint8_t)i;
    rgb[1] = (uint8_t)(255 - i);
    rgb[2] = 255;
}

struct VoRun {                          // SplatViewRun's fields
    int num_frames;                     // n: frames of the run (the stride of the pose arrays, the colours' scale, the layout)
    const float *w2c_all;               // [n][16] row-major, or NULL for the map-pose form:
    const float *cam_unnorm_rots, *cam_trans, *first_w2c;
    int w, h;
    double fx, fy, cx, cy, scale;
    int frusta;                         // 0: the trajectory alone
    int fixed;                          // != 0: every segment in `color`
    uint8_t color[3];
};

// the w2c of frame t, row-major, double
SPLAT_HD void vo_run_pose(const VoRun &r, int t, double *M) {
    if (r.w2c_all) {
        for (int i = 0; i < 16; ++i) M[i] = (double)r.w2c_all[16 * (size_t)t + i];
    } else {
        double first[16], T[16];
        for (int i = 0; i < 16; ++i) first[i] = (double)r.first_w2c[i];
        view_rel_w2c(r.cam_unnorm_rots + t, r.cam_trans + t, r.num_frames, T);
        view_mat4_mul(first, T, M);
    }
}

// the camera centre -R^T t of a rigid w2c
SPLAT_HD void vo_centre(const double *M, double *c) {
    VO_EXACT
    for (int k = 0; k < 3; ++k) c[k] = -(M[k] * M[3] + M[4 + k] * M[7] + M[8 + k] * M[11]);
}

SPLAT_HD void vo_store_segment(float *seg, const double *a, const double *b) {
    for (int k = 0; k < 3; ++k) {
        seg[k] = (float)a[k];
        seg[3 + k] = (float)b[k];
    }
}

// what frame t adds to a block: segments [.][6] floats, colors [.][3] bytes (see RUN for the layout)
SPLAT_HD void vo_run_frame(const VoRun &r, int t, float *segments, uint8_t *colors) {
    VO_EXACT
    const int n = r.num_frames;
    double M[16], c[3];
    vo_run_pose(r, t, M);
    vo_centre(M, c);
    if (t > 0) {
        double Mp[16], cp[3];
        vo_run_pose(r, t - 1, Mp);
        vo_centre(Mp, cp);
        vo_store_segment(segments + 6 * (size_t)(t - 1), cp, c);
        uint8_t *col = colors + 3 * (size_t)(t - 1);
        if (r.fixed) { col[0] = r.color[0]; col[1] = r.color[1]; col[2] = r.color[2]; }
        else vo_cool(msh_divd(0.5 * (double)(t - 1), (double)(n - 1)) + 0.5, col);
    }
    if (!r.frusta) return;
    const double us[4] = {0.0, (double)(r.w - 1), (double)(r.w - 1), 0.0}, vs[4] = {0.0, 0.0, (double)(r.h - 1), (double)(r.h - 1)};
    double p[5][3];
    for (int k = 0; k < 3; ++k) p[0][k] = c[k];
    for (int q = 0; q < 4; ++q) {
        const double X = msh_divd(us[q] - r.cx, r.fx) * r.scale, Y = msh_divd(vs[q] - r.cy, r.fy) * r.scale, Z = r.scale;
        for (int k = 0; k < 3; ++k) p[1 + q][k] = M[k] * X + M[4 + k] * Y + M[8 + k] * Z + c[k];       // R^T (X, Y, Z) + centre
    }
    const int ends[kVoFrustumSegments][2] = {{0, 1}, {0, 2}, {0, 3}, {0, 4}, {1, 2}, {2, 3}, {3, 4}, {4, 1}};
    uint8_t col[3];
    if (r.fixed) { col[0] = r.color[0]; col[1] = r.color[1]; col[2] = r.color[2]; }
    else vo_cool(msh_divd(0.5 * (double)t, (double)n), col);
    const size_t base = (size_t)(n - 1) + (size_t)kVoFrustumSegments * t;
    for (int e = 0; e < kVoFrustumSegments; ++e) {
        vo_store_segment(segments + 6 * (base + e), p[ends[e][0]], p[ends[e][1]]);
        for (int k = 0; k < 3; ++k) colors[3 * (base + e) + k] = col[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- POINT
struct VoBox {
    int i0, i1, j0, j1;                 // inclusive; empty when i0 > i1
    float z;
};
// the pixels of the centre p seen through w2c rows m[12]
SPLAT_HD VoBox vo_point(const MrPinhole &c, float near_z, const float *m, const float *p, int size) {
    VoBox b;
    b.i0 = b.j0 = 0; b.i1 = b.j1 = -1;
    b.z = mr_cam_coord(m + 8, p);
    if (!(b.z > near_z)) return b;                                  // (NaN: skipped)
    const float x = mr_cam_coord(m, p), y = mr_cam_coord(m + 4, p);
    const float u = mr_add(mr_div(mr_mul(c.fx, x), b.z), c.cx), v = mr_add(mr_div(mr_mul(c.fy, y), b.z), c.cy);
    const float uf = floorf(mr_add(u, 0.5f)), vf = floorf(mr_add(v, 0.5f));
    const float reach = (float)kVoMaxPointSize;
    if (!(uf >= -reach && uf <= (float)c.W + reach && vf >= -reach && vf <= (float)c.H + reach)) return b;     // (NaN, infinities: skipped)
    const int i = (int)uf - (size - 1) / 2, j = (int)vf - (size - 1) / 2;
    b.i0 = i < 0 ? 0 : i; b.i1 = i + size - 1 > c.W - 1 ? c.W - 1 : i + size - 1;
    b.j0 = j < 0 ? 0 : j; b.j1 = j + size - 1 > c.H - 1 ? c.H - 1 : j + size - 1;
    if (b.j0 > b.j1) { b.i0 = 0; b.i1 = -1; }
    return b;
}

// ---------------------------------------------------------------------------------------------------------------- SEGMENT
struct VoLine {
    int steps;                          // 0: nothing to draw
    int steep;                          // the major axis is y
    int m0;                             // major pixel of step 0
    double a0, a1, b0, b1, w0, w1;      // major, minor and 1 / z at the walk's two ends
};

// one side of Liang-Barsky: the part of [t0, t1] where p t <= q
SPLAT_HD bool vo_clip_side(double p, double q, double &t0, double &t1) {
    VO_EXACT
    if (p == 0.0) return q >= 0.0;
    const double r = msh_divd(q, p);
    if (p < 0.0) {
        if (r > t1) return false;
        if (r > t0) t0 = r;
    } else {
        if (r < t0) return false;
        if (r < t1) t1 = r;
    }
    return true;
}

// seg: 6 floats (two world points); m: 12 floats (w2c rows)
SPLAT_HD VoLine vo_line(const MrPinhole &c, float near_z, const float *m, const float *seg) {
    VO_EXACT
    VoLine L;
    L.steps = 0; L.steep = 0; L.m0 = 0;
    L.a0 = L.a1 = L.b0 = L.b1 = L.w0 = L.w1 = 0.0;
    // one order for a segment and its reverse
    int swap = 0;
    for (int k = 0; k < 3; ++k) {
        if (seg[k] < seg[3 + k]) break;
        if (seg[k] > seg[3 + k]) { swap = 1; break; }
    }
    const float *pa = seg + (swap ? 3 : 0), *pb = seg + (swap ? 0 : 3);
    double A[3], B[3];
    for (int r = 0; r < 3; ++r) {
        A[r] = (double)m[4 * r] * (double)pa[0] + (double)m[4 * r + 1] * (double)pa[1] + (double)m[4 * r + 2] * (double)pa[2] + (double)m[4 * r + 3];
        B[r] = (double)m[4 * r] * (double)pb[0] + (double)m[4 * r + 1] * (double)pb[1] + (double)m[4 * r + 2] * (double)pb[2] + (double)m[4 * r + 3];
        if (!vo_finite(A[r]) || !vo_finite(B[r])) return L;
    }
    const double zn = (double)near_z;
    if (A[2] < zn && B[2] < zn) return L;
    if (A[2] < zn || B[2] < zn) {                                   // (then the two depths differ)
        double *in = A[2] < zn ? B : A, *out = A[2] < zn ? A : B;
        const double t = msh_divd(zn - in[2], out[2] - in[2]);
        out[0] = in[0] + t * (out[0] - in[0]);
        out[1] = in[1] + t * (out[1] - in[1]);
        out[2] = zn;
    }
    double u0 = msh_divd((double)c.fx * A[0], A[2]) + (double)c.cx, v0 = msh_divd((double)c.fy * A[1], A[2]) + (double)c.cy;
    double u1 = msh_divd((double)c.fx * B[0], B[2]) + (double)c.cx, v1 = msh_divd((double)c.fy * B[1], B[2]) + (double)c.cy;
    double w0 = msh_divd(1.0, A[2]), w1 = msh_divd(1.0, B[2]);
    if (!vo_finite(u0) || !vo_finite(v0) || !vo_finite(u1) || !vo_finite(v1)) return L;
    const double du = u1 - u0, dv = v1 - v0;
    double t0 = 0.0, t1 = 1.0;
    if (!vo_clip_side(-du, u0 + 0.5, t0, t1) || !vo_clip_side(du, ((double)c.W - 0.5) - u0, t0, t1)
        || !vo_clip_side(-dv, v0 + 0.5, t0, t1) || !vo_clip_side(dv, ((double)c.H - 0.5) - v0, t0, t1))
        return L;
    const double dw = w1 - w0;
    if (t1 < 1.0) { u1 = u0 + t1 * du; v1 = v0 + t1 * dv; w1 = w0 + t1 * dw; }
    if (t0 > 0.0) { u0 = u0 + t0 * du; v0 = v0 + t0 * dv; w0 = w0 + t0 * dw; }
    // (t du is rounded: far-away endpoints can land a whisker -- or, at 1e30 pixels, anywhere -- outside the rectangle they were clipped to)
    const double ulo = -0.5, uhi = (double)c.W - 0.5, vlo = -0.5, vhi = (double)c.H - 0.5;
    u0 = fmin(fmax(u0, ulo), uhi); u1 = fmin(fmax(u1, ulo), uhi);
    v0 = fmin(fmax(v0, vlo), vhi); v1 = fmin(fmax(v1, vlo), vhi);
    L.steep = fabs(v1 - v0) > fabs(u1 - u0) ? 1 : 0;
    L.a0 = L.steep ? v0 : u0; L.a1 = L.steep ? v1 : u1;
    L.b0 = L.steep ? u0 : v0; L.b1 = L.steep ? u1 : v1;
    L.w0 = w0; L.w1 = w1;
    if (L.a0 > L.a1) {
        double s;
        s = L.a0; L.a0 = L.a1; L.a1 = s;
        s = L.b0; L.b0 = L.b1; L.b1 = s;
        s = L.w0; L.w0 = L.w1; L.w1 = s;
    }
    // (inside the clip rectangle: |a| <= max(W, H) + 0.5, the conversions below cannot overflow)
    const int limit = (c.W > c.H ? c.W : c.H) + 1;
    L.m0 = (int)ceil(L.a0);
    const int steps = (int)floor(L.a1) - L.m0 + 1;
    if (steps < 1) L.m0 = (int)floor(L.a0 + 0.5);                   // no pixel centre inside the span: one stamp where it starts
    L.steps = steps < 1 ? 1 : (steps > limit ? limit : steps);
    return L;
}

// step k of the walk: the pixel (i, j) of its centre line and its depth
SPLAT_HD void vo_line_step(const VoLine &L, int k, int &i, int &j, float &z) {
    VO_EXACT
    const double span = L.a1 - L.a0;
    double s = span > 0.0 ? msh_divd((double)(L.m0 + k) - L.a0, span) : 0.0;
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    const int major = L.m0 + k, minor = (int)floor(L.b0 + s * (L.b1 - L.b0) + 0.5);
    i = L.steep ? minor : major;
    j = L.steep ? major : minor;
    z = (float)msh_divd(1.0, L.w0 + s * (L.w1 - L.w0));
}

// the pixels of step k at `width`: sink(offset, z) for each one inside the image
template <class Sink>
SPLAT_HD void vo_line_stamp(const MrPinhole &c, const VoLine &L, int k, int width, Sink sink) {
    int i, j;
    float z;
    vo_line_step(L, k, i, j, z);
    const int lo = (L.steep ? i : j) - (width - 1) / 2;
    for (int q = lo; q < lo + width; ++q) {
        const int x = L.steep ? q : i, y = L.steep ? j : q;
        if (x >= 0 && x < c.W && y >= 0 && y < c.H) sink((uint32_t)y * (uint32_t)c.W + (uint32_t)x, z);
    }
}

// ---------------------------------------------------------------------------------------------------------------- RESOLVE
struct VoResolve {
    int occlude;
    const float *rgb_colors;            // [rows][3]
    int rows;
    const uint8_t *segment_colors;      // [segments][3]
    int segments;
};
// whether `key` changes the pixel whose scene depth is d (0: none), and to which bytes
SPLAT_HD bool vo_resolve(const VoResolve &a, uint64_t key, float d, uint8_t *out) {
    if (key == kMshNoKey) return false;
    const float z = msh_float((uint32_t)(key >> 32));
    if (!(!a.occlude || d <= 0.f || z <= d)) return false;
    const uint32_t id = (uint32_t)key;
    if (id & kVoSegmentBit) {
        const uint32_t s = id & ~kVoSegmentBit;
        if (s >= (uint32_t)(a.segments > 0 ? a.segments : 0)) return false;
        for (int k = 0; k < 3; ++k) out[k] = a.segment_colors[3 * (size_t)s + k];
    } else {
        if (id >= (uint32_t)(a.rows > 0 ? a.rows : 0)) return false;
        for (int k = 0; k < 3; ++k) out[k] = view_byte(view_clamp01(a.rgb_colors[3 * (size_t)id + k]));
    }
    return true;
}

}  // namespace splat
