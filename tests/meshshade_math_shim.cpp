// Host build of splatam_amd/csrc/meshshade_math.h for tests/test_meshshade_cpu.py (and, as the bit-exact reference of every kernel, for
// tests/test_gpu_meshshade.py): plain-loop models of the kernels of csrc/meshshade.hip that call nothing but the header's functions.
// Built with -ffp-contract=off: every float32 and double step of the header is then one operation, as on the device.
#include <string.h>

#include "../splatam_amd/csrc/meshshade_math.h"

using namespace splat;

extern "C" {

// N0 - N2: accum [V][3] is scratch, normals [V][3]
int msh_vertex_normals(const float *vertices, int32_t V, const int32_t *faces, int32_t F, int64_t *accum, float *normals) {
    if (V < 0 || F < 0) return -1;
    for (int64_t k = 0; k < 3 * (int64_t)V; ++k) accum[k] = 0;
    for (int32_t f = 0; f < F; ++f) msh_add_face(vertices, V, faces + 3 * (int64_t)f, accum);
    for (int32_t v = 0; v < V; ++v) msh_vertex_normal(accum + 3 * (int64_t)v, normals + 3 * (int64_t)v);
    return 0;
}

// V0 - V1: keys [H][W].  Every face walks its own box alone: the plane is a minimum and does not depend on who tests a pixel.
int msh_visibility(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const float *w2c, const float *k4, int W, int H,
                   float near_z, int split, uint64_t *keys) {
    if (W <= 0 || H <= 0 || !(near_z > 0.f)) return -1;
    const MrPinhole c = mr_pinhole(W, H, k4);
    const size_t n = (size_t)W * H;
    for (size_t o = 0; o < n; ++o) keys[o] = kMshNoKey;
    for (int32_t f = 0; f < F && V > 0; ++f) {
        MrFace face;
        mr_face_setup(c, near_z, w2c, vertices, V, faces + 3 * (int64_t)f, split > 0 ? split : kMrSplit, face);
        if (face.kind == kMrNothing) continue;
        mr_walk_box(c, face, near_z, [&](uint32_t o, float z) {
            const uint64_t key = msh_key(z, (uint32_t)f);
            if (key < keys[o]) keys[o] = key;
        });
    }
    return 0;
}

// S: rgb8 [H][W][3] from keys [H samples][W samples]; k4 / near_z / w2c describe the KEY plane.  ints: mode, samples, smooth,
// normal_frame; floats: bg [3], albedo [3], ambient, vmin, vmax.  depth / face / normal: with samples == 1, or NULL.
int msh_shade(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const float *colors, const float *normals, const float *w2c,
              const float *k4, int W, int H, float near_z, const uint64_t *keys, const int32_t *ints, const float *floats, const uint8_t *lut,
              uint8_t *rgb8, float *depth, int32_t *face, float *normal) {
    MshShade a;
    a.mode = ints[0]; a.samples = ints[1]; a.smooth = ints[2]; a.normal_frame = ints[3];
    for (int k = 0; k < 3; ++k) { a.bg[k] = floats[k]; a.albedo[k] = floats[3 + k]; }
    a.ambient = floats[6]; a.vmin = floats[7]; a.vmax = floats[8];
    a.lut = lut;
    if (W <= 0 || H <= 0 || a.samples < 1 || a.samples > kMshMaxSamples || a.mode < kMshColor || a.mode > kMshDepth) return -1;
    if ((a.mode == kMshDepth && !lut) || (a.samples > 1 && (depth || face || normal))) return -1;
    const MrPinhole c = mr_pinhole(W * a.samples, H * a.samples, k4);
    if (V <= 0) F = 0;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)j * W + i;
            MshSample last;
            msh_pixel(c, near_z, w2c, vertices, V, faces, F, colors, normals, a, keys, i, j, rgb8 + 3 * p, last);
            if (depth) depth[p] = last.z;
            if (face) face[p] = last.face;
            if (normal) { normal[3 * p] = last.n[0]; normal[3 * p + 1] = last.n[1]; normal[3 * p + 2] = last.n[2]; }
        }
    return 0;
}

// view_math.h's view_pixel_bytes in depth mode over a plane of n depths, and view_byte of n values: what S is held to
void msh_view_depth_bytes(const float *depth, long long n, float vmin, float vmax, const uint8_t *lut, uint8_t *rgb8) {
    ViewFinish f = {};
    f.mode = 1;
    f.vmin = vmin; f.vmax = vmax;
    f.lut = lut;
    const float none[3] = {0.f, 0.f, 0.f};
    for (long long p = 0; p < n; ++p) view_pixel_bytes(f, none, depth[p], 0.f, rgb8 + 3 * p);
}
void msh_view_bytes(const float *values, long long n, uint8_t *bytes) {
    for (long long p = 0; p < n; ++p) bytes[p] = view_byte(view_clamp01(values[p]));
}

// one barycentric evaluation, for the S == 0 test: l [3] of the face idx [3] at pixel (i, j)
int msh_barycentrics_at(const float *vertices, int32_t V, const int32_t *idx, const float *w2c, const float *k4, int W, int H, float near_z, int i,
                        int j, float *l) {
    const MrPinhole c = mr_pinhole(W, H, k4);
    MrFace g;
    mr_face_setup(c, near_z, w2c, vertices, V, idx, kMrSplit, g);
    if (g.kind == kMrNothing) return 1;
    msh_barycentrics(g, mr_ray_x(c, i), mr_ray_y(c, j), l);
    return 0;
}

}

#ifdef MESHSHADE_SHIM_MAIN
// The same functions as a stand-alone host program for a build with -fsanitize=address,undefined (tests/test_meshshade_cpu.py): inputs
// chosen to reach every early exit and every index the loops form.  Buffers are exactly as large as documented, so a read or write
// outside them is a report; a wrong answer is a non-zero exit.
#include <stdio.h>
#include <vector>

static int fail(const char *what) {
    printf("FAILED: %s\n", what);
    return 1;
}

int main() {
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const int W = 11, H = 7;
    // a square in front of the camera, then: an out-of-range face, a negative index, a NaN vertex, a repeated index, a triangle
    // wholly behind, one with an infinite vertex, one with vertices 1e20 apart (a component beyond 2^22 m^2)
    std::vector<float> v = {-1, -1, 2, 1, -1, 2, 1, 1, 2, -1, 1, 2, NAN, 0, 1, 0, 0, -5, 1, 0, -5, 0, 1, -6, INFINITY, 0, 1, 1e20f, 0, -3, 0, 1e20f, -3, 5, 5, 5};
    const int32_t V = (int32_t)(v.size() / 3);
    std::vector<int32_t> f = {0, 1, 2, 0, 2, 3, 0, 1, V, -1, 1, 2, 0, 1, 4, 2, 2, 1, 5, 6, 7, 0, 1, 8, 5, 9, 10};
    const int32_t F = (int32_t)(f.size() / 3);
    std::vector<int64_t> accum((size_t)3 * V);
    std::vector<float> normals((size_t)3 * V), colors((size_t)3 * V);
    for (size_t k = 0; k < colors.size(); ++k) colors[k] = (float)(k % 7) / 6.f;
    if (msh_vertex_normals(v.data(), V, f.data(), F, accum.data(), normals.data()) != 0) return fail("normals");
    for (int k = 0; k < 4; ++k)
        if (normals[3 * k] != 0.f || normals[3 * k + 1] != 0.f || normals[3 * k + 2] != 1.f) return fail("the square's normals are not exactly +z");
    if (normals[3 * 11] != 0.f || normals[3 * 4 + 2] != 0.f || normals[3 * 9] != 0.f) return fail("a vertex no accepted face names has a normal");
    if (msh_vertex_normals(nullptr, 0, f.data(), F, nullptr, nullptr) != 0) return fail("no vertices");
    std::vector<uint8_t> lut(768);
    for (int k = 0; k < 768; ++k) lut[k] = (uint8_t)(k / 3);
    for (int s = 1; s <= kMshMaxSamples; ++s) {
        const float k4[4] = {6.f * s, 6.5f * s, (5.1f + 0.5f) * s - 0.5f, (3.3f + 0.5f) * s - 0.5f};
        std::vector<uint64_t> keys((size_t)W * s * H * s);
        for (int split : {0, 1, 1 << 30})
            if (msh_visibility(v.data(), V, f.data(), F, eye, k4, W * s, H * s, 0.01f, split, keys.data()) != 0) return fail("visibility");
        if ((uint32_t)(keys[((size_t)(H * s) / 2) * W * s + (W * s) / 2] >> 32) != 0x40000000u) return fail("the square's depth");
        for (uint64_t key : keys)
            if (key != kMshNoKey && (uint32_t)key >= 2u) return fail("a face that must render nothing won a pixel");
        keys[0] = ((uint64_t)0x40000000u << 32) | (uint32_t)F;          // an id past the faces, ids of the faces that render nothing
        for (int32_t k = 2; k < F && k < (int32_t)keys.size(); ++k) keys[k] = ((uint64_t)0x40000000u << 32) | (uint32_t)k;
        std::vector<uint8_t> rgb((size_t)W * H * 3);
        std::vector<float> depth((size_t)W * H), normal((size_t)W * H * 3);
        std::vector<int32_t> face((size_t)W * H);
        for (int mode = kMshColor; mode <= kMshDepth; ++mode)
            for (int variant = 0; variant < 4; ++variant) {
                const int32_t ints[4] = {mode, s, variant & 1, variant >> 1};
                const float floats[9] = {1.f, 0.5f, 0.25f, 0.8f, 0.8f, 0.8f, 0.25f, 0.f, 6.f};
                const bool planes = s == 1;
                if (msh_shade(v.data(), V, f.data(), F, variant & 2 ? colors.data() : nullptr, variant & 1 ? normals.data() : nullptr, eye, k4, W, H,
                              0.01f, keys.data(), ints, floats, lut.data(), rgb.data(), planes ? depth.data() : nullptr,
                              planes ? face.data() : nullptr, planes ? normal.data() : nullptr) != 0)
                    return fail("shade");
                if (planes && (face[0] != -1 || depth[0] != 0.f)) return fail("an id past the faces is not background");
                if (rgb[3 * ((size_t)W * H - 1)] != 255 || rgb[3 * ((size_t)W * H - 1) + 1] != 128) return fail("the background's bytes");
            }
        const int32_t ints[4] = {kMshShaded, s, 1, 0};
        const float floats[9] = {1.f, 1.f, 1.f, 0.8f, 0.8f, 0.8f, 0.25f, 0.f, 6.f};
        if (msh_shade(nullptr, 0, nullptr, 0, nullptr, nullptr, eye, k4, W, H, 0.01f, keys.data(), ints, floats, nullptr, rgb.data(), nullptr, nullptr,
                      nullptr) != 0)
            return fail("an empty mesh");
        for (uint8_t b : rgb)
            if (b != 255) return fail("an empty mesh is not a picture of the background");
    }
    printf("meshshade host check: clean (%d faces)\n", F);
    return 0;
}
#endif
