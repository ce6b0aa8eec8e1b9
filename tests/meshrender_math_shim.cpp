// Host build of splatam_amd/csrc/meshrender_math.h for tests/test_meshrender_cpu.py (and, as the bit-exact reference of R1 and S, for
// tests/test_gpu_meshrender.py): plain-loop models of the kernels of csrc/meshrender.hip that call nothing but the header's functions.
// Built with -ffp-contract=off: every float32 step of the header is then one operation, as on the device.
#include <string.h>

#include "../splatam_amd/csrc/meshrender_math.h"

using namespace splat;

extern "C" {

int mr_default_split(void) { return kMrSplit; }

// R0 - R2: depth [H][W] (0 = no hit); kinds [F] (or NULL): what the setup made of every face; tested (or NULL): pixel tests made.
// Every face walks its own box alone -- the plane is a minimum and does not depend on who tests a pixel.
int mr_render(const float *vertices, int32_t V, const int32_t *faces, int32_t F, const float *w2c, const float *k4, int W, int H, float near_z,
              int split, float *depth, int32_t *kinds, long long *tested) {
    if (W <= 0 || H <= 0 || !(near_z > 0.f)) return -1;
    const MrPinhole c = mr_pinhole(W, H, k4);
    const size_t n = (size_t)W * H;
    for (size_t o = 0; o < n; ++o) depth[o] = INFINITY;
    long long tests = 0;
    for (int32_t f = 0; f < F; ++f) {
        MrFace face;
        mr_face_setup(c, near_z, w2c, vertices, V, faces + 3 * (int64_t)f, split > 0 ? split : kMrSplit, face);
        if (kinds) kinds[f] = face.kind;
        if (face.kind == kMrNothing) continue;
        tests += mr_walk_box(c, face, near_z, [&](uint32_t o, float z) {
            if (z < depth[o]) depth[o] = z;
        });
    }
    for (size_t o = 0; o < n; ++o)
        if (depth[o] == INFINITY) depth[o] = 0.f;
    if (tested) *tested = tests;
    return 0;
}

// S: seen [V] is incremented
int mr_seen_counts(const float *vertices, int32_t V, const float *w2c, int32_t n, const float *k4, int W, int H, int edge, const float *depth,
                   float eps, int32_t *seen) {
    if (W <= 0 || H <= 0 || edge < 0 || n < 0) return -1;
    const MrPinhole c = mr_pinhole(W, H, k4);
    for (int32_t v = 0; v < V; ++v) {
        int32_t count = 0;
        for (int32_t k = 0; k < n; ++k)
            count += mr_seen(c, w2c + 16 * (size_t)k, vertices + 3 * (size_t)v, edge, depth ? depth + (size_t)W * H * k : nullptr, eps) ? 1 : 0;
        seen[v] += count;
    }
    return 0;
}

}

#ifdef MESHRENDER_SHIM_MAIN
// The same functions as a stand-alone host program for a build with -fsanitize=address,undefined (tests/test_meshrender_cpu.py): inputs
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
    const float k4[4] = {20.f, 21.f, 15.3f, 10.7f};
    const int W = 33, H = 21;
    // a square in front of the camera, then: an out-of-range face, a negative index, a NaN vertex, a triangle through the camera centre,
    // a triangle crossing z = 0, one wholly behind, one with an infinite vertex
    std::vector<float> v = {-1, -1, 2, 1, -1, 2, 1, 1, 2, -1, 1, 2, NAN, 0, 1, -1, -1, -1, 1, 1, 1, 0, 1, 0,
                            0, 0, -3, 0.5f, 0, 3, 0, 0.5f, 3, 0, 0, -5, 1, 0, -5, 0, 1, -6, INFINITY, 0, 1};
    const int32_t V = (int32_t)(v.size() / 3);
    std::vector<int32_t> f = {0, 1, 2, 0, 2, 3, 0, 1, V, -1, 1, 2, 0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 0, 1, 14, 2, 2, 2};
    const int32_t F = (int32_t)(f.size() / 3);
    std::vector<float> depth((size_t)W * H);
    std::vector<int32_t> kinds(F);
    long long tested = 0;
    for (int split : {0, 1, 1 << 30}) {
        if (mr_render(v.data(), V, f.data(), F, eye, k4, W, H, 0.01f, split, depth.data(), kinds.data(), &tested) != 0) return fail("render");
        if (kinds[2] != kMrNothing || kinds[3] != kMrNothing || kinds[4] != kMrNothing || kinds[7] != kMrNothing || kinds[8] != kMrNothing)
            return fail("a face that must render nothing was set up");
        if (kinds[5] == kMrSmall || kinds[6] != kMrLarge) return fail("a face with a vertex at z <= near is walked by the wave, or lies outside the image");
        if (depth[(size_t)10 * W + 15] != 2.f) return fail("the square's depth");
        for (float z : depth)
            if (!(z == 0.f || (z >= 0.01f && z < INFINITY))) return fail("a depth that is neither a hole nor a hit");
    }
    // a 1 x 1 image, and a mesh without vertices or faces
    float one = -1.f;
    if (mr_render(v.data(), V, f.data(), F, eye, k4, 1, 1, 0.01f, 0, &one, nullptr, nullptr) != 0 || !(one >= 0.f)) return fail("1 x 1");
    if (mr_render(nullptr, 0, f.data(), F, eye, k4, 1, 1, 0.01f, 0, &one, kinds.data(), nullptr) != 0 || one != 0.f) return fail("no vertices");
    if (mr_render(v.data(), V, nullptr, 0, eye, k4, W, H, 0.01f, 0, depth.data(), nullptr, nullptr) != 0 || depth[0] != 0.f) return fail("no faces");
    // seen: zero views, two views with and without planes, a margin wider than the image
    std::vector<int32_t> seen(V, 7);
    if (mr_seen_counts(v.data(), V, nullptr, 0, k4, W, H, 0, nullptr, 0.f, seen.data()) != 0) return fail("zero views");
    for (int32_t s : seen)
        if (s != 7) return fail("zero views changed a count");
    std::vector<float> poses(32);
    for (int k = 0; k < 32; ++k) poses[k] = eye[k % 16];
    poses[16 + 11] = 1.f;                                                // the second camera one metre back
    std::vector<float> planes((size_t)2 * W * H);
    for (int k = 0; k < 2; ++k)
        if (mr_render(v.data(), V, f.data(), 2, poses.data() + 16 * k, k4, W, H, 0.01f, 0, planes.data() + (size_t)k * W * H, nullptr, nullptr) != 0)
            return fail("planes");
    std::fill(seen.begin(), seen.end(), 0);
    if (mr_seen_counts(v.data(), V, poses.data(), 2, k4, W, H, 0, planes.data(), 0.03f, seen.data()) != 0) return fail("seen");
    if (seen[0] != 1 || seen[4] != 0 || seen[14] != 0) return fail("seen counts (corner: outside the first image, inside the second)");
    if (mr_seen_counts(v.data(), V, poses.data(), 2, k4, W, H, 40, nullptr, 0.f, seen.data()) != 0 || seen[0] != 1) return fail("a margin wider than the image");
    printf("meshrender host check: clean (%d faces, %lld pixel tests in the last render)\n", F, tested);
    return 0;
}
#endif
