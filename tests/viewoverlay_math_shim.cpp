// Host build of splatam_amd/csrc/viewoverlay_math.h for tests/test_viewoverlay_cpu.py and tests/test_gpu_view_overlay.py: plain-loop
// models of the four kernels of csrc/viewoverlay.hip that call nothing but the header's per-lane functions (an atomic minimum is a
// minimum here), so that the overlay is checked against the float64 restatement (tests/viewoverlay_ref.py) without a GPU and the
// kernels against these loops bit for bit.  Built with -ffp-contract=off.  With -DVIEWOVERLAY_SHIM_MAIN it is a stand-alone program
// that drives the same loops over hostile inputs, for the sanitizers.
#include "../splatam_amd/csrc/viewoverlay_math.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace splat;

extern "C" {

void vo_shim_cool(double x, uint8_t *rgb) { vo_cool(x, rgb); }

// frames [first, first + count) of a run into segments / colors (the block's layout); rots / trans NULL with w2c_all given
void vo_shim_run(int num_frames, int first, int count, const float *w2c_all, const float *rots, const float *trans, const float *first_w2c, int w,
                 int h, double fx, double fy, double cx, double cy, double scale, int frusta, const uint8_t *fixed, float *segments,
                 uint8_t *colors) {
    VoRun r;
    r.num_frames = num_frames;
    r.w2c_all = w2c_all; r.cam_unnorm_rots = rots; r.cam_trans = trans; r.first_w2c = first_w2c;
    r.w = w; r.h = h; r.fx = fx; r.fy = fy; r.cx = cx; r.cy = cy; r.scale = scale;
    r.frusta = frusta; r.fixed = fixed != nullptr;
    for (int k = 0; k < 3; ++k) r.color[k] = fixed ? fixed[k] : 0;
    for (int t = first; t < first + count; ++t) vo_run_frame(r, t, segments, colors);
}

void vo_shim_clear(uint64_t *keys, long long n) {
    for (long long i = 0; i < n; ++i) keys[i] = kMshNoKey;
}

static void put(uint64_t *keys, uint32_t o, float z, uint32_t id) {
    const uint64_t k = msh_key(z, id);
    if (k < keys[o]) keys[o] = k;
}

void vo_shim_points(int W, int H, const float *k4, float near_z, const float *w2c, const float *means3D, int count, int size, uint64_t *keys) {
    const MrPinhole c = mr_pinhole(W, H, k4);
    for (int row = 0; row < count; ++row) {
        const VoBox b = vo_point(c, near_z, w2c, means3D + 3 * (size_t)row, size);
        for (int j = b.j0; j <= b.j1; ++j)
            for (int i = b.i0; i <= b.i1; ++i) put(keys, (uint32_t)j * (uint32_t)W + (uint32_t)i, b.z, (uint32_t)row);
    }
}

// returns the largest step count met
int vo_shim_segments(int W, int H, const float *k4, float near_z, const float *w2c, const float *segments, int first, int count, int width,
                     uint64_t *keys) {
    const MrPinhole c = mr_pinhole(W, H, k4);
    int most = 0;
    for (int s = first; s < first + count; ++s) {
        const VoLine L = vo_line(c, near_z, w2c, segments + 6 * (size_t)s);
        if (L.steps > most) most = L.steps;
        const uint32_t id = kVoSegmentBit | (uint32_t)s;
        for (int k = 0; k < L.steps; ++k) vo_line_stamp(c, L, k, width, [=](uint32_t at, float z) { put(keys, at, z, id); });
    }
    return most;
}

// the centre line of ONE segment: ij [capacity][2], z [capacity]; returns the step count (steps beyond capacity are not written)
int vo_shim_walk(int W, int H, const float *k4, float near_z, const float *w2c, const float *seg, int capacity, int32_t *ij, float *z) {
    const MrPinhole c = mr_pinhole(W, H, k4);
    const VoLine L = vo_line(c, near_z, w2c, seg);
    for (int k = 0; k < L.steps && k < capacity; ++k) {
        int i, j;
        vo_line_step(L, k, i, j, z[k]);
        ij[2 * k] = i; ij[2 * k + 1] = j;
    }
    return L.steps;
}

void vo_shim_finish(int W, int H, const uint64_t *keys, const float *depth, int occlude, int fill, const float *rgb_colors, int rows,
                    const uint8_t *segment_colors, int segments, const float *bg, uint8_t *rgb8) {
    VoResolve r;
    r.occlude = occlude; r.rgb_colors = rgb_colors; r.rows = rows; r.segment_colors = segment_colors; r.segments = segments;
    for (long long p = 0; p < (long long)W * H; ++p) {
        uint8_t out[3];
        for (int k = 0; k < 3; ++k) out[k] = view_byte(view_clamp01(bg[k]));
        const float d = depth && keys[p] != kMshNoKey ? depth[p] : 0.f;
        if (!vo_resolve(r, keys[p], d, out) && !fill) continue;
        for (int k = 0; k < 3; ++k) rgb8[3 * p + k] = out[k];
    }
}

}

#ifdef VIEWOVERLAY_SHIM_MAIN
// Hostile inputs through every loop above; heap buffers of the exact sizes, so that any store or load outside them is a report.
static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const float nan = nanf(""), inf = INFINITY, big = 3.0e38f;
    const float w2cs[2][16] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1},
                               {0.8f, 0, 0.6f, 0.3f, 0, 1, 0, -0.2f, -0.6f, 0, 0.8f, 0.5f, 0, 0, 0, 1}};
    const float segs[][6] = {
        {-1, -0.5f, 2, 1, 0.5f, 2},    {-1, -1, 1, 1, 1, 3},          {0.1f, -2, 2, 0.12f, 2, 2.5f},  {-3, 0.2f, 4, 3, 0.25f, 1},
        {0, 0, -1, 0.5f, 0.2f, 3},     {0, 0, -1, 1, 1, -2},          {50, 50, 1, 60, 60, 1},         {-5, -5, 2, 5, 5, 2},
        {0.2f, 0.1f, 2, 0.2f, 0.1f, 2}, {nan, 0, 1, 0, 0, 1},          {0, 0, 1, inf, 0, 1},           {0, 0, 1, 0, -inf, 2},
        {big, big, big, -big, -big, big}, {big, 0, 1e-30f, -big, 0, 1e-30f}, {0, 0, 0.01f, 0, 0, 0.01f},  {0, 0, 0, 0, 0, 0},
        {-1e6f, 3, 1e-3f, 1e6f, -3, 1e3f}, {0, 0, 1, 0, 0, nan},
    };
    const int nsegs = (int)(sizeof(segs) / sizeof(segs[0]));
    const float pts[][3] = {{0, 0, 2}, {0.5f, 0.3f, 1}, {-10, 0, 1}, {0, 0, -1}, {nan, 0, 1}, {0, inf, 1}, {0, 0, inf}, {big, big, big},
                            {0, 0, 0.01f}, {-0.6f, -0.3f, 1}, {0, 0, 1e-30f}, {1e30f, 0, 1e-30f}};
    const int npts = (int)(sizeof(pts) / sizeof(pts[0]));
    const int sizes[4][2] = {{72, 40}, {70, 37}, {16, 16}, {1, 1}};
    for (int si = 0; si < 4; ++si) {
        const int W = sizes[si][0], H = sizes[si][1], limit = (W > H ? W : H) + 1;
        const float k4[4] = {0.8f * W, 0.8f * W + 1.5f, W / 2.f - 0.5f, H / 2.f - 0.25f};
        for (int wi = 0; wi < 2; ++wi) {
            std::vector<uint64_t> keys((size_t)W * H);
            std::vector<float> seg(segs[0], segs[0] + 6 * nsegs), mean(pts[0], pts[0] + 3 * npts);
            for (int width = 1; width <= kVoMaxLineWidth; ++width) {
                vo_shim_clear(keys.data(), (long long)W * H);
                EXPECT(vo_shim_segments(W, H, k4, 0.01f, w2cs[wi], seg.data(), 0, nsegs, width, keys.data()) <= limit);
            }
            for (int s = 0; s < nsegs; ++s) {
                std::vector<int32_t> ij(2 * (size_t)limit);
                std::vector<float> z((size_t)limit);
                const int n = vo_shim_walk(W, H, k4, 0.01f, w2cs[wi], seg.data() + 6 * s, limit, ij.data(), z.data());
                EXPECT(n >= 0 && n <= limit);
                for (int k = 1; k < n; ++k) EXPECT(abs(ij[2 * k] - ij[2 * k - 2]) <= 1 && abs(ij[2 * k + 1] - ij[2 * k - 1]) <= 1);
            }
            for (int size = 1; size <= kVoMaxPointSize; ++size)
                vo_shim_points(W, H, k4, 0.01f, w2cs[wi], mean.data(), npts, size, keys.data());
            // keys that name rows and segments past the end, colours out of range
            std::vector<float> colours = {0.5f, -1.f, 2.f, nan, inf, -inf}, depth((size_t)W * H, 1.5f);
            std::vector<uint8_t> seg_colours(3 * (size_t)nsegs, 9), rgb8(3 * (size_t)W * H, 1);
            const float bg[3] = {nan, 2.f, 0.25f};
            keys[0] = msh_key(1.f, 5);
            if (W * H > 1) keys[1] = msh_key(1.f, kVoSegmentBit | 1000u);
            for (int occlude = 0; occlude < 2; ++occlude)
                for (int fill = 0; fill < 2; ++fill) {
                    vo_shim_finish(W, H, keys.data(), depth.data(), occlude, fill, colours.data(), 2, seg_colours.data(), nsegs, bg, rgb8.data());
                    vo_shim_finish(W, H, keys.data(), nullptr, occlude, fill, nullptr, 0, nullptr, 0, bg, rgb8.data());
                }
        }
    }
    // a run: pose parameters (a zero quaternion among them), explicit matrices, one frame, ranges
    const int n = 5;
    std::vector<float> rots(4 * n), trans(3 * n), mats(16 * n), segments(6 * (size_t)(9 * n - 1)), first(w2cs[1], w2cs[1] + 16);
    std::vector<uint8_t> colours(3 * (size_t)(9 * n - 1));
    for (int t = 0; t < n; ++t) {
        for (int k = 0; k < 4; ++k) rots[k * n + t] = t == 2 ? 0.f : 0.3f * (k + 1) - 0.1f * t;
        for (int k = 0; k < 3; ++k) trans[k * n + t] = 0.2f * t - 0.1f * k;
        memcpy(&mats[16 * t], w2cs[t % 2], sizeof(w2cs[0]));
    }
    const uint8_t fixed[3] = {255, 255, 0};
    vo_shim_run(n, 0, n, nullptr, rots.data(), trans.data(), first.data(), 72, 40, 60, 58, 35.5, 19.25, 0.045, 1, nullptr, segments.data(), colours.data());
    vo_shim_run(n, 2, 2, mats.data(), nullptr, nullptr, nullptr, 72, 40, 60, 58, 35.5, 19.25, 0.045, 1, fixed, segments.data(), colours.data());
    std::vector<float> line(6 * (size_t)(n - 1));
    std::vector<uint8_t> line_colours(3 * (size_t)(n - 1));
    vo_shim_run(n, 0, n, mats.data(), nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, fixed, line.data(), line_colours.data());
    std::vector<float> one(6 * 8);
    std::vector<uint8_t> one_colours(3 * 8);
    vo_shim_run(1, 0, 1, mats.data(), nullptr, nullptr, nullptr, 72, 40, 60, 58, 35.5, 19.25, 0.045, 1, nullptr, one.data(), one_colours.data());
    uint8_t c[3];
    const double xs[] = {-1.0, 0.0, 0.5, 1.0, 2.0, 1e300, (double)nan, (double)inf, -(double)inf};
    for (double x : xs) {
        vo_shim_cool(x, c);
        EXPECT(c[2] == 255);
    }
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
#endif
