// mesh_device.h -- what the kernels that work on a finished triangle mesh share, one definition each, so that "bit for bit
// mesh_render.render_depth's plane" is held by the source and not by two copies kept in step: the raster walk of the depth plane
// (meshrender.hip R1) and of the key plane (meshshade.hip V1), and the camera of a SplatMeshView.  The arithmetic per face and pixel is meshrender_math.h's.  What differs stays in its
// file: what a hit does to its plane.
#pragma once

#include "splat_device.h"
#include "meshrender_math.h"

namespace splat {

inline MrPinhole pinhole_of(const SplatMeshView &v) {
    const float k4[4] = {v.fx, v.fy, v.cx, v.cy};
    return mr_pinhole(v.width, v.height, k4);
}

#if defined(__HIPCC__)

// ---------------------------------------------------------------------------------------------------------------- the raster walk
// One lane per triangle sets it up (camera-space vertices, the three edge planes, the normal, the box).  A lane whose box holds at
// most `split` pixels walks it alone (mr_walk_box).  The others are taken one after the other by the whole WAVE: the owner's lane
// broadcasts the 13 floats and the box, and lane l tests pixels l, l + 64, ... of the box, so no lane's loop is proportional to a
// large triangle's pixel count while 63 idle.  Large faces are found by a ballot, not a list: nothing is deferred, nothing can
// overflow.  put(offset, z, face) receives every hit with the index of the face that made it: the lane's own in the one-lane
// branch, the owner's in the wave's.
//
// EVERY lane of the wave must reach the ballot and stay for the broadcasts behind it: the walk is the whole body of a kernel of
// BLOCK threads per workgroup, a lane past the last face sets up nothing (kind 0) and no lane returns early.  Every loop is bounded
// by width x height: the one-lane walk by its box, the wave's by at most width x height / 64 trips (j grows every trip or two).
//
// Faces are [F][3] int32 and vertices [V][3] float32: rows of 12 bytes, which no 16-byte access fits without straddling rows, so a
// lane reads its three indices and nine coordinates as 4-byte loads (consecutive lanes read consecutive rows: the wave's loads of the
// faces are contiguous).  Pixel offsets fit 32 bits: the entry points refuse more than 2^30 - 1 pixels.
template <int BLOCK, typename Put>
__device__ __forceinline__ void mesh_raster_walk(const MrPinhole &cam, float near_z, const float *__restrict__ w2c,
                                                 const float *__restrict__ vertices, int32_t V, const int32_t *__restrict__ faces, int32_t F,
                                                 int split, Put put) {
    const long long f = (long long)blockIdx.x * BLOCK + threadIdx.x;
    float m[12];
    for (int k = 0; k < 12; ++k) m[k] = w2c[k];
    MrFace face = {};                                                   // (kind 0: nothing)
    if (f < F) {
        const int32_t idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        mr_face_setup(cam, near_z, m, vertices, V, idx, split, face);
    }
    if (face.kind == kMrSmall) mr_walk_box(cam, face, near_z, [&](uint32_t o, float z) { put(o, z, (uint32_t)f); });
    unsigned long long large = __ballot(face.kind == kMrLarge);
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t first = (uint32_t)(f - lane);                        // the face of lane 0 of this wave
    while (large) {
        const int src = __ffsll((long long)large) - 1;
        large &= large - 1;
        MrFace g;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) g.e[a][b] = __shfl(face.e[a][b], src, kWave);
        for (int a = 0; a < 3; ++a) g.n[a] = __shfl(face.n[a], src, kWave);
        g.na = __shfl(face.na, src, kWave);
        g.i0 = __shfl(face.i0, src, kWave); g.i1 = __shfl(face.i1, src, kWave);
        g.j0 = __shfl(face.j0, src, kWave); g.j1 = __shfl(face.j1, src, kWave);
        // lane l tests pixels l, l + 64, ... of the box in row order.  Two divisions per FACE (wave-uniform), none per pixel: a step of
        // 64 pixels is `rows` rows and `cols` columns, with one carry when the column leaves the box.
        const int bw = g.i1 - g.i0 + 1;
        const int rows = kWave / bw, cols = kWave % bw;
        int j = g.j0 + lane / bw, i = g.i0 + lane % bw;
        float dy = mr_ray_y(cam, j);
        int row = j;
        while (j <= g.j1) {
            if (j != row) { dy = mr_ray_y(cam, j); row = j; }
            float z;
            if (mr_hit(g, near_z, mr_ray_x(cam, i), dy, z)) put((uint32_t)j * cam.W + i, z, first + (uint32_t)src);
            i += cols;
            j += rows;
            if (i > g.i1) { i -= bw; ++j; }
        }
    }
}

#endif  // __HIPCC__

}  // namespace splat
