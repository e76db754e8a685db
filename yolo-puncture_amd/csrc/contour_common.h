// __device__ helpers shared by the two contour paths (contour.hip: bit image in LDS; contour_large.hip: bit image in a workspace).
#pragma once
#include "common.h"

namespace yp {

// hostops.scale_coords((H,W) -> (H0,W0)) of one polygon coordinate as numpy evaluates it on an int32 polygon, then the int32 truncation of
// get_coord_min_rect_len: float32 (v - pad) / gain (gain and pad computed in double and rounded to float32 on the host), clipped to
// [0, hi]. Correctly rounded fp32 division; nothing is contracted.
__device__ __forceinline__ int scale_coord(int v, float pad, float gain, int hi) {
#pragma clang fp contract(off)
    const float d = (float)v - pad;
    const float s = d / gain;
    return (int)fminf(fmaxf(s, 0.f), (float)hi);
}

// clockwise from east, as hostops._DIRS: (dy,dx)
// (dy, dx) = {0,1,1,1,0,-1,-1,-1}, {1,1,0,-1,-1,-1,0,1}, each + 1 in two bits per direction: decoded in registers - a `__constant__` table indexed
// per lane is a vector memory load, two of them on the serial path of every trace step (measured: 643 -> see DESIGN us per 720p mask)
__device__ __forceinline__ int c_dy(int d) { return (int)((0x01a9u >> (2 * d)) & 3u) - 1; }
__device__ __forceinline__ int c_dx(int d) { return (int)((0x901au >> (2 * d)) & 3u) - 1; }

// A bit image with one zero word left of every row, two right of it and one zero row above and below: row y of the image lives at stored
// row y + 1, column x at bit x + 32 of the row.
struct Bitmap {
    const unsigned* w;   // LDS (contour.hip) or the workspace (contour_large.hip)
    int pitch;           // words per row
    // 8-neighbour ring of the pixel in column x whose row ABOVE starts at word `rb`: bits E, SE, S, SW, W, NW, N, NE. Three 64-bit
    // windows, one shift each; the row below arrives mirrored through a packed 3-bit reversal table.
    __device__ __forceinline__ unsigned ring(int rb, int x) const {
        const int pos = x + 31;                              // bit position of x-1
        const unsigned* r0 = w + rb + (pos >> 5);
        const int sh = pos & 31;
        const unsigned long long u = ((unsigned long long)r0[1] << 32) | r0[0];
        const unsigned long long m = ((unsigned long long)r0[pitch + 1] << 32) | r0[pitch];
        const unsigned long long d = ((unsigned long long)r0[2 * pitch + 1] << 32) | r0[2 * pitch];
        const unsigned uu = (unsigned)(u >> sh) & 7u, mm = (unsigned)(m >> sh) & 7u, dd = (unsigned)(d >> sh) & 7u;
        return (mm >> 2) | ((0x73516240u >> (4 * dd)) & 7u) << 1 | (mm & 1u) << 4 | uu << 5;
    }
};

}  // namespace yp
