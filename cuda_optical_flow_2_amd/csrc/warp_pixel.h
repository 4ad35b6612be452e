// The part of a frame warp that follows the position (IN RANGE, BORDER and VALUE of "affine frame warp" in include/ofx.h), shared by
// warp_affine.hip and warp_persp.hip: a lane's four adjacent output pixels of a row from their source positions on the 1/32 px
// lattice -- the geometry of a pixel once for all its channels, every tap clamped before it becomes an address -- stored as dwords
// where the address allows and the quad is whole, as bytes otherwise.
//   Item  a kernel's per-item record with src, src_pitch, sw, sh, dst, dst_pitch, w, border and fill;
//   Pos   bool pos(k, qx, qy): the position of pixel x0 + k, called for k = 0 .. 3 in order; false for a pixel that has none, which
//         gets `fill` under either border mode.
// Returns how many of the quad's pixels inside the row are out of range or have no position.
#pragma once

#include <stdint.h>

#include "ofx.h"

constexpr int kWarpQuad = 4;

template <int C, class Item, class Pos> __device__ __forceinline__ unsigned warp_quad_at(const Item &it, int y, int x0, Pos pos)
{
    const int xmax = 32 * (it.sw - 1), ymax = 32 * (it.sh - 1);
    const bool constant = it.border == OFX_BORDER_CONSTANT;
    unsigned out = 0;
    uint8_t v[kWarpQuad][C];
#pragma unroll
    for (int k = 0; k < kWarpQuad; ++k) {
        long long qx, qy;
        const bool defined = pos(k, qx, qy);
        const bool in = defined && qx >= 0 && qx <= xmax && qy >= 0 && qy <= ymax;
        out += (x0 + k < it.w && !in) ? 1u : 0u;
        const int cx = (int)(qx < 0 ? 0 : qx > xmax ? xmax : qx), cy = (int)(qy < 0 ? 0 : qy > ymax ? ymax : qy); // (clamped: in 0 .. 32 (size - 1))
        const int ix = cx >> 5, fa = cx & 31, iy = cy >> 5, fb = cy & 31;
        const int ix1 = ix + 1 < it.sw ? ix + 1 : it.sw - 1, iy1 = iy + 1 < it.sh ? iy + 1 : it.sh - 1;
        const uint8_t *r0 = it.src + (size_t)iy * (size_t)it.src_pitch, *r1 = it.src + (size_t)iy1 * (size_t)it.src_pitch;
        const int w00 = (32 - fa) * (32 - fb), w10 = fa * (32 - fb), w01 = (32 - fa) * fb, w11 = fa * fb;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const int s = w00 * r0[C * ix + ch] + w10 * r0[C * ix1 + ch] + w01 * r1[C * ix + ch] + w11 * r1[C * ix1 + ch];
            v[k][ch] = ((constant && !in) || !defined) ? (uint8_t)it.fill : (uint8_t)((s + 512) >> 10);
        }
    }
    uint8_t *d = it.dst + (size_t)y * (size_t)it.dst_pitch + (size_t)(C * x0);
    if (x0 + kWarpQuad <= it.w && ((uintptr_t)d & 3) == 0) {
        const uint8_t *b = &v[0][0];
#pragma unroll
        for (int k = 0; k < C; ++k)
            reinterpret_cast<uint32_t *>(d)[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < kWarpQuad; ++k)
            if (x0 + k < it.w) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) d[C * k + ch] = v[k][ch];
            }
    }
    return out;
}
