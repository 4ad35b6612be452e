// The composed flow of ONE pixel (main.cu:138-147): what compose_flow_kernel (pyramid.hip) and compose_ring_kernel compute for it,
// bit for bit -- coarsest level first, a float accumulator updated through a double product,
// u = (float)((double)u + 2^s * (double)f) with s = k - level.  2^s * f is exact in double, so the only roundings are the double
// sum and its conversion back to float.
//
// For callers that sample the field at a few positions (sample_ring.hip): the loads of all levels are issued before the first
// accumulation, so a sample costs one memory round trip and not levels - level of them; the accumulation order stays fixed.
#pragma once

#include "ofx_internal.h"

// One pair's flow pyramid as seen from `level`: entry s is level `level + s` (n = levels - level of them; the entries beyond repeat
// the coarsest level, so all of them are valid).  lv[s] points at global row own0[s] of its level, rows tightly packed,
// w >> s float2 wide.  Built from wave-uniform values with constant indices: it lives in scalar registers.
struct ofx_px_pyramid {
    const float2 *lv[OFX_MAX_LEVELS];
    int own0[OFX_MAX_LEVELS];
    int n;
};

// lv[k], own0[k] (k = level .. levels-1) as in ofx_compose_batch
__device__ __forceinline__ ofx_px_pyramid ofx_px_pyramid_of(const float *const *lv, const int *own0, int levels, int level)
{
    ofx_px_pyramid P;
    P.n = levels - level;
#pragma unroll
    for (int s = 0; s < OFX_MAX_LEVELS; ++s) {
        const int k = level + s < levels ? level + s : levels - 1;
        P.lv[s] = reinterpret_cast<const float2 *>(lv[k]);
        P.own0[s] = own0[k];
    }
    return P;
}

// kN = levels - level at compile time: straight-line code, so the kN loads go out back to back and the accumulation waits for them
// with counted waits.  (One body with the loads under `if (s < n)` compiles to a wait after every load: the compiler moves each
// value's conversion to double into the load's block.)  (y, x): a pixel of level `level` (w wide), y counted from own0[0].
template <int kN>
__device__ __forceinline__ float2 ofx_compose_px_n(const ofx_px_pyramid &P, int w, int y, int x)
{
    const int gy = y + P.own0[0];
    float2 f[kN];
#pragma unroll
    for (int s = 0; s < kN; ++s) {
        const size_t row = (size_t)((gy >> s) - P.own0[s]);
        f[s] = P.lv[s][row * (size_t)(w >> s) + (size_t)(x >> s)];
    }
    float u = 0.0f, v = 0.0f;
#pragma unroll
    for (int s = kN - 1; s >= 0; --s) {
        const double m = (double)(1 << s);
        u = (float)((double)u + m * (double)f[s].x);
        v = (float)((double)v + m * (double)f[s].y);
    }
    return make_float2(u, v);
}

__device__ __forceinline__ float2 ofx_compose_px(const ofx_px_pyramid &P, int w, int y, int x)
{
    switch (P.n) {
#define OFX_COMPOSE_CASE(n) \
    case n: return ofx_compose_px_n<n>(P, w, y, x);
        OFX_COMPOSE_CASE(1)
        OFX_COMPOSE_CASE(2)
        OFX_COMPOSE_CASE(3)
        OFX_COMPOSE_CASE(4)
        OFX_COMPOSE_CASE(5)
        OFX_COMPOSE_CASE(6)
        OFX_COMPOSE_CASE(7)
        OFX_COMPOSE_CASE(8)
        OFX_COMPOSE_CASE(9)
        OFX_COMPOSE_CASE(10)
        OFX_COMPOSE_CASE(11)
#undef OFX_COMPOSE_CASE
    default: return ofx_compose_px_n<OFX_MAX_LEVELS>(P, w, y, x);
    }
}
