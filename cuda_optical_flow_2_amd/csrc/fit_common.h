// LATTICE, USABLE and SAMPLER of "camera motion from point matches" (include/ofx.h), shared by fit_motion.hip and
// fit_homography.hip, with the ranges of their arguments and the wave reductions both use.
//   Item  a kernel's per-item record with p, q (float2), status (int32 or null), pair, w and h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kFitMaxMatches = 1 << 20, kFitMaxSize = 1 << 16, kFitMaxHyp = 4096, kFitMaxThr = 1 << 15, kFitMaxRefits = 3;

// USABLE and LATTICE: the centred lattice values of match i, 0 for a match that is not usable
template <class Item> __device__ __forceinline__ bool load_match(const Item &it, int i, int &ux, int &uy, int &vx, int &vy)
{
    const float2 p = it.p[i], q = it.q[i];
    const float xm = (float)(it.w - 1), ym = (float)(it.h - 1);
    bool ok = p.x >= 0.0f && p.x <= xm && p.y >= 0.0f && p.y <= ym && q.x >= 0.0f && q.x <= xm && q.y >= 0.0f && q.y <= ym; // (false for NaN, inf)
    if (it.status) {
        const int s = it.status[i];
        ok = ok && (s == 0 || (s >> 8) > it.pair);
    }
    const int ox = 16 * (it.w - 1), oy = 16 * (it.h - 1);
    ux = ok ? (int)lrintf(ldexpf(p.x, 5)) - ox : 0;
    uy = ok ? (int)lrintf(ldexpf(p.y, 5)) - oy : 0;
    vx = ok ? (int)lrintf(ldexpf(q.x, 5)) - ox : 0;
    vy = ok ? (int)lrintf(ldexpf(q.y, 5)) - oy : 0;
    return ok;
}

__device__ __forceinline__ unsigned mix(unsigned seed, unsigned j, unsigned k, unsigned a)
{
    unsigned h = seed ^ (j * 0x9E3779B1u) ^ (k * 0x85EBCA77u) ^ (a * 0xC2B2AE3Du);
    h ^= h >> 16, h *= 0x7FEB352Du, h ^= h >> 15, h *= 0x846CA68Bu, h ^= h >> 16;
    return h;
}

__device__ __forceinline__ long long wave_sum64(long long v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, s, 64);
        v = o > v ? o : v;
    }
    return v;
}
