// 128-bit two's-complement sums kept as two 64-bit halves (lo, hi), for the degree-3 and degree-4 sums of the homography refit
// ("planar homography from point matches" in include/ofx.h): the add with a carry between the halves, and the conversion to
// float64, to nearest even in ONE rounding.  Plain C++ that compiles for the host and for the device (tests/wide_sum_check.cpp
// runs it on the host).
#pragma once

#include <math.h>
#include <stdint.h>

typedef unsigned long long wide_u64; // (atomicAdd's 64-bit type)

#if defined(__HIPCC__)
#define OFX_WIDE_FN __host__ __device__ __forceinline__
#else
#define OFX_WIDE_FN static inline
#endif

// the carry out of lo when `add` was added to a low half that held `old`: (old + add) mod 2^64 < old
OFX_WIDE_FN wide_u64 wide_carry(wide_u64 old, wide_u64 add) { return (wide_u64)(old + add) < old ? 1u : 0u; }

// (lo, hi) += (alo, ahi) modulo 2^128.  With atomics: old = atomicAdd(&lo, alo), then atomicAdd(&hi, ahi + wide_carry(old, alo)) --
// every add's carry reaches hi exactly once, so the total is exact in any order
OFX_WIDE_FN void wide_add(wide_u64 &lo, wide_u64 &hi, wide_u64 alo, wide_u64 ahi)
{
    const wide_u64 old = lo;
    lo = old + alo;
    hi += ahi + wide_carry(old, alo);
}

// the float64 nearest to the signed 128-bit integer (lo, hi), ties to even: the top 53 bits of the magnitude, incremented when the
// bits below them exceed a half, or equal a half and bit 53 is odd.  Every bit below takes part (a sticky bit), so this is not a
// double rounding through 64 bits.
OFX_WIDE_FN double wide_to_double(wide_u64 lo, wide_u64 hi)
{
    const bool neg = (hi >> 63) != 0;
    if (neg) { // the magnitude: ~v + 1 (2^127 for the most negative value)
        lo = ~lo, hi = ~hi;
        lo += 1;
        hi += lo == 0 ? 1u : 0u;
    }
    const int top = hi ? 127 - __builtin_clzll(hi) : lo ? 63 - __builtin_clzll(lo) : -1; // the highest set bit
    double r;
    if (top <= 52) {
        r = (double)lo; // (exact)
    } else {
        const int shift = top - 52; // 1 .. 75
        wide_u64 mant, rest_hi, rest_lo, half_hi, half_lo;
        if (shift >= 64) {
            mant = hi >> (shift - 64);
            rest_hi = shift == 64 ? 0 : hi & ((1ull << (shift - 64)) - 1), rest_lo = lo;
            half_hi = shift == 64 ? 0 : 1ull << (shift - 65), half_lo = shift == 64 ? 1ull << 63 : 0;
        } else {
            mant = (lo >> shift) | (hi << (64 - shift)); // (hi has at most shift - 11 bits: nothing is lost)
            rest_hi = 0, rest_lo = lo & ((1ull << shift) - 1);
            half_hi = 0, half_lo = 1ull << (shift - 1);
        }
        const bool above = rest_hi > half_hi || (rest_hi == half_hi && rest_lo > half_lo);
        const bool tie = rest_hi == half_hi && rest_lo == half_lo;
        if (above || (tie && (mant & 1))) mant += 1; // (2^53 at most: still exact below)
        r = ldexp((double)mant, shift);
    }
    return neg ? -r : r;
}
