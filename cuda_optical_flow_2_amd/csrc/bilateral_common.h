// Bilateral filter pieces shared by primitives.hip (ofx_bilateral_3ch / ofx_bilateral_3ch_fast) and frontend.hip (the stream
// pipeline's colour front end): the kernel-argument tables, the host code that fills them, and the tap loops of the bit-exact
// kernel (bilateral_exact_own_kernel) and of the +-1 LSB kernel (bilateral_lut_kernel).  The comments at those kernels in
// primitives.hip describe the arithmetic.  Everything here sits in an unnamed namespace: each translation unit gets its own copy.
#pragma once

#include <math.h>
#include <stdlib.h>

#include "ofx_internal.h"

namespace {

constexpr int kMaxBilateral = 13;
struct BilateralArg {
    double range[256];
    double spatial[kMaxBilateral * kMaxBilateral];
};
constexpr int kBilSentinel = 1023;                 // grey "value" of a pixel outside the image
constexpr int kBilLut = kBilSentinel + 255 + 1;    // entries: index = g - f0 + 255

// bilateral_exact_own_kernel: a block's tile and its threads; the taps of one tile row for a lane's two pixels of one output row
constexpr int kExTileW = 128, kExTileH = 32, kExThreads = 512;

template <int WW>
__device__ __forceinline__ void exact_row_taps(const int (&v)[WW + 1], int baseA, int baseB, const uint8_t *lut_b, const double *ns, double (&acc)[4])
{
#pragma unroll
    for (int n = 0; n < WW; ++n) {
        const double nbA = *reinterpret_cast<const double *>(lut_b + (8 * v[n] + baseA)), nbB = *reinterpret_cast<const double *>(lut_b + (8 * v[n + 1] + baseB));
        const double s = ns[n];
        acc[0] += nbA * s;
        acc[1] += (double)(uint32_t)v[n] * nbA * s;
        acc[2] += nbB * s;
        acc[3] += (double)(uint32_t)v[n + 1] * nbB * s;
    }
}

// bilateral_lut_kernel
constexpr int kLutTileW = 128, kLutTileH = 32, kLutEntries = 512, kLutThreads = 512; // (eight waves share one table and one halo)
constexpr float kLutOutside = -1024.0f; // 4 * -256
struct BilateralLutArg {
    float row[kMaxBilateral];      // a_m (= a_n: the mask is symmetric)
    float log2_col[kMaxBilateral]; // log2 a_n (tiles with colour)
    float c;                       // -log2(e) / (2 sigma_b^2)
    float range[kLutEntries];      // exp2(c * i * i), zero from 256 on
};

// The LDS serves one lookup per ~2 clocks and CU plus what the bank conflicts of a wave's 64 addresses cost (1.6 ... 4 clocks more
// by the image's content, SQ_LDS_BANK_CONFLICT), and that is the kernel's bound; the vector memory path idles meanwhile.  So some
// window columns take range(|d|) out of the kernel-argument block instead -- the same byte offset, a gather the L1 serves out of one
// or two cache lines for the |d| that matter -- at one more multiplication per tap (a_n is not folded into that table).
// A third engine is the transcendental unit: a column can also compute its weight (v_exp_f32, two more instructions).
// SPLIT = 10 * columns through memory (columns 1, 5) + columns computed (columns 3, 7, 0, WW - 1).  Measured on a 4K frame, 9 x 9
// (profiles/r04_ablation.txt batch 9): all LDS 108 us; two through memory 100; three 130 (the gather costs the texture path more
// than the LDS); two computed 95; one through memory + two computed 92-94 -- the default; more of either is slower again.
// OFX_LUT_SPLIT selects 0, 2, 10 or 12 at run time for the A/B.
#ifndef OFX_LUT_SPLIT_DEFAULT
#define OFX_LUT_SPLIT_DEFAULT 12
#endif
__device__ __host__ constexpr bool lut_column_in_memory(int n, int ww, int split) { return ww >= 7 && ((split / 10 >= 1 && n == 1) || (split / 10 >= 2 && n == 5)); }
__device__ __host__ constexpr bool lut_column_computed(int n, int ww, int split)
{
    return ww >= 7 && ((split % 10 >= 1 && n == 3) || (split % 10 >= 2 && n == 7 % ww) || (split % 10 >= 3 && n == 0) || (split % 10 >= 4 && n == ww - 1 && ww > 7));
}

// the taps of one tile row for the lane's two pixels of one output row: v = the WW + 1 tile values, g = the two centre values
template <int WW, int EVERY>
__device__ __forceinline__ void lut_row_taps(const float (&v)[WW + 1], float gA, float gB, const char *tabb, float am, float (&acc)[4], const BilateralLutArg &B)
{
    const char *rangeb = reinterpret_cast<const char *>(B.range);
    float wsA = 0.0f, asA = 0.0f, wsB = 0.0f, asB = 0.0f;
#pragma unroll
    for (int n = 0; n < WW; ++n) {
        const float dA = v[n] - gA, dB = v[n + 1] - gB; // exact: multiples of 4 below 2^12
        const uint32_t iA = (uint32_t)__builtin_fabsf(dA), iB = (uint32_t)__builtin_fabsf(dB); // = 4 |d|: the entry's byte offset
        if (lut_column_in_memory(n, WW, EVERY)) { // range(|d|) out of the kernel-argument block through the vector memory path; a_n applied here
            const float rA = *reinterpret_cast<const float *>(rangeb + iA), rB = *reinterpret_cast<const float *>(rangeb + iB);
            const float an = B.row[n];
            wsA = __builtin_fmaf(an, rA, wsA);
            asA = __builtin_fmaf(dA * an, rA, asA);
            wsB = __builtin_fmaf(an, rB, wsB);
            asB = __builtin_fmaf(dB * an, rB, asB);
        } else if (lut_column_computed(n, WW, EVERY)) { // (an out-of-image tap: d4 = -1024 - 4 g_0, the exponent far below the underflow for any sigma_b the entry accepts)
            const float wA = __builtin_amdgcn_exp2f(__builtin_fmaf(dA * dA, 0.0625f * B.c, B.log2_col[n]));
            const float wB = __builtin_amdgcn_exp2f(__builtin_fmaf(dB * dB, 0.0625f * B.c, B.log2_col[n]));
            wsA += wA;
            asA = __builtin_fmaf(dA, wA, asA);
            wsB += wB;
            asB = __builtin_fmaf(dB, wB, asB);
        } else {
            const float wA = *reinterpret_cast<const float *>(tabb + n * (kLutEntries * 4) + iA);
            const float wB = *reinterpret_cast<const float *>(tabb + n * (kLutEntries * 4) + iB);
            wsA += wA;
            asA = __builtin_fmaf(dA, wA, asA);
            wsB += wB;
            asB = __builtin_fmaf(dB, wB, asB);
        }
    }
    acc[0] = __builtin_fmaf(am, wsA, acc[0]);
    acc[1] = __builtin_fmaf(am, asA, acc[1]);
    acc[2] = __builtin_fmaf(am, wsB, acc[2]);
    acc[3] = __builtin_fmaf(am, asB, acc[3]);
}

// ---- host: the tables, filled once per (window, sigma_s, sigma_b) ------------------------------------------------------------
// The bit-exact filter's: the spatial mask of gpu::bilateral_filter (ofx_generate_gaussian_kernel) and the range weight
// 1/(2 pi sB^2) * pow(e, -k^2/(2 sB^2)) for k = 0 .. 255 -- the very expression the CPU path evaluates per tap.
inline void bilateral_exact_tables(double sigma_s, double sigma_b, int ww, BilateralArg *B)
{
    ofx_generate_gaussian_kernel(sigma_s, ww, B->spatial);
    const double sb2 = sigma_b * sigma_b;
    for (int k = 0; k < 256; ++k) {
        const double kk = (double)k * (double)k;
        B->range[k] = 1.0 / (2.0 * M_PI * sb2) * pow(M_E, -0.5 * (kk) / sb2);
    }
}

// The +-1 LSB filters' factors of a square window's spatial mask sp (ww x ww): ns(m, n) = a_m a_n with a_n = ns(c, n) / sqrt(ns(c, c)),
// c the centre -- checked, not assumed.  false: the mask is not separable (row / log2_col untouched).
inline bool bilateral_sep_rows(const double *sp, int ww, float *row, float *log2_col)
{
    const int c = ww >> 1;
    const double root = sqrt(sp[c * ww + c]);
    bool separable = root > 0.0;
    for (int m = 0; m < ww && separable; ++m)
        for (int n = 0; n < ww; ++n) {
            const double prod = (sp[c * ww + m] / root) * (sp[c * ww + n] / root);
            if (!(fabs(prod - sp[m * ww + n]) <= 1e-9 * sp[m * ww + n])) separable = false;
        }
    if (!separable) return false;
    for (int n = 0; n < ww; ++n) {
        row[n] = (float)(sp[c * ww + n] / root);
        log2_col[n] = (float)log2(sp[c * ww + n] / root);
    }
    return true;
}

// bilateral_lut_kernel's range table exp2(c i^2) (zero from 256 on) and its constant c = -log2(e) / (2 sigma_b^2)
inline void bilateral_lut_range(float c, BilateralLutArg *T)
{
    for (int i = 0; i < kLutEntries; ++i) T->range[i] = i < 256 ? (float)exp2((double)c * i * i) : 0.0f;
    T->c = c;
}

} // namespace
