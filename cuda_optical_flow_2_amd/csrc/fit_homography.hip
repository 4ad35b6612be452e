// Planar homography from point matches (the definition: "planar homography from point matches" in include/ofx.h): RANSAC over
// fit_motion's counter-based sampler with K = 4, an 8 x 8 elimination per hypothesis, integer inlier counts from a division-free
// rational residual, and a least-squares refit whose 23 sums are exact integers, eleven of them 128 bits wide.  5 + 2 refits
// launches per call:
//   hypotheses  one thread per (item, hypothesis): sample, build the 8 x 9 system in LDS (a thread's entries 64 doubles apart: a
//               run-time pivot row costs nothing there and no bank is shared), solve, store h0 .. h7 in the item's d_work with a
//               valid flag and a zero count; it also zeroes the item's sums;
//   score       (tile of matches, group of hypotheses, item): a lane keeps kPerLane matches as normalised float64 in registers, X
//               of an unusable match a NaN so that it fails the comparison without a flag; the models arrive as wave-uniform
//               loads, a wave's count is the population of its ballots, a block's goes through LDS and leaves as ONE integer
//               atomic per block and hypothesis; the first group's blocks count the usable matches too;
//   select      one block per item: the best hypothesis by an integer key, the status, the starting model;
//   sums        once per refit, (tile, item): the 23 sums over the tile's inliers of the current model, per thread in int64 and
//               __int128, across the wave and the block as 64-bit halves, into memory by one 64-bit atomic per narrow sum and two
//               per wide one (wide_sum.h);
//   solve       once per refit, one thread per item: the sums to float64 (wide_sum.h), the normal equations, the same solve; the
//               last one also conjugates the model to pixels;
//   final       (tile, item): the mask and the count of inliers under the final model;
//   output      one thread per item: d_model and d_info.
// The build has -ffp-contract=off: no float64 operation below is fused.  A product by a power of two stands for ldexp where no
// underflow can occur (it is exact).
#include <math.h>
#include <string.h>

#include "ofx_internal.h"
#include "fit_common.h"
#include "wide_sum.h"

namespace {

constexpr int kHypThreads = 64, kSolveThreads = 16;
constexpr int kScoreThreads = 256, kPerLane = 4, kTile = kScoreThreads * kPerLane, kGroup = 32;
constexpr int kSelectThreads = 256, kWaves = kScoreThreads / 64;
constexpr int kSums = 23, kNarrow = 12, kWide = kSums - kNarrow; // sums 0 .. 11 fit int64, 12 .. 22 need 128 bits
// the sums in order: m | Sx Sy SX SY | Sxx Sxy Syy SxX SyX SxY SyY | SxxX SxyX SyyX SxxY SxyY SyyY SxR SyR | SxxR SxyR SyyR
enum { M_, SX_, SY_, SVX_, SVY_, SXX_, SXY_, SYY_, SXVX_, SYVX_, SXVY_, SYVY_, SXXVX_, SXYVX_, SYYVX_, SXXVY_, SXYVY_, SYYVY_, SXR_, SYR_, SXXR_, SXYR_, SYYR_ };
__device__ const int kDegree[kSums] = {0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4};

struct HState { // the tail of d_work
    double cur[8];                               // the current model h0 .. h7 (h8 = 1)
    double out[9];                               // the final model in pixels
    unsigned long long lo[kFitMaxRefits][kSums]; // per refit pass: the sums' low halves (of a narrow sum: all of it)
    unsigned long long hi[kFitMaxRefits][kWide]; //                 the wide sums' high halves
    unsigned long long final_count;
    int usable, n_valid, best, best_count, status, done;
};
struct HItem {
    const float2 *p, *q;
    const int32_t *status;
    double *model;
    int32_t *info;
    uint8_t *inlier;
    double *models;   // d_work: [H][8]
    unsigned *counts; //         [H]
    int32_t *valid;   //         [H]
    HState *state;
    double inv, t, s, cx, cy; // SCALE and OUTPUTS: 2^-e, thr_q 2^-e, 2^(5-e), 16 (w - 1) 2^-e, 16 (h - 1) 2^-e
    int n, pair, w, h, e;
};
struct HArgs {
    HItem item[OFX_STREAM_MAX_BATCH];
    int hyp, refits;
    unsigned seed;
};

// SOLVE: M[(9 r + k) * stride] is entry (r, k) of the augmented system; false when INVALID
__device__ __forceinline__ bool solve8(double *M, const int stride, double (&h)[8])
{
#define OFX_M(r, k) M[(9 * (r) + (k)) * stride]
    for (int c = 0; c < 8; ++c) {
        int p = c;
        double best = fabs(OFX_M(c, c));
        for (int r = c + 1; r < 8; ++r) {
            const double a = fabs(OFX_M(r, c));
            if (a > best) best = a, p = r;
        }
        const double piv = OFX_M(p, c);
        if (piv == 0.0 || !__builtin_isfinite(piv)) return false;
        if (p != c)
            for (int k = c; k < 9; ++k) {
                const double a = OFX_M(p, k);
                OFX_M(p, k) = OFX_M(c, k), OFX_M(c, k) = a;
            }
        for (int r = c + 1; r < 8; ++r) {
            const double f = OFX_M(r, c) / piv;
            for (int k = c + 1; k < 9; ++k) OFX_M(r, k) = OFX_M(r, k) - f * OFX_M(c, k);
        }
    }
    bool finite = true;
#pragma unroll
    for (int c = 7; c >= 0; --c) {
        double s = OFX_M(c, 8);
#pragma unroll
        for (int k = c + 1; k < 8; ++k) s = s - OFX_M(c, k) * h[k];
        h[c] = s / OFX_M(c, c);
        finite = finite && __builtin_isfinite(h[c]);
    }
#undef OFX_M
    return finite;
}

__global__ __launch_bounds__(kHypThreads) void hfit_hypotheses_kernel(const HArgs A)
{
    const HItem &it = A.item[blockIdx.y];
    const int t = threadIdx.x, j = blockIdx.x * kHypThreads + t;
    __shared__ double lds[72 * kHypThreads];
    if (blockIdx.x == 0) {
        for (int k = t; k < kFitMaxRefits * kSums; k += kHypThreads) (&it.state->lo[0][0])[k] = 0ull;
        if (t < kFitMaxRefits * kWide) (&it.state->hi[0][0])[t] = 0ull;
        if (t == 0) it.state->usable = 0, it.state->final_count = 0ull, it.state->done = 0;
    }
    if (j >= A.hyp) return;
    int idx[4] = {-1, -1, -1, -1};
    double x[4], y[4], X[4], Y[4];
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bool found = false;
        for (int a = 0; a < 8 && valid && !found; ++a) {
            const int i = (int)(((unsigned long long)mix(A.seed, (unsigned)j, (unsigned)k, (unsigned)a) * (unsigned long long)it.n) >> 32);
            if (i == idx[0] || i == idx[1] || i == idx[2]) continue;
            int ux, uy, vx, vy;
            if (!load_match(it, i, ux, uy, vx, vy)) continue;
            idx[k] = i, found = true;
            x[k] = (double)ux * it.inv, y[k] = (double)uy * it.inv, X[k] = (double)vx * it.inv, Y[k] = (double)vy * it.inv;
        }
        valid = valid && found;
    }
    double h[8] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (valid) {
        double *M = lds + t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double r0[9] = {x[k], y[k], 1.0, 0.0, 0.0, 0.0, -(x[k] * X[k]), -(y[k] * X[k]), X[k]};
            const double r1[9] = {0.0, 0.0, 0.0, x[k], y[k], 1.0, -(x[k] * Y[k]), -(y[k] * Y[k]), Y[k]};
#pragma unroll
            for (int c = 0; c < 9; ++c) M[(9 * (2 * k) + c) * kHypThreads] = r0[c], M[(9 * (2 * k + 1) + c) * kHypThreads] = r1[c];
        }
        valid = solve8(M, kHypThreads, h);
#pragma unroll
        for (int k = 0; k < 4; ++k) valid = valid && (h[6] * x[k] + h[7] * y[k]) + 1.0 > 0.0;
    }
    double *m = it.models + 8 * (size_t)j;
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = h[k];
    it.valid[j] = valid ? 1 : 0;
    it.counts[j] = 0u;
}

__global__ __launch_bounds__(kScoreThreads) void hfit_score_kernel(const HArgs A)
{
    const HItem &it = A.item[blockIdx.z];
    const int base = blockIdx.x * kTile;
    if (base >= it.n) return; // (block-uniform: the grid is sized for the launch's largest item)
    __shared__ unsigned cnt[kGroup];
    const int t = threadIdx.x;
    if (t < kGroup) cnt[t] = 0u;
    unsigned usable = 0;
    // an unusable match, or a slot past the item's end, can never be an inlier: X = NaN makes rx NaN, and NaN <= .. is false
    double x[kPerLane], y[kPerLane], X[kPerLane], Y[kPerLane];
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int i = base + r * kScoreThreads + t;
        int a = 0, b = 0, c = 0, d = 0;
        const bool ok = i < it.n && load_match(it, i, a, b, c, d);
        x[r] = (double)a * it.inv, y[r] = (double)b * it.inv, X[r] = ok ? (double)c * it.inv : __builtin_nan(""), Y[r] = (double)d * it.inv;
        usable += (unsigned)__popcll(__ballot(ok));
    }
    if (blockIdx.y == 0 && (t & 63) == 0 && usable) atomicAdd(&it.state->usable, (int)usable); // (zeroed by hfit_hypotheses_kernel)
    __syncthreads();
    const int j0 = blockIdx.y * kGroup, j1 = min(j0 + kGroup, A.hyp);
    const double thr = it.t;
    for (int j = j0; j < j1; ++j) {
        if (!it.valid[j]) continue; // (wave-uniform)
        const double *m = it.models + 8 * (size_t)j;
        const double h0 = m[0], h1 = m[1], h2 = m[2], h3 = m[3], h4 = m[4], h5 = m[5], h6 = m[6], h7 = m[7];
        unsigned wave = 0;
#pragma unroll
        for (int r = 0; r < kPerLane; ++r) {
            const double W = (h6 * x[r] + h7 * y[r]) + 1.0;
            const double rx = ((h0 * x[r] + h1 * y[r]) + h2) - X[r] * W;
            const double ry = ((h3 * x[r] + h4 * y[r]) + h5) - Y[r] * W;
            const double tw = thr * W;
            wave += (unsigned)__popcll(__ballot(W > 0.0 && rx * rx + ry * ry <= tw * tw));
        }
        if ((t & 63) == 0 && wave) atomicAdd(&cnt[j - j0], wave);
    }
    __syncthreads();
    if (t < j1 - j0 && cnt[t]) atomicAdd(&it.counts[j0 + t], cnt[t]); // (zeroed by hfit_hypotheses_kernel, earlier on the stream)
}

// SCORE of one match from its lattice integers
__device__ __forceinline__ bool is_inlier(const HItem &it, const double *h, int ux, int uy, int vx, int vy)
{
    const double x = (double)ux * it.inv, y = (double)uy * it.inv, X = (double)vx * it.inv, Y = (double)vy * it.inv;
    const double W = (h[6] * x + h[7] * y) + 1.0;
    const double rx = ((h[0] * x + h[1] * y) + h[2]) - X * W;
    const double ry = ((h[3] * x + h[4] * y) + h[5]) - Y * W;
    const double tw = it.t * W;
    return W > 0.0 && rx * rx + ry * ry <= tw * tw;
}

// OUTPUTS: the current model conjugated to pixels; the item ends DEGENERATE when its entry 8 is 0 or not finite
__device__ __forceinline__ void finish_model(const HItem &it, HState *st)
{
    const double h[9] = {st->cur[0], st->cur[1], st->cur[2], st->cur[3], st->cur[4], st->cur[5], st->cur[6], st->cur[7], 1.0};
    double a[3][3], b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i][0] = h[3 * i] * it.s, a[i][1] = h[3 * i + 1] * it.s;
        a[i][2] = h[3 * i + 2] - (h[3 * i] * it.cx + h[3 * i + 1] * it.cy);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) b[0][j] = a[0][j] + it.cx * a[2][j], b[1][j] = a[1][j] + it.cy * a[2][j], b[2][j] = it.s * a[2][j];
    const double d = b[2][2];
    if (d == 0.0 || !__builtin_isfinite(d)) {
        st->status = OFX_FIT_DEGENERATE;
        return;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) st->out[3 * i + j] = b[i][j] / d;
}

__global__ __launch_bounds__(kSelectThreads) void hfit_select_kernel(const HArgs A)
{
    const HItem &it = A.item[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __shared__ unsigned long long keys[kSelectThreads / 64];
    __shared__ long long valids[kSelectThreads / 64];
    // the valid hypotheses, and the best one: the largest count, among equal counts the smallest j
    long long n_valid = 0;
    unsigned long long key = 0;
    for (int j = t; j < A.hyp; j += kSelectThreads)
        if (it.valid[j]) {
            const unsigned long long k = ((unsigned long long)(it.counts[j] + 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
            key = k > key ? k : key;
            ++n_valid;
        }
    n_valid = wave_sum64(n_valid), key = wave_max64(key);
    if (lane == 0) valids[wv] = n_valid, keys[wv] = key;
    __syncthreads();
    if (t != 0) return;
    n_valid = 0, key = 0;
    for (int k = 0; k < kSelectThreads / 64; ++k) {
        n_valid += valids[k];
        key = keys[k] > key ? keys[k] : key;
    }
    HState *st = it.state;
    const int status = st->usable < 4 ? OFX_FIT_FEW : n_valid == 0 ? OFX_FIT_DEGENERATE : OFX_FIT_OK;
    st->status = status, st->n_valid = (int)n_valid;
    if (status != OFX_FIT_OK) {
        st->best = -1, st->best_count = 0;
        return;
    }
    const int best = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    st->best = best, st->best_count = (int)((key >> 32) - 1ull);
    for (int k = 0; k < 8; ++k) st->cur[k] = it.models[8 * (size_t)best + k];
    if (A.refits == 0) finish_model(it, st);
}

__device__ __forceinline__ void wave_sum128(unsigned long long &lo, unsigned long long &hi)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long olo = (unsigned long long)__shfl_xor((long long)lo, s, 64), ohi = (unsigned long long)__shfl_xor((long long)hi, s, 64);
        wide_add(lo, hi, olo, ohi);
    }
}

__global__ __launch_bounds__(kScoreThreads) void hfit_sums_kernel(const HArgs A, const int pass)
{
    const HItem &it = A.item[blockIdx.y];
    const int base = blockIdx.x * kTile;
    if (base >= it.n || it.state->status != OFX_FIT_OK) return; // (block-uniform)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __shared__ unsigned long long part[kWaves][kSums][2];
    double h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = it.state->cur[k]; // (the solve of the pass before wrote it, earlier on the stream)
    long long s[kNarrow];
    __int128 ws[kWide];
#pragma unroll
    for (int k = 0; k < kNarrow; ++k) s[k] = 0;
#pragma unroll
    for (int k = 0; k < kWide; ++k) ws[k] = 0;
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int i = base + r * kScoreThreads + t;
        int a, b, c, d;
        if (i < it.n && load_match(it, i, a, b, c, d) && is_inlier(it, h, a, b, c, d)) {
            const long long x = a, y = b, X = c, Y = d; // |.| <= 2^20
            const long long xx = x * x, xy = x * y, yy = y * y, R = X * X + Y * Y; // <= 2^40, 2^41
            s[M_] += 1, s[SX_] += x, s[SY_] += y, s[SVX_] += X, s[SVY_] += Y, s[SXX_] += xx, s[SXY_] += xy, s[SYY_] += yy;
            s[SXVX_] += x * X, s[SYVX_] += y * X, s[SXVY_] += x * Y, s[SYVY_] += y * Y;
            ws[SXXVX_ - kNarrow] += (__int128)xx * X, ws[SXYVX_ - kNarrow] += (__int128)xy * X, ws[SYYVX_ - kNarrow] += (__int128)yy * X;
            ws[SXXVY_ - kNarrow] += (__int128)xx * Y, ws[SXYVY_ - kNarrow] += (__int128)xy * Y, ws[SYYVY_ - kNarrow] += (__int128)yy * Y;
            ws[SXR_ - kNarrow] += (__int128)x * R, ws[SYR_ - kNarrow] += (__int128)y * R;
            ws[SXXR_ - kNarrow] += (__int128)xx * R, ws[SXYR_ - kNarrow] += (__int128)xy * R, ws[SYYR_ - kNarrow] += (__int128)yy * R;
        }
    }
#pragma unroll
    for (int k = 0; k < kNarrow; ++k) {
        const long long r = wave_sum64(s[k]);
        if (lane == 0) part[wv][k][0] = (unsigned long long)r, part[wv][k][1] = 0ull;
    }
#pragma unroll
    for (int k = 0; k < kWide; ++k) {
        unsigned long long lo = (unsigned long long)ws[k], hi = (unsigned long long)(ws[k] >> 64);
        wave_sum128(lo, hi);
        if (lane == 0) part[wv][kNarrow + k][0] = lo, part[wv][kNarrow + k][1] = hi;
    }
    __syncthreads();
    if (t < kSums) {
        unsigned long long lo = 0, hi = 0;
        for (int k = 0; k < kWaves; ++k) wide_add(lo, hi, part[k][t][0], part[k][t][1]);
        // (two's complement: the unsigned sum of the blocks' parts is the signed one; zeroed by hfit_hypotheses_kernel)
        HState *st = it.state;
        if (t < kNarrow) {
            if (lo) atomicAdd(&st->lo[pass][t], lo);
        } else if (lo | hi) {
            const unsigned long long old = atomicAdd(&st->lo[pass][t], lo);
            const unsigned long long up = hi + wide_carry(old, lo);
            if (up) atomicAdd(&st->hi[pass][t - kNarrow], up);
        }
    }
}

// REFIT on the finished sums of a pass, one thread per item
__global__ __launch_bounds__(kSolveThreads) void hfit_solve_kernel(const HArgs A, const int n_items, const int pass)
{
    const int t = threadIdx.x;
    __shared__ double lds[72 * kSolveThreads];
    if (t >= n_items) return;
    const HItem &it = A.item[t];
    HState *st = it.state;
    if (st->status != OFX_FIT_OK) return;
    double S[kSums];
    for (int k = 0; k < kSums; ++k) {
        const unsigned long long lo = st->lo[pass][k];
        const double v = k < kNarrow ? (double)(long long)lo : wide_to_double(lo, st->hi[pass][k - kNarrow]);
        S[k] = ldexp(v, -kDegree[k] * it.e);
    }
    if ((long long)st->lo[pass][M_] >= 4) {
        const double rows[8][9] = {
            {S[SXX_], S[SXY_], S[SX_], 0.0, 0.0, 0.0, -S[SXXVX_], -S[SXYVX_], S[SXVX_]},
            {S[SXY_], S[SYY_], S[SY_], 0.0, 0.0, 0.0, -S[SXYVX_], -S[SYYVX_], S[SYVX_]},
            {S[SX_], S[SY_], S[M_], 0.0, 0.0, 0.0, -S[SXVX_], -S[SYVX_], S[SVX_]},
            {0.0, 0.0, 0.0, S[SXX_], S[SXY_], S[SX_], -S[SXXVY_], -S[SXYVY_], S[SXVY_]},
            {0.0, 0.0, 0.0, S[SXY_], S[SYY_], S[SY_], -S[SXYVY_], -S[SYYVY_], S[SYVY_]},
            {0.0, 0.0, 0.0, S[SX_], S[SY_], S[M_], -S[SXVY_], -S[SYVY_], S[SVY_]},
            {-S[SXXVX_], -S[SXYVX_], -S[SXVX_], -S[SXXVY_], -S[SXYVY_], -S[SXVY_], S[SXXR_], S[SXYR_], -S[SXR_]},
            {-S[SXYVX_], -S[SYYVX_], -S[SYVX_], -S[SXYVY_], -S[SYYVY_], -S[SYVY_], S[SXYR_], S[SYYR_], -S[SYR_]}};
        double *M = lds + t;
        for (int r = 0; r < 8; ++r)
            for (int k = 0; k < 9; ++k) M[(9 * r + k) * kSolveThreads] = rows[r][k];
        double h[8];
        if (solve8(M, kSolveThreads, h)) {
            for (int k = 0; k < 8; ++k) st->cur[k] = h[k];
            st->done += 1;
        }
    }
    if (pass == A.refits - 1) finish_model(it, st);
}

__global__ __launch_bounds__(kScoreThreads) void hfit_final_kernel(const HArgs A)
{
    const HItem &it = A.item[blockIdx.y];
    const int base = blockIdx.x * kTile;
    if (base >= it.n) return; // (block-uniform)
    const int t = threadIdx.x;
    const bool fit = it.state->status == OFX_FIT_OK;
    if (!fit && it.inlier == nullptr) return;
    __shared__ unsigned block_count;
    if (t == 0) block_count = 0u;
    __syncthreads();
    double h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = fit ? it.state->cur[k] : 0.0;
    unsigned count = 0;
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int i = base + r * kScoreThreads + t;
        int a, b, c, d;
        const bool in = fit && i < it.n && load_match(it, i, a, b, c, d) && is_inlier(it, h, a, b, c, d);
        count += (unsigned)__popcll(__ballot(in));
        if (it.inlier && i < it.n) it.inlier[i] = in ? 1 : 0;
    }
    if ((t & 63) == 0 && count) atomicAdd(&block_count, count);
    __syncthreads();
    if (t == 0 && block_count) atomicAdd(&it.state->final_count, (unsigned long long)block_count);
}

__global__ void hfit_output_kernel(const HArgs A, const int n_items)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const HItem &it = A.item[i];
    const HState *st = it.state;
    const bool fit = st->status == OFX_FIT_OK;
    for (int k = 0; k < 9; ++k) it.model[k] = fit ? st->out[k] : (k % 4 == 0 ? 1.0 : 0.0);
    it.info[0] = st->status, it.info[1] = st->usable, it.info[2] = st->n_valid, it.info[3] = fit ? st->best : -1, it.info[4] = fit ? st->best_count : 0;
    it.info[5] = fit ? (int)st->final_count : 0, it.info[6] = fit ? st->done : 0, it.info[7] = 0;
}

int check_params(const ofx_fit_params *prm, const char *who)
{
    OFX_REQUIRE(prm != nullptr, "%s: prm is null", who);
    OFX_REQUIRE(prm->model == OFX_MOTION_HOMOGRAPHY, "%s: model = %d is not 3 (OFX_MOTION_HOMOGRAPHY)", who, prm->model);
    OFX_REQUIRE(prm->hypotheses >= 1 && prm->hypotheses <= kFitMaxHyp, "%s: hypotheses = %d is not in 1 .. %d", who, prm->hypotheses, kFitMaxHyp);
    OFX_REQUIRE(prm->thr_q >= 0 && prm->thr_q <= kFitMaxThr, "%s: thr_q = %d is not in 0 .. 2^15", who, prm->thr_q);
    OFX_REQUIRE(prm->refits >= 0 && prm->refits <= kFitMaxRefits, "%s: refits = %d is not in 0 .. %d", who, prm->refits, kFitMaxRefits);
    return OFX_OK;
}

} // namespace

extern "C" size_t ofx_fit_homography_work_bytes(const ofx_fit_params *prm)
{
    if (check_params(prm, "ofx_fit_homography_work_bytes") != OFX_OK) return 0;
    return (size_t)prm->hypotheses * (8 * sizeof(double) + sizeof(unsigned) + sizeof(int32_t)) + sizeof(HState);
}

extern "C" int ofx_fit_homography(const ofx_fit_desc *items, int n_items, const ofx_fit_params *prm, void *stream)
{
    const char *who = "ofx_fit_homography";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_TRY(check_params(prm, who));
    OFX_REQUIRE(n_items >= 1 && n_items <= OFX_STREAM_MAX_BATCH, "%s: n_items = %d is not in 1 .. %d", who, n_items, OFX_STREAM_MAX_BATCH);
    static thread_local HArgs A;
    memset(&A, 0, sizeof A);
    const int H = prm->hypotheses;
    int n_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const ofx_fit_desc &d = items[i];
        OFX_REQUIRE(d.d_p != nullptr && d.d_q != nullptr, "%s: item %d: d_p or d_q is null", who, i);
        OFX_REQUIRE(d.d_model != nullptr && d.d_info != nullptr, "%s: item %d: d_model or d_info is null", who, i);
        OFX_REQUIRE(d.d_work != nullptr, "%s: item %d: d_work is null", who, i);
        OFX_REQUIRE(d.n >= 1 && d.n <= kFitMaxMatches, "%s: item %d: n = %d is not in 1 .. 2^20", who, i, d.n);
        OFX_REQUIRE(d.w >= 1 && d.w <= kFitMaxSize && d.h >= 1 && d.h <= kFitMaxSize, "%s: item %d: the size %d x %d is not in 1 .. 2^16", who, i, d.w, d.h);
        OFX_REQUIRE(((uintptr_t)d.d_p & 7) == 0 && ((uintptr_t)d.d_q & 7) == 0, "%s: item %d: d_p and d_q must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_model & 7) == 0, "%s: item %d: d_model must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_work & 7) == 0, "%s: item %d: d_work must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_info & 3) == 0 && ((uintptr_t)d.d_status & 3) == 0, "%s: item %d: d_info and d_status must be 4-byte aligned", who, i);
        HItem &it = A.item[i];
        it.p = reinterpret_cast<const float2 *>(d.d_p), it.q = reinterpret_cast<const float2 *>(d.d_q), it.status = d.d_status;
        it.model = d.d_model, it.info = d.d_info, it.inlier = d.d_inlier;
        it.models = static_cast<double *>(d.d_work);
        it.counts = reinterpret_cast<unsigned *>(it.models + 8 * (size_t)H);
        it.valid = reinterpret_cast<int32_t *>(it.counts + H);
        it.state = reinterpret_cast<HState *>(it.valid + H); // (72 H bytes in: 8-byte aligned)
        it.n = d.n, it.pair = d.pair, it.w = d.w, it.h = d.h;
        const int ox = 16 * (d.w - 1), oy = 16 * (d.h - 1), big = ox > oy ? ox : oy;
        int e = 0;
        while ((1 << e) < big) ++e; // SCALE: the smallest e with 2^e >= max(ox, oy, 1)
        it.e = e, it.inv = ldexp(1.0, -e), it.t = ldexp((double)prm->thr_q, -e);
        it.s = ldexp(1.0, 5 - e), it.cx = ldexp((double)ox, -e), it.cy = ldexp((double)oy, -e);
        n_max = d.n > n_max ? d.n : n_max;
    }
    A.hyp = H, A.refits = prm->refits, A.seed = prm->seed;
    hipStream_t st = ofx_stream(stream);
    hipLaunchKernelGGL(hfit_hypotheses_kernel, dim3(ofx_div_up(H, kHypThreads), n_items), dim3(kHypThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(hfit_score_kernel, dim3(ofx_div_up(n_max, kTile), ofx_div_up(H, kGroup), n_items), dim3(kScoreThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(hfit_select_kernel, dim3(n_items), dim3(kSelectThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    const dim3 tiles(ofx_div_up(n_max, kTile), n_items);
    for (int pass = 0; pass < prm->refits; ++pass) {
        hipLaunchKernelGGL(hfit_sums_kernel, tiles, dim3(kScoreThreads), 0, st, A, pass);
        OFX_HIP(hipGetLastError());
        hipLaunchKernelGGL(hfit_solve_kernel, dim3(1), dim3(kSolveThreads), 0, st, A, n_items, pass);
        OFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(hfit_final_kernel, tiles, dim3(kScoreThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(hfit_output_kernel, dim3(1), dim3(64), 0, st, A, n_items);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
