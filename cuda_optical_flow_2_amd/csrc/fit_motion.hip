// Camera motion from point matches (the definition: "camera motion from point matches" in include/ofx.h): RANSAC over a
// counter-based sampler with integer inlier counts and a least-squares refit on exact int64 sums.  5 + refits launches per call:
//   hypotheses  one thread per (item, hypothesis): sample, build the six float64 once, store them in the item's d_work with a
//               valid flag and a zero count -- built once, so every later reader sees the same bits; it also zeroes the item's
//               sums;
//   score       (tile of matches, group of hypotheses, item): a lane keeps kPerLane matches as centred float64 lattice values in
//               registers, the models arrive as wave-uniform loads, a wave's count is the population of its ballots, a block's
//               goes through LDS and leaves as ONE integer atomic per block and hypothesis; the first group's blocks count the
//               usable matches too;
//   select      one block per item: the best hypothesis by an integer key, the status, the starting model;
//   sums        once per refit, (tile, item): the twelve int64 sums over the tile's inliers of the current model, one atomic per
//               block and sum.  The current model of pass r is the starting model put through the solves of passes 0 .. r - 1,
//               which every thread works out from the finished sums: the same operations on the same integers, the same bits;
//   final       (tile, item): the mask and the count of inliers under the final model;
//   output      one thread per item: d_model and d_info.
// The build has -ffp-contract=off: no float64 operation below is fused.  Integer -> float64 conversions are the compiler's, which
// round to nearest even.  Also here: the two host-only helpers ofx_motion_compose and ofx_motion_invert.
#include <math.h>
#include <string.h>

#include "ofx_internal.h"
#include "fit_common.h"

namespace {

constexpr int kMaxMatches = kFitMaxMatches, kMaxSize = kFitMaxSize, kMaxHyp = kFitMaxHyp, kMaxThr = kFitMaxThr, kMaxRefits = kFitMaxRefits;
constexpr int kHypThreads = 128;
constexpr int kScoreThreads = 256, kPerLane = 4, kTile = kScoreThreads * kPerLane, kGroup = 32;
constexpr int kSelectThreads = 256, kWaves = kScoreThreads / 64;
constexpr int kSums = 12, kSlots = kMaxRefits + 1; // a slot of sums per refit pass, and one for the final count

struct FitItem {
    const float2 *p, *q;
    const int32_t *status;
    double *model;
    int32_t *info;
    uint8_t *inlier;
    double *models;      // d_work: [H][6]
    unsigned *counts;    //         [H]
    int32_t *valid;      //         [H]
    struct FitState *state;
    int n, pair, w, h;
};
struct FitState { // the tail of d_work
    double start[6];            // the best hypothesis's model
    long long sums[kSlots][kSums];
    int usable, n_valid, best, best_count, status, pad;
};
struct FitArgs {
    FitItem item[OFX_STREAM_MAX_BATCH];
    int model, hyp, refits;
    unsigned seed;
    double thr2;
};

__global__ __launch_bounds__(kHypThreads) void fit_hypotheses_kernel(const FitArgs A)
{
    const FitItem &it = A.item[blockIdx.y];
    const int j = blockIdx.x * kHypThreads + threadIdx.x;
    if (blockIdx.x == 0) {
        if (threadIdx.x < kSlots * kSums) (&it.state->sums[0][0])[threadIdx.x] = 0;
        if (threadIdx.x == 0) it.state->usable = 0;
    }
    if (j >= A.hyp) return;
    const int K = A.model + 1;
    int idx[3] = {-1, -1, -1};
    long long u[3][2], v[3][2];
    bool valid = true;
    for (int k = 0; k < K && valid; ++k) {
        bool found = false;
        for (int a = 0; a < 8 && !found; ++a) {
            const int i = (int)(((unsigned long long)mix(A.seed, (unsigned)j, (unsigned)k, (unsigned)a) * (unsigned long long)it.n) >> 32);
            if (i == idx[0] || i == idx[1]) continue;
            int ux, uy, vx, vy;
            if (!load_match(it, i, ux, uy, vx, vy)) continue;
            idx[k] = i, u[k][0] = ux, u[k][1] = uy, v[k][0] = vx, v[k][1] = vy, found = true;
        }
        valid = found;
    }
    double a = 1.0, b = 0.0, c = 0.0, d = 1.0, tx = 0.0, ty = 0.0;
    if (valid) {
        if (A.model == OFX_MOTION_TRANSLATION) {
            tx = (double)(v[0][0] - u[0][0]), ty = (double)(v[0][1] - u[0][1]);
        } else {
            if (A.model == OFX_MOTION_SIMILARITY) {
                const long long dpx = u[1][0] - u[0][0], dpy = u[1][1] - u[0][1], dqx = v[1][0] - v[0][0], dqy = v[1][1] - v[0][1];
                const long long den = dpx * dpx + dpy * dpy;
                valid = den != 0;
                if (valid) {
                    const double sa = (double)(dpx * dqx + dpy * dqy) / (double)den, sb = (double)(dpx * dqy - dpy * dqx) / (double)den;
                    a = sa, b = -sb, c = sb, d = sa;
                }
            } else {
                const long long d1x = u[1][0] - u[0][0], d1y = u[1][1] - u[0][1], d2x = u[2][0] - u[0][0], d2y = u[2][1] - u[0][1];
                const long long e1x = v[1][0] - v[0][0], e1y = v[1][1] - v[0][1], e2x = v[2][0] - v[0][0], e2y = v[2][1] - v[0][1];
                const long long det = d1x * d2y - d1y * d2x;
                valid = det != 0;
                if (valid) {
                    a = (double)(e1x * d2y - e2x * d1y) / (double)det;
                    b = (double)(e2x * d1x - e1x * d2x) / (double)det;
                    c = (double)(e1y * d2y - e2y * d1y) / (double)det;
                    d = (double)(e2y * d1x - e1y * d2x) / (double)det;
                }
            }
            if (valid) {
                const double u0x = (double)u[0][0], u0y = (double)u[0][1];
                tx = (double)v[0][0] - (a * u0x + b * u0y);
                ty = (double)v[0][1] - (c * u0x + d * u0y);
            }
        }
    }
    double *m = it.models + 6 * (size_t)j;
    m[0] = a, m[1] = b, m[2] = tx, m[3] = c, m[4] = d, m[5] = ty;
    it.valid[j] = valid ? 1 : 0;
    it.counts[j] = 0u;
}

__global__ __launch_bounds__(kScoreThreads) void fit_score_kernel(const FitArgs A)
{
    const FitItem &it = A.item[blockIdx.z];
    const int base = blockIdx.x * kTile;
    if (base >= it.n) return; // (block-uniform: the grid is sized for the launch's largest item)
    __shared__ unsigned cnt[kGroup];
    const int t = threadIdx.x;
    if (t < kGroup) cnt[t] = 0u;
    unsigned usable = 0;
    // an unusable match, or a slot past the item's end, can never be an inlier: vx = NaN makes e2 NaN, and NaN <= thr2 is false
    double ux[kPerLane], uy[kPerLane], vx[kPerLane], vy[kPerLane];
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int i = base + r * kScoreThreads + t;
        int a = 0, b = 0, c = 0, d = 0;
        const bool ok = i < it.n && load_match(it, i, a, b, c, d);
        ux[r] = (double)a, uy[r] = (double)b, vx[r] = ok ? (double)c : __builtin_nan(""), vy[r] = (double)d;
        usable += (unsigned)__popcll(__ballot(ok));
    }
    if (blockIdx.y == 0 && (t & 63) == 0 && usable) atomicAdd(&it.state->usable, (int)usable); // (zeroed by fit_hypotheses_kernel)
    __syncthreads();
    const int j0 = blockIdx.y * kGroup, j1 = min(j0 + kGroup, A.hyp);
    const double thr2 = A.thr2;
    for (int j = j0; j < j1; ++j) {
        if (!it.valid[j]) continue; // (wave-uniform)
        const double *m = it.models + 6 * (size_t)j;
        const double a = m[0], b = m[1], tx = m[2], c = m[3], d = m[4], ty = m[5];
        unsigned wave = 0;
#pragma unroll
        for (int r = 0; r < kPerLane; ++r) {
            const double rx = (a * ux[r] + b * uy[r]) + (tx - vx[r]);
            const double ry = (c * ux[r] + d * uy[r]) + (ty - vy[r]);
            const double e2 = rx * rx + ry * ry;
            wave += (unsigned)__popcll(__ballot(e2 <= thr2));
        }
        if ((t & 63) == 0 && wave) atomicAdd(&cnt[j - j0], wave);
    }
    __syncthreads();
    if (t < j1 - j0 && cnt[t]) atomicAdd(&it.counts[j0 + t], cnt[t]); // (zeroed by fit_hypotheses_kernel, earlier on the stream)
}

struct Model {
    double a, b, tx, c, d, ty;
};

__device__ __forceinline__ bool is_inlier(const Model &m, int ux, int uy, int vx, int vy, double thr2)
{
    const double x = (double)ux, y = (double)uy;
    const double rx = (m.a * x + m.b * y) + (m.tx - (double)vx);
    const double ry = (m.c * x + m.d * y) + (m.ty - (double)vy);
    return rx * rx + ry * ry <= thr2;
}

__global__ __launch_bounds__(kSelectThreads) void fit_select_kernel(const FitArgs A)
{
    const FitItem &it = A.item[blockIdx.x];
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
    FitState *st = it.state;
    const int status = st->usable < A.model + 1 ? OFX_FIT_FEW : n_valid == 0 ? OFX_FIT_DEGENERATE : OFX_FIT_OK;
    st->status = status, st->n_valid = (int)n_valid, st->pad = 0;
    if (status != OFX_FIT_OK) {
        st->best = -1, st->best_count = 0;
        st->start[0] = 1.0, st->start[1] = 0.0, st->start[2] = 0.0, st->start[3] = 0.0, st->start[4] = 1.0, st->start[5] = 0.0;
        return;
    }
    const int best = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    st->best = best, st->best_count = (int)((key >> 32) - 1ull);
    for (int k = 0; k < 6; ++k) st->start[k] = it.models[6 * (size_t)best + k];
}

// REFIT on one pass's finished sums; false (and m as it was) when the refit is skipped
__device__ __forceinline__ bool refit(int model, const long long *s, Model &m)
{
    const double N = (double)s[0], Sx = (double)s[1], Sy = (double)s[2], Sxx = (double)s[3], Sxy = (double)s[4], Syy = (double)s[5], Vx = (double)s[6],
                 Vy = (double)s[7], Sxvx = (double)s[8], Syvx = (double)s[9], Sxvy = (double)s[10], Syvy = (double)s[11];
    if (model == OFX_MOTION_TRANSLATION) {
        if (s[0] == 0) return false;
        m.tx = (Vx - Sx) / N, m.ty = (Vy - Sy) / N;
        return true;
    }
    const double Cxx = N * Sxx - Sx * Sx, Cyy = N * Syy - Sy * Sy, Cxy = N * Sxy - Sx * Sy;
    const double Cxvx = N * Sxvx - Sx * Vx, Cyvx = N * Syvx - Sy * Vx, Cxvy = N * Sxvy - Sx * Vy, Cyvy = N * Syvy - Sy * Vy;
    if (model == OFX_MOTION_SIMILARITY) {
        const double den = Cxx + Cyy;
        if (!(den > 0.0)) return false;
        const double sa = (Cxvx + Cyvy) / den, sb = (Cxvy - Cyvx) / den;
        m.a = sa, m.b = -sb, m.c = sb, m.d = sa;
    } else {
        const double D = Cxx * Cyy - Cxy * Cxy;
        if (!(D > 0.0)) return false;
        m.a = (Cyy * Cxvx - Cxy * Cyvx) / D;
        m.b = (Cxx * Cyvx - Cxy * Cxvx) / D;
        m.c = (Cyy * Cxvy - Cxy * Cyvy) / D;
        m.d = (Cxx * Cyvy - Cxy * Cxvy) / D;
    }
    m.tx = (Vx - (m.a * Sx + m.b * Sy)) / N;
    m.ty = (Vy - (m.c * Sx + m.d * Sy)) / N;
    return true;
}

// the model after `passes` refits (their sums are finished: earlier launches wrote them); returns how many were not skipped
__device__ __forceinline__ int model_after(const FitState *st, int model, int passes, Model &m)
{
    m.a = st->start[0], m.b = st->start[1], m.tx = st->start[2], m.c = st->start[3], m.d = st->start[4], m.ty = st->start[5];
    int done = 0;
    for (int r = 0; r < passes; ++r) done += refit(model, st->sums[r], m) ? 1 : 0;
    return done;
}

__global__ __launch_bounds__(kScoreThreads) void fit_sums_kernel(const FitArgs A, const int pass)
{
    const FitItem &it = A.item[blockIdx.y];
    const int base = blockIdx.x * kTile;
    if (base >= it.n || it.state->status != OFX_FIT_OK) return; // (block-uniform)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __shared__ long long part[kWaves][kSums];
    Model m;
    model_after(it.state, A.model, pass, m);
    long long s[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0;
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int i = base + r * kScoreThreads + t;
        int a, b, c, d;
        if (i < it.n && load_match(it, i, a, b, c, d) && is_inlier(m, a, b, c, d, A.thr2)) {
            const long long x = a, y = b, p = c, q = d;
            s[0] += 1, s[1] += x, s[2] += y, s[3] += x * x, s[4] += x * y, s[5] += y * y;
            s[6] += p, s[7] += q, s[8] += x * p, s[9] += y * p, s[10] += x * q, s[11] += y * q;
        }
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        const long long r = wave_sum64(s[k]);
        if (lane == 0) part[wv][k] = r;
    }
    __syncthreads();
    if (t < kSums) {
        long long r = 0;
        for (int k = 0; k < kWaves; ++k) r += part[k][t];
        // (two's complement: the unsigned sum of the blocks' parts is the signed one; zeroed by fit_hypotheses_kernel)
        if (r) atomicAdd(reinterpret_cast<unsigned long long *>(&it.state->sums[pass][t]), (unsigned long long)r);
    }
}

__global__ __launch_bounds__(kScoreThreads) void fit_final_kernel(const FitArgs A)
{
    const FitItem &it = A.item[blockIdx.y];
    const int base = blockIdx.x * kTile;
    if (base >= it.n) return; // (block-uniform)
    const int t = threadIdx.x;
    const bool fit = it.state->status == OFX_FIT_OK;
    if (!fit && it.inlier == nullptr) return;
    __shared__ unsigned block_count;
    if (t == 0) block_count = 0u;
    __syncthreads();
    Model m;
    model_after(it.state, A.model, A.refits, m);
    unsigned count = 0;
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int i = base + r * kScoreThreads + t;
        int a, b, c, d;
        const bool in = fit && i < it.n && load_match(it, i, a, b, c, d) && is_inlier(m, a, b, c, d, A.thr2);
        count += (unsigned)__popcll(__ballot(in));
        if (it.inlier && i < it.n) it.inlier[i] = in ? 1 : 0;
    }
    if ((t & 63) == 0 && count) atomicAdd(&block_count, count);
    __syncthreads();
    if (t == 0 && block_count) atomicAdd(reinterpret_cast<unsigned long long *>(&it.state->sums[A.refits][0]), (unsigned long long)block_count);
}

__global__ void fit_output_kernel(const FitArgs A, const int n_items)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const FitItem &it = A.item[i];
    const FitState *st = it.state;
    Model m;
    const int done = model_after(st, A.model, st->status == OFX_FIT_OK ? A.refits : 0, m);
    if (st->status == OFX_FIT_OK) {
        const double ox = (double)(16 * (it.w - 1)), oy = (double)(16 * (it.h - 1));
        it.model[0] = m.a, it.model[1] = m.b, it.model[2] = ((m.tx + ox) - (m.a * ox + m.b * oy)) / 32.0;
        it.model[3] = m.c, it.model[4] = m.d, it.model[5] = ((m.ty + oy) - (m.c * ox + m.d * oy)) / 32.0;
    } else {
        it.model[0] = 1.0, it.model[1] = 0.0, it.model[2] = 0.0, it.model[3] = 0.0, it.model[4] = 1.0, it.model[5] = 0.0;
    }
    it.info[0] = st->status, it.info[1] = st->usable, it.info[2] = st->n_valid, it.info[3] = st->best, it.info[4] = st->best_count;
    it.info[5] = st->status == OFX_FIT_OK ? (int)st->sums[A.refits][0] : 0, it.info[6] = done, it.info[7] = 0;
}

int check_params(const ofx_fit_params *prm, const char *who)
{
    OFX_REQUIRE(prm != nullptr, "%s: prm is null", who);
    OFX_REQUIRE(prm->model >= OFX_MOTION_TRANSLATION && prm->model <= OFX_MOTION_AFFINE, "%s: model = %d is not in 0 .. 2", who, prm->model);
    OFX_REQUIRE(prm->hypotheses >= 1 && prm->hypotheses <= kMaxHyp, "%s: hypotheses = %d is not in 1 .. %d", who, prm->hypotheses, kMaxHyp);
    OFX_REQUIRE(prm->thr_q >= 0 && prm->thr_q <= kMaxThr, "%s: thr_q = %d is not in 0 .. 2^15", who, prm->thr_q);
    OFX_REQUIRE(prm->refits >= 0 && prm->refits <= kMaxRefits, "%s: refits = %d is not in 0 .. %d", who, prm->refits, kMaxRefits);
    return OFX_OK;
}

} // namespace

extern "C" size_t ofx_fit_motion_work_bytes(const ofx_fit_params *prm)
{
    if (check_params(prm, "ofx_fit_motion_work_bytes") != OFX_OK) return 0;
    return (size_t)prm->hypotheses * (6 * sizeof(double) + sizeof(unsigned) + sizeof(int32_t)) + sizeof(FitState);
}

extern "C" int ofx_fit_motion(const ofx_fit_desc *items, int n_items, const ofx_fit_params *prm, void *stream)
{
    const char *who = "ofx_fit_motion";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_TRY(check_params(prm, who));
    OFX_REQUIRE(n_items >= 1 && n_items <= OFX_STREAM_MAX_BATCH, "%s: n_items = %d is not in 1 .. %d", who, n_items, OFX_STREAM_MAX_BATCH);
    static thread_local FitArgs A;
    memset(&A, 0, sizeof A);
    const int H = prm->hypotheses;
    int n_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const ofx_fit_desc &d = items[i];
        OFX_REQUIRE(d.d_p != nullptr && d.d_q != nullptr, "%s: item %d: d_p or d_q is null", who, i);
        OFX_REQUIRE(d.d_model != nullptr && d.d_info != nullptr, "%s: item %d: d_model or d_info is null", who, i);
        OFX_REQUIRE(d.d_work != nullptr, "%s: item %d: d_work is null", who, i);
        OFX_REQUIRE(d.n >= 1 && d.n <= kMaxMatches, "%s: item %d: n = %d is not in 1 .. 2^20", who, i, d.n);
        OFX_REQUIRE(d.w >= 1 && d.w <= kMaxSize && d.h >= 1 && d.h <= kMaxSize, "%s: item %d: the size %d x %d is not in 1 .. 2^16", who, i, d.w, d.h);
        OFX_REQUIRE(((uintptr_t)d.d_p & 7) == 0 && ((uintptr_t)d.d_q & 7) == 0, "%s: item %d: d_p and d_q must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_model & 7) == 0, "%s: item %d: d_model must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_work & 7) == 0, "%s: item %d: d_work must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_info & 3) == 0 && ((uintptr_t)d.d_status & 3) == 0, "%s: item %d: d_info and d_status must be 4-byte aligned", who, i);
        FitItem &it = A.item[i];
        it.p = reinterpret_cast<const float2 *>(d.d_p), it.q = reinterpret_cast<const float2 *>(d.d_q), it.status = d.d_status;
        it.model = d.d_model, it.info = d.d_info, it.inlier = d.d_inlier;
        it.models = static_cast<double *>(d.d_work);
        it.counts = reinterpret_cast<unsigned *>(it.models + 6 * (size_t)H);
        it.valid = reinterpret_cast<int32_t *>(it.counts + H);
        it.state = reinterpret_cast<FitState *>(it.valid + H); // (56 H bytes in: 8-byte aligned)
        it.n = d.n, it.pair = d.pair, it.w = d.w, it.h = d.h;
        n_max = d.n > n_max ? d.n : n_max;
    }
    A.model = prm->model, A.hyp = H, A.refits = prm->refits, A.seed = prm->seed;
    A.thr2 = (double)prm->thr_q * (double)prm->thr_q;
    hipStream_t st = ofx_stream(stream);
    hipLaunchKernelGGL(fit_hypotheses_kernel, dim3(ofx_div_up(H, kHypThreads), n_items), dim3(kHypThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_score_kernel, dim3(ofx_div_up(n_max, kTile), ofx_div_up(H, kGroup), n_items), dim3(kScoreThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_select_kernel, dim3(n_items), dim3(kSelectThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    const dim3 tiles(ofx_div_up(n_max, kTile), n_items);
    for (int pass = 0; pass < prm->refits; ++pass) {
        hipLaunchKernelGGL(fit_sums_kernel, tiles, dim3(kScoreThreads), 0, st, A, pass);
        OFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(fit_final_kernel, tiles, dim3(kScoreThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_output_kernel, dim3(1), dim3(64), 0, st, A, n_items);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_motion_compose(const double *m2, const double *m1, double *out)
{
    OFX_REQUIRE(m2 != nullptr && m1 != nullptr && out != nullptr, "ofx_motion_compose: m2, m1 or out is null");
    const double a2 = m2[0], b2 = m2[1], tx2 = m2[2], c2 = m2[3], d2 = m2[4], ty2 = m2[5];
    const double a1 = m1[0], b1 = m1[1], tx1 = m1[2], c1 = m1[3], d1 = m1[4], ty1 = m1[5];
    out[0] = a2 * a1 + b2 * c1, out[1] = a2 * b1 + b2 * d1, out[2] = (a2 * tx1 + b2 * ty1) + tx2;
    out[3] = c2 * a1 + d2 * c1, out[4] = c2 * b1 + d2 * d1, out[5] = (c2 * tx1 + d2 * ty1) + ty2;
    return OFX_OK;
}

extern "C" int ofx_motion_invert(const double *m, double *out)
{
    OFX_REQUIRE(m != nullptr && out != nullptr, "ofx_motion_invert: m or out is null");
    const double a = m[0], b = m[1], tx = m[2], c = m[3], d = m[4], ty = m[5];
    const double det = a * d - b * c;
    OFX_REQUIRE(det != 0.0 && __builtin_isfinite(det), "ofx_motion_invert: the determinant is 0 or not finite");
    const double ia = d / det, ib = -b / det, ic = -c / det, id = a / det;
    out[0] = ia, out[1] = ib, out[2] = -(ia * tx + ib * ty);
    out[3] = ic, out[4] = id, out[5] = -(ic * tx + id * ty);
    return OFX_OK;
}
