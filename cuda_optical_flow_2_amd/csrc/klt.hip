// Sparse pyramidal Lucas-Kanade (ofx_track_points).  The definition is the comment block "sparse Lucas-Kanade tracking" in
// include/ofx.h; DESIGN.md section 4.17 has the choices and the times.
//
// ONE launch.  A wave64 owns a point (four points per block of 256 threads; a block takes its points in turn) and walks the
// call's pairs and, per pair, the levels from the coarsest down; pair and level are wave-uniform, so the plane pointers -- a table
// of at most 17 x 8 in the kernel arguments -- are picked by scalar loads.  Per level the wave brings the (2R + 4)^2 bytes of A
// around the point into its own piece of LDS, every tap's column and row clamped before it becomes an address, and each lane forms
// I, gx, gy of its window pixels (pixel lane + 64 m, at most nine) and keeps them in registers.  Per iteration it brings the
// (2R + 2)^2 bytes of B around c + d into the same piece of LDS, forms e and its two partial sums in int32 (9 * 8160^2 < 2^31);
// the cross-lane sum -- four steps across a row of 16 lanes in the vector unit, the four rows through scalar registers, low and
// high halves apart so that nothing overflows -- is exact and uniform, and the float64 solve runs in all lanes alike.  The step
// goes through readfirstlane, so the loops stay uniform.  The waves of a block never wait for one another inside the point loop:
// LDS is private to a wave there and ordered by wave-scope fences.
//
// The counts of d_stats are gathered per block in LDS (one 64-bit LDS atomic per wave, pair and counter) and leave in one global
// atomic per block and non-zero counter.  Every store is plain C++.
#include <math.h>
#include <string.h>

#include "ofx_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxR = 11;
constexpr int kMaxFrames = OFX_STREAM_MAX_BATCH + 1;
constexpr int kStats = 7;
constexpr unsigned kMaxBlocks = 8192; // beyond this a block's waves take their points in turn

struct KltArgs {
    const uint8_t *plane[kMaxFrames][OFX_TRACK_MAX_LEVELS];
    int pitch[OFX_TRACK_MAX_LEVELS];
    int w, h, levels, pairs, pair0;
    int max_iters, eps_q, max_sad;
    double min_lambda;
    float *points;
    int32_t *status;
    float *history;
    int32_t *sad;
    unsigned long long *stats;
    unsigned n_points;
};

// the LDS of a wave is its own: what orders a wave's stores before its other lanes' loads is the order of its own instructions
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum of 16 lanes (a row), left in each of them: four steps across the row in the vector unit, no LDS
__device__ __forceinline__ int row_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);  // quad_perm [1, 0, 3, 2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);  // quad_perm [2, 3, 0, 1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false); // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false); // row_mirror
    return v;
}
__device__ __forceinline__ int rows_sum(int v)
{
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
// the sum of the 64 lanes' int32 partial sums, below 2^37 in magnitude, as the float64 the solve wants, the same in every lane: the
// low 16 bits and the rest are summed apart (a row's sum of either fits int32), the four rows meet in scalar registers, and
// hi * 2^16 + lo is exact in float64.  All 64 lanes are active wherever this is called (the loops are wave-uniform).
__device__ __forceinline__ double wave_sum(int p)
{
    const int lo = rows_sum(row_sum(p & 0xFFFF)), hi = rows_sum(row_sum(p >> 16));
    return (double)hi * 65536.0 + (double)lo;
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// P x P bytes of a plane with the corner (ox, oy), every column and row clamped to the plane
template <int P> __device__ __forceinline__ void load_patch(uint8_t *lds, const uint8_t *plane, int pitch, int wk, int hk, int ox, int oy, int lane)
{
    constexpr int N = (P * P + 63) / 64;
    uint8_t v[N];
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int idx = min(lane + 64 * m, P * P - 1);
        const int r = idx / P, c = idx - r * P;
        const int x = min(max(ox + c, 0), wk - 1), y = min(max(oy + r, 0), hk - 1);
        v[m] = plane[(size_t)y * (size_t)pitch + (size_t)x];
    }
#pragma unroll
    for (int m = 0; m < N; ++m)
        if (lane + 64 * m < P * P) lds[lane + 64 * m] = v[m];
}

struct Weights {
    int w00, w10, w01, w11;
};
__device__ __forceinline__ Weights weights(int a, int b) { return Weights{(32 - a) * (32 - b), a * (32 - b), (32 - a) * b, a * b}; }

// SAMPLE of the definition on a patch: the tap (row, col) and its three neighbours
template <int P> __device__ __forceinline__ int sample(const uint8_t *lds, int row, int col, const Weights &k)
{
    const uint8_t *q = lds + row * P + col;
    const int s = __mul24(k.w00, (int)q[0]) + __mul24(k.w10, (int)q[1]) + __mul24(k.w01, (int)q[P]) + __mul24(k.w11, (int)q[P + 1]);
    return (s + 16) >> 5;
}

template <int R> __global__ __launch_bounds__(kThreads) void klt_kernel(const KltArgs A)
{
    constexpr int W = 2 * R + 1, NP = W * W, M = (NP + 63) / 64, PA = 2 * R + 4, PB = 2 * R + 2;
    __shared__ uint8_t patch[kWaves][(PA * PA + 15) & ~15];
    __shared__ unsigned long long counts[OFX_STREAM_MAX_BATCH * kStats];

    const int t = (int)threadIdx.x, lane = t & 63, wave = uniform(t >> 6);
    uint8_t *lds = patch[wave];
    const bool want_stats = A.stats != nullptr;
    if (want_stats) {
        if (t < A.pairs * kStats) counts[t] = 0ull;
        __syncthreads();
    }
    // this lane's window pixels: (wi[m], wj[m]) in 0 .. 2R, pixel lane + 64 m (beyond the window: pixel 0, weight 0)
    int wi[M], wj[M];
    bool in[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int idx = lane + 64 * m;
        in[m] = idx < NP;
        const int id = in[m] ? idx : 0;
        wj[m] = id / W, wi[m] = id - wj[m] * W;
    }
    const int w = A.w, h = A.h, levels = A.levels;
    const float fw = (float)(w - 1), fh = (float)(h - 1);

    for (unsigned pt = blockIdx.x * kWaves + (unsigned)wave; pt < A.n_points; pt += gridDim.x * kWaves) {
        float x = __builtin_bit_cast(float, uniform(__builtin_bit_cast(int, A.points[2 * (size_t)pt])));
        float y = __builtin_bit_cast(float, uniform(__builtin_bit_cast(int, A.points[2 * (size_t)pt + 1])));
        const int st0 = uniform(A.status[pt]);
        int st = st0;
        for (int b = 0; b < A.pairs; ++b) {
            int sad_out = -1;
            if (st == 0) {
                int reason = 0, n_iters = 0;
                if (!(x >= 0.0f && x <= fw && y >= 0.0f && y <= fh)) { // (a NaN fails every comparison)
                    reason = OFX_TRACK_START;
                } else {
                    int dx = 0, dy = 0, cx = 0, cy = 0;
                    int I[M], gx[M], gy[M];
                    for (int k = levels - 1; k >= 0; --k) {
                        if (k != levels - 1) dx *= 2, dy *= 2;
                        const int wk = w >> k, hk = h >> k, pitch = A.pitch[k];
                        const uint8_t *pa = A.plane[b][k], *pb = A.plane[b + 1][k];
                        cx = uniform((int)lrintf(ldexpf(x, 5 - k))), cy = uniform((int)lrintf(ldexpf(y, 5 - k)));
                        // the template and its derivatives
                        wave_sync(); // (the patch of the level before is read)
                        load_patch<PA>(lds, pa, pitch, wk, hk, (cx >> 5) - R - 1, (cy >> 5) - R - 1, lane);
                        wave_sync();
                        const Weights ka = weights(cx & 31, cy & 31);
                        int pxx = 0, pyy = 0, pxy = 0;
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            const int r = wj[m] + 1, c = wi[m] + 1;
                            I[m] = sample<PA>(lds, r, c, ka);
                            const int vx = sample<PA>(lds, r, c + 1, ka) - sample<PA>(lds, r, c - 1, ka);
                            const int vy = sample<PA>(lds, r + 1, c, ka) - sample<PA>(lds, r - 1, c, ka);
                            gx[m] = in[m] ? vx : 0, gy[m] = in[m] ? vy : 0;
                            pxx += __mul24(gx[m], gx[m]), pyy += __mul24(gy[m], gy[m]), pxy += __mul24(gx[m], gy[m]);
                        }
                        const double gxx = wave_sum(pxx), gyy = wave_sum(pyy), gxy = wave_sum(pxy);
                        // (the build has -ffp-contract=off: nothing below fuses)
                        const double g1 = gxx * gyy, g2 = gxy * gxy;
                        const double D = g1 - g2;
                        const double tr = gxx + gyy, df = gxx - gyy;
                        const double q = df * df, p2 = gxy * gxy;
                        const double p4 = 4.0 * p2;
                        const double rr = q + p4;
                        const double lam = 0.5 * (tr - __dsqrt_rn(rr));
                        if (uniform(!(D > 0.0) || !(lam > A.min_lambda))) {
                            if (k == 0) reason = OFX_TRACK_SINGULAR;
                            continue;
                        }
                        for (int it = 0; it < A.max_iters; ++it) {
                            const int qx = cx + dx, qy = cy + dy;
                            wave_sync();
                            load_patch<PB>(lds, pb, pitch, wk, hk, (qx >> 5) - R, (qy >> 5) - R, lane);
                            wave_sync();
                            const Weights kb = weights(qx & 31, qy & 31);
                            int px = 0, py = 0;
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                const int e = sample<PB>(lds, wj[m], wi[m], kb) - I[m];
                                px += __mul24(gx[m], e), py += __mul24(gy[m], e);
                            }
                            const double bx = wave_sum(px), by = wave_sum(py);
                            const double n1 = gyy * bx, n2 = gxy * by, n3 = gxx * by, n4 = gxy * bx;
                            const double ux = n1 - n2, uy = n3 - n4;
                            const double sx = -64.0 * __ddiv_rn(ux, D), sy = -64.0 * __ddiv_rn(uy, D);
                            const int tx = uniform((int)rint(fmin(fmax(sx, -2048.0), 2048.0)));
                            const int ty = uniform((int)rint(fmin(fmax(sy, -2048.0), 2048.0)));
                            dx += tx, dy += ty;
                            ++n_iters;
                            if (abs(tx) <= A.eps_q && abs(ty) <= A.eps_q) break;
                        }
                    }
                    if (reason == 0) {
                        const int qx = cx + dx, qy = cy + dy;
                        if (qx < 0 || qx > 32 * (w - 1) || qy < 0 || qy > 32 * (h - 1)) {
                            reason = OFX_TRACK_OUT;
                        } else {
                            wave_sync();
                            load_patch<PB>(lds, A.plane[b + 1][0], A.pitch[0], w, h, (qx >> 5) - R, (qy >> 5) - R, lane);
                            wave_sync();
                            const Weights kb = weights(qx & 31, qy & 31);
                            int ps = 0;
#pragma unroll
                            for (int m = 0; m < M; ++m) ps += in[m] ? abs(sample<PB>(lds, wj[m], wi[m], kb) - I[m]) : 0;
                            const int sad = rows_sum(row_sum(ps));
                            if (A.max_sad > 0 && sad > A.max_sad) {
                                reason = OFX_TRACK_RESIDUAL;
                            } else {
                                sad_out = sad;
                                x = (float)qx / 32.0f, y = (float)qy / 32.0f;
                            }
                        }
                    }
                }
                if (reason) st = ((A.pair0 + b) << 8) | reason;
                if (want_stats && lane == 0) {
                    unsigned long long *cnt = counts + b * kStats;
                    if (reason) {
                        atomicAdd(&cnt[reason], 1ull);
                    } else {
                        atomicAdd(&cnt[0], 1ull);
                        atomicAdd(&cnt[6], (unsigned long long)sad_out);
                    }
                    if (n_iters) atomicAdd(&cnt[5], (unsigned long long)n_iters);
                }
            }
            if (lane == 0) {
                if (A.history) reinterpret_cast<float2 *>(A.history)[(size_t)b * A.n_points + pt] = make_float2(x, y);
                if (A.sad) A.sad[(size_t)b * A.n_points + pt] = sad_out;
            }
        }
        if (st0 == 0 && lane == 0) {
            reinterpret_cast<float2 *>(A.points)[pt] = make_float2(x, y);
            if (st != 0) A.status[pt] = st;
        }
    }
    if (!want_stats) return;
    __syncthreads();
    if (t < A.pairs * kStats && counts[t]) atomicAdd(&A.stats[t], counts[t]); // (zeroed on the stream before the launch)
}

template <int R> int launch(const KltArgs &A, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL(klt_kernel<R>, dim3(blocks), dim3(kThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

} // namespace

extern "C" int ofx_track_points(const ofx_track_clip *clip, const ofx_track_params *prm, int pair0, float *d_points, int32_t *d_status, int n_points,
                                float *d_history, int32_t *d_sad, int64_t *d_stats, void *stream)
{
    const char *who = "ofx_track_points";
    OFX_REQUIRE(clip != nullptr, "%s: clip is null", who);
    OFX_REQUIRE(prm != nullptr, "%s: prm is null", who);
    OFX_REQUIRE(clip->planes != nullptr && clip->pitches != nullptr, "%s: clip->planes or clip->pitches is null", who);
    OFX_REQUIRE(d_points != nullptr && d_status != nullptr, "%s: d_points or d_status is null", who);
    const int w = clip->w, h = clip->h, levels = clip->levels, frames = clip->n_frames;
    OFX_REQUIRE(levels >= 1 && levels <= OFX_TRACK_MAX_LEVELS, "%s: levels = %d is not in 1 .. %d", who, levels, OFX_TRACK_MAX_LEVELS);
    OFX_REQUIRE(w > 0 && h > 0 && (w >> (levels - 1)) >= 1 && (h >> (levels - 1)) >= 1,
                "%s: %d levels of %d x %d: the coarsest level has width or height 0", who, levels, w, h);
    OFX_REQUIRE(w <= (1 << 19) && h <= (1 << 19), "%s: the size %d x %d is above 2^19 (positions on the 1/32 lattice must be exact in float32)", who, w, h);
    OFX_REQUIRE(frames >= 2 && frames <= kMaxFrames, "%s: n_frames = %d is not in 2 .. %d", who, frames, kMaxFrames);
    OFX_REQUIRE((prm->window & 1) == 1 && prm->window >= 3 && prm->window <= 2 * kMaxR + 1, "%s: the window %d is not odd and in 3 .. %d", who, prm->window,
                2 * kMaxR + 1);
    OFX_REQUIRE(prm->max_iters >= 1 && prm->max_iters <= 32, "%s: max_iters = %d is not in 1 .. 32", who, prm->max_iters);
    OFX_REQUIRE(prm->eps_q >= 0, "%s: eps_q = %d is negative", who, prm->eps_q);
    OFX_REQUIRE(__builtin_isfinite(prm->min_lambda) && prm->min_lambda >= 0.0f, "%s: min_lambda must be finite and not negative", who);
    OFX_REQUIRE(prm->max_sad >= 0, "%s: max_sad = %d is negative", who, prm->max_sad);
    const int pairs = frames - 1;
    OFX_REQUIRE(pair0 >= 1 && (long long)pair0 + pairs < (1 << 23), "%s: pair0 = %d: pair0 must be >= 1 and pair0 + pairs below 2^23", who, pair0);
    OFX_REQUIRE(n_points >= 1, "%s: n_points = %d is not positive", who, n_points);
    static thread_local KltArgs A;
    memset(&A, 0, sizeof A);
    for (int k = 0; k < levels; ++k) {
        const int wk = w >> k, hk = h >> k, pitch = clip->pitches[k];
        OFX_REQUIRE(pitch >= wk, "%s: level %d: the pitch %d is below the width %d", who, k, pitch, wk);
        OFX_REQUIRE((size_t)hk * (size_t)pitch < ((size_t)1 << 31), "%s: level %d: the pitch %d makes a plane of 2^31 bytes or more", who, k, pitch);
        A.pitch[k] = pitch;
        for (int f = 0; f < frames; ++f) {
            const uint8_t *p = clip->planes[(size_t)f * levels + k];
            OFX_REQUIRE(p != nullptr, "%s: the plane of frame %d, level %d is null", who, f, k);
            A.plane[f][k] = p;
        }
    }
    OFX_REQUIRE(((uintptr_t)d_points & 7) == 0 && ((uintptr_t)d_history & 7) == 0, "%s: d_points and d_history must be 8-byte aligned", who);
    OFX_REQUIRE(((uintptr_t)d_status & 3) == 0 && ((uintptr_t)d_sad & 3) == 0, "%s: d_status and d_sad must be 4-byte aligned", who);
    OFX_REQUIRE(((uintptr_t)d_stats & 7) == 0, "%s: d_stats must be 8-byte aligned", who);
    A.w = w, A.h = h, A.levels = levels, A.pairs = pairs, A.pair0 = pair0;
    A.max_iters = prm->max_iters, A.eps_q = prm->eps_q, A.max_sad = prm->max_sad, A.min_lambda = (double)prm->min_lambda;
    A.points = d_points, A.status = d_status, A.history = d_history, A.sad = d_sad, A.stats = reinterpret_cast<unsigned long long *>(d_stats);
    A.n_points = (unsigned)n_points;
    hipStream_t st = ofx_stream(stream);
    if (d_stats) OFX_TRY(ofx_zero_words(d_stats, (size_t)pairs * kStats, st));
    const unsigned need = ((unsigned)n_points + kWaves - 1) / kWaves, blocks = need < kMaxBlocks ? need : kMaxBlocks;
    switch (prm->window >> 1) {
    case 1: return launch<1>(A, blocks, st);
    case 2: return launch<2>(A, blocks, st);
    case 3: return launch<3>(A, blocks, st);
    case 4: return launch<4>(A, blocks, st);
    case 5: return launch<5>(A, blocks, st);
    case 6: return launch<6>(A, blocks, st);
    case 7: return launch<7>(A, blocks, st);
    case 8: return launch<8>(A, blocks, st);
    case 9: return launch<9>(A, blocks, st);
    case 10: return launch<10>(A, blocks, st);
    default: return launch<11>(A, blocks, st);
    }
}
