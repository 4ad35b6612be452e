// Frame mosaic (the definition: "frame mosaic" in include/ofx.h): up to OFX_MOSAIC_MAX_SOURCES u8 sources of 1 or 3 interleaved
// channels, each seen through a float64 [9] inverse homography of its own, looked through in priority order; an output pixel shows
// the first source that COVERS it (a defined position in range), and `which` names that source.  The position is
// warp_persp.hip's (three float64 dot products, ONE reciprocal, two products, each rounded once: the build has -ffp-contract=off),
// the value warp_pixel.h's bilinear sum on the 1/32 px lattice, restated here per pixel, so a mosaic of one source is
// ofx_warp_perspective's bytes.  ONE launch for up to OFX_STREAM_MAX_BATCH items of any sizes: a lane makes four adjacent output
// pixels of a row, every tap clamped before it becomes an address, dword stores where the address allows and the quad is whole.
// The source loop leaves as soon as NO lane of the wave holds an unresolved pixel (a ballot, so the exit is wave-uniform): the
// interior of a stabilised frame, which source 0 covers, evaluates one source per pixel, and only the waves at the border pay for
// the neighbours.  Lanes beyond an item's last quad stay in the wave, with nothing to resolve, until the loop and the counts are
// done.  The counts of the entries 1 .. 9 are formed per wave (popcounts of ballots), summed per block in LDS, and leave as one
// integer atomic per non-zero entry and block; entry 0 is w h less the others (see the kernel), so a block that source 0 covers
// sends no atomic at all.
#include <math.h>
#include <string.h>

#include "ofx_internal.h"
#include "warp_pixel.h"

namespace {

constexpr int kThreads = 256, kQuad = kWarpQuad;
constexpr int kMaxSize = 1 << 16;
constexpr double kMaxPos = 1099511627776.0; // 2^40: a position beyond it, in 1/32 px, is UNDEFINED
constexpr int kBins = OFX_MOSAIC_MAX_SOURCES + 1;
constexpr unsigned kNone = 255u;

struct MosaicSrc {
    const uint8_t *src;
    double m[9];
    int src_pitch, sw, sh, pad;
};
struct MosaicHead {
    uint8_t *dst, *which;
    unsigned long long *counts;
    int dst_pitch, which_pitch, w, h, channels, border, fill, n_sources;
    unsigned quads_per_row, quads;
};
// The table travels by value in the kernel arguments, and the host writes every byte of it per launch: a call gets the smallest
// of the nine tables (1, 4 or 16 items of 1, 5 or 9 sources: 160 B .. 14.5 KB) that holds it.
template <int SCAP> struct MosaicItem {
    MosaicHead h;
    MosaicSrc s[SCAP];
};
template <int N, int SCAP> struct MosaicArgs {
    MosaicItem<SCAP> item[N];
};
using MosaicTable = MosaicArgs<OFX_STREAM_MAX_BATCH, OFX_MOSAIC_MAX_SOURCES>;

// POSITION and UNDEFINED of "perspective frame warp" for output pixel (x, y) through m; (0, 0) where undefined
__device__ __forceinline__ bool mosaic_position(const double *m, int x, double yd, long long &qx, long long &qy)
{
    const double xd = (double)x;
    const double X = (m[0] * xd + m[1] * yd) + m[2], Y = (m[3] * xd + m[4] * yd) + m[5], W = (m[6] * xd + m[7] * yd) + m[8];
    const double r = 1.0 / W;
    const double fx = (X * r) * 32.0, fy = (Y * r) * 32.0;
    const bool defined = W > 0.0 && fabs(fx) <= kMaxPos && fabs(fy) <= kMaxPos; // (false for a NaN or an infinity)
    qx = defined ? __double2ll_rn(fx) : 0ll, qy = defined ? __double2ll_rn(fy) : 0ll;
    return defined;
}

// the quad of lane g (live: it lies in the item); bins: the block's counts in LDS, or nullptr
template <int C> __device__ __forceinline__ void mosaic_quad(const MosaicHead &it, const MosaicSrc *srcs, unsigned g, bool live, unsigned *bins)
{
    const int y = (int)(g / it.quads_per_row), x0 = kQuad * (int)(g - (unsigned)y * it.quads_per_row);
    const double yd = (double)y;
    const bool constant = it.border == OFX_BORDER_CONSTANT;
    const bool lead = (threadIdx.x & 63) == 0;
    unsigned open = 0; // bit j: pixel x0 + j lies in the row and no source covers it yet
#pragma unroll
    for (int j = 0; j < kQuad; ++j) open |= (live && x0 + j < it.w) ? 1u << j : 0u;
    uint8_t v[kQuad][C];
    unsigned which = kNone | kNone << 8 | kNone << 16 | kNone << 24;
#pragma unroll
    for (int j = 0; j < kQuad; ++j)
#pragma unroll
        for (int ch = 0; ch < C; ++ch) v[j][ch] = (uint8_t)it.fill;
    for (int k = 0; k < it.n_sources; ++k) {
        if (__ballot(open != 0u) == 0ull) break; // (wave-uniform)
        const MosaicSrc &s = srcs[k];
        const int xmax = 32 * (s.sw - 1), ymax = 32 * (s.sh - 1);
        unsigned taken = 0;
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
            if (open & (1u << j)) {
                long long qx, qy;
                const bool defined = mosaic_position(s.m, x0 + j, yd, qx, qy);
                const bool in = defined && qx >= 0 && qx <= xmax && qy >= 0 && qy <= ymax;
                // source 0's value stays as the fallback of a pixel that nothing covers
                if (in || (k == 0 && defined && !constant)) {
                    const int cx = (int)(qx < 0 ? 0 : qx > xmax ? xmax : qx), cy = (int)(qy < 0 ? 0 : qy > ymax ? ymax : qy); // (clamped: in 0 .. 32 (size - 1))
                    const int ix = cx >> 5, fa = cx & 31, iy = cy >> 5, fb = cy & 31;
                    const int ix1 = ix + 1 < s.sw ? ix + 1 : s.sw - 1, iy1 = iy + 1 < s.sh ? iy + 1 : s.sh - 1;
                    const uint8_t *r0 = s.src + (size_t)iy * (size_t)s.src_pitch, *r1 = s.src + (size_t)iy1 * (size_t)s.src_pitch;
                    const int w00 = (32 - fa) * (32 - fb), w10 = fa * (32 - fb), w01 = (32 - fa) * fb, w11 = fa * fb;
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        const int sum = w00 * r0[C * ix + ch] + w10 * r0[C * ix1 + ch] + w01 * r1[C * ix + ch] + w11 * r1[C * ix1 + ch];
                        v[j][ch] = (uint8_t)((sum + 512) >> 10);
                    }
                }
                if (in) {
                    which = (which & ~(0xFFu << (8 * j))) | ((unsigned)k << (8 * j));
                    taken |= 1u << j;
                }
            }
        }
        open &= ~taken;
        if (bins != nullptr && k != 0) { // (block-uniform; entry 0 is what the other entries leave of w h: see the kernel)
            unsigned n = 0;
#pragma unroll
            for (int j = 0; j < kQuad; ++j) n += (unsigned)__popcll(__ballot((taken >> j) & 1u));
            if (lead && n) atomicAdd(&bins[k], n);
        }
    }
    if (bins != nullptr) {
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < kQuad; ++j) n += (unsigned)__popcll(__ballot((open >> j) & 1u));
        if (lead && n) atomicAdd(&bins[kBins - 1], n);
    }
    if (!live) return;
    const bool whole = x0 + kQuad <= it.w;
    uint8_t *d = it.dst + (size_t)y * (size_t)it.dst_pitch + (size_t)(C * x0);
    if (whole && ((uintptr_t)d & 3) == 0) {
        const uint8_t *b = &v[0][0];
#pragma unroll
        for (int k = 0; k < C; ++k)
            reinterpret_cast<uint32_t *>(d)[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < kQuad; ++j)
            if (x0 + j < it.w) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) d[C * j + ch] = v[j][ch];
            }
    }
    if (it.which == nullptr) return;
    uint8_t *q = it.which + (size_t)y * (size_t)it.which_pitch + (size_t)x0;
    if (whole && ((uintptr_t)q & 3) == 0) {
        *reinterpret_cast<uint32_t *>(q) = which;
    } else {
#pragma unroll
        for (int j = 0; j < kQuad; ++j)
            if (x0 + j < it.w) q[j] = (uint8_t)(which >> (8 * j));
    }
}

// Entry 0 of the counts is NOT summed from the blocks: in the interior of a frame every block would add to that one address, and
// the atomics of a 4K frame's 8100 blocks, one behind the other, take longer than the frame.  Block 0 adds w h to it, and every
// block takes off the pixels that it gave to another entry -- modulo 2^64, in any order -- so a block of the interior sends nothing.
template <int N, int SCAP> __global__ __launch_bounds__(kThreads) void warp_mosaic_kernel(const MosaicArgs<N, SCAP> A)
{
    const MosaicHead &it = A.item[blockIdx.y].h;
    const MosaicSrc *srcs = A.item[blockIdx.y].s;
    const unsigned base = blockIdx.x * kThreads;
    if (base >= it.quads) return; // (block-uniform: the grid is sized for the launch's largest item)
    __shared__ unsigned block_bins[kBins];
    unsigned *bins = it.counts != nullptr ? block_bins : nullptr;
    if (bins != nullptr) {
        if (threadIdx.x < kBins) block_bins[threadIdx.x] = 0u;
        __syncthreads();
    }
    const unsigned g = base + threadIdx.x;
    const bool live = g < it.quads; // (a lane beyond the last quad stays for the ballots, with no pixel of its own)
    if (it.channels == 3)
        mosaic_quad<3>(it, srcs, live ? g : 0u, live, bins);
    else
        mosaic_quad<1>(it, srcs, live ? g : 0u, live, bins);
    if (bins == nullptr) return;
    __syncthreads();
    // (the counts were zeroed on the stream before the launch)
    if (threadIdx.x >= 1 && threadIdx.x < kBins && block_bins[threadIdx.x]) atomicAdd(&it.counts[threadIdx.x], (unsigned long long)block_bins[threadIdx.x]);
    if (threadIdx.x == 0) {
        unsigned long long delta = blockIdx.x == 0 ? (unsigned long long)it.w * (unsigned long long)it.h : 0ull;
#pragma unroll
        for (int k = 1; k < kBins; ++k) delta -= (unsigned long long)block_bins[k];
        if (delta) atomicAdd(&it.counts[0], delta);
    }
}

template <int N, int SCAP> void launch(const MosaicTable &T, int n, unsigned max_quads, hipStream_t st)
{
    static thread_local MosaicArgs<N, SCAP> A;
    for (int i = 0; i < n; ++i) {
        A.item[i].h = T.item[i].h;
        for (int k = 0; k < SCAP; ++k) A.item[i].s[k] = T.item[i].s[k];
    }
    hipLaunchKernelGGL((warp_mosaic_kernel<N, SCAP>), dim3((max_quads + kThreads - 1) / kThreads, n), dim3(kThreads), 0, st, A);
}
template <int N> void launch_for(const MosaicTable &T, int n, int max_sources, unsigned max_quads, hipStream_t st)
{
    if (max_sources <= 1)
        launch<N, 1>(T, n, max_quads, st);
    else if (max_sources <= 5)
        launch<N, 5>(T, n, max_quads, st);
    else
        launch<N, OFX_MOSAIC_MAX_SOURCES>(T, n, max_quads, st);
}

struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const void *p, int rows, int pitch, int row_bytes) { return {(uintptr_t)p, (uintptr_t)p + (size_t)(rows - 1) * (size_t)pitch + (size_t)row_bytes}; }
inline bool apart(Span a, Span b) { return a.hi <= b.lo || b.hi <= a.lo; }

} // namespace

extern "C" int ofx_warp_mosaic(const ofx_mosaic_desc *items, int n, void *stream)
{
    const char *who = "ofx_warp_mosaic";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    static thread_local MosaicTable A;
    memset(&A, 0, sizeof A);
    unsigned max_quads = 0;
    int max_sources = 0;
    for (int i = 0; i < n; ++i) {
        const ofx_mosaic_desc &d = items[i];
        OFX_REQUIRE(d.n_sources >= 1 && d.n_sources <= OFX_MOSAIC_MAX_SOURCES, "%s: item %d: n_sources = %d is not in 1 .. %d", who, i, d.n_sources,
                    OFX_MOSAIC_MAX_SOURCES);
        OFX_REQUIRE(d.d_dst != nullptr, "%s: item %d: d_dst is null", who, i);
        OFX_REQUIRE(d.channels == 1 || d.channels == 3, "%s: item %d: channels = %d is not 1 or 3", who, i, d.channels);
        OFX_REQUIRE(d.border == OFX_BORDER_CONSTANT || d.border == OFX_BORDER_REPLICATE, "%s: item %d: border = %d is not 0 or 1", who, i, d.border);
        OFX_REQUIRE(d.fill >= 0 && d.fill <= 255, "%s: item %d: fill = %d is not in 0 .. 255", who, i, d.fill);
        OFX_REQUIRE(d.w >= 1 && d.w <= kMaxSize && d.h >= 1 && d.h <= kMaxSize, "%s: item %d: the size %d x %d is not in 1 .. 2^16", who, i, d.w, d.h);
        OFX_REQUIRE(d.dst_pitch >= d.channels * d.w, "%s: item %d: dst_pitch = %d is below %d", who, i, d.dst_pitch, d.channels * d.w);
        const Span dst = span_of(d.d_dst, d.h, d.dst_pitch, d.channels * d.w);
        Span which = {0, 0};
        if (d.d_which != nullptr) {
            OFX_REQUIRE(d.which_pitch >= d.w, "%s: item %d: which_pitch = %d is below %d", who, i, d.which_pitch, d.w);
            which = span_of(d.d_which, d.h, d.which_pitch, d.w);
            OFX_REQUIRE(apart(which, dst), "%s: item %d: d_which and d_dst overlap", who, i);
        }
        MosaicHead &it = A.item[i].h;
        for (int k = 0; k < d.n_sources; ++k) {
            const ofx_mosaic_source &s = d.source[k];
            OFX_REQUIRE(s.d_src != nullptr, "%s: item %d: source %d: d_src is null", who, i, k);
            OFX_REQUIRE(s.sw >= 1 && s.sw <= kMaxSize && s.sh >= 1 && s.sh <= kMaxSize, "%s: item %d: source %d: the source size %d x %d is not in 1 .. 2^16", who,
                        i, k, s.sw, s.sh);
            OFX_REQUIRE(s.src_pitch >= d.channels * s.sw, "%s: item %d: source %d: src_pitch = %d is below %d", who, i, k, s.src_pitch, d.channels * s.sw);
            for (int e = 0; e < 9; ++e) {
                const double lim = (e == 2 || e == 5) ? 1048576.0 : (e == 6 || e == 7) ? 1.0 : 16.0;
                OFX_REQUIRE(__builtin_isfinite(s.model[e]) && fabs(s.model[e]) <= lim, "%s: item %d: source %d: model[%d] is not finite or above %s in magnitude",
                            who, i, k, e, lim == 16.0 ? "16" : lim == 1.0 ? "1" : "2^20");
            }
            const Span src = span_of(s.d_src, s.sh, s.src_pitch, d.channels * s.sw);
            OFX_REQUIRE(apart(src, dst), "%s: item %d: source %d: d_src and d_dst overlap", who, i, k);
            OFX_REQUIRE(d.d_which == nullptr || apart(src, which), "%s: item %d: source %d: d_src and d_which overlap", who, i, k);
            MosaicSrc &o = A.item[i].s[k];
            o.src = s.d_src, o.src_pitch = s.src_pitch, o.sw = s.sw, o.sh = s.sh;
            for (int e = 0; e < 9; ++e) o.m[e] = s.model[e];
        }
        OFX_REQUIRE(((uintptr_t)d.d_counts & 7) == 0, "%s: item %d: d_counts must be 8-byte aligned", who, i);
        it.dst = d.d_dst, it.which = d.d_which, it.counts = reinterpret_cast<unsigned long long *>(d.d_counts);
        it.dst_pitch = d.dst_pitch, it.which_pitch = d.which_pitch, it.w = d.w, it.h = d.h;
        it.channels = d.channels, it.border = d.border, it.fill = d.fill, it.n_sources = d.n_sources;
        it.quads_per_row = (unsigned)ofx_div_up(d.w, kQuad);
        it.quads = it.quads_per_row * (unsigned)d.h; // (at most 2^14 * 2^16)
        max_quads = it.quads > max_quads ? it.quads : max_quads;
        max_sources = d.n_sources > max_sources ? d.n_sources : max_sources;
    }
    hipStream_t st = ofx_stream(stream);
    for (int i = 0; i < n; ++i)
        if (items[i].d_counts) OFX_TRY(ofx_zero_words(items[i].d_counts, kBins, st));
    if (n == 1)
        launch_for<1>(A, n, max_sources, max_quads, st);
    else if (n <= 4)
        launch_for<4>(A, n, max_sources, max_quads, st);
    else
        launch_for<OFX_STREAM_MAX_BATCH>(A, n, max_sources, max_quads, st);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
