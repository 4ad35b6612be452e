// Temporal noise filter (the definition: "temporal noise filter" in include/ofx.h): a u8 centre plane of 1 or 3 interleaved channels
// averaged with up to OFX_TEMPORAL_MAX_NEIGHBOURS neighbour planes, each fetched along a displacement field of its own on the 1/32 px
// lattice and weighted per pixel by the rounded mean absolute difference of its 3 x 3 patch against the centre's (the patch test).
// ONE launch for up to OFX_STREAM_MAX_BATCH items of any sizes: a lane makes four adjacent output pixels of a row (warp_pixel.h's
// quad and its store: dwords where the address allows and the quad is whole, bytes otherwise).
//   centre patch  three rows of the quad's 6 (18) bytes, once per quad: one unaligned block per row where the six columns lie in
//                 the row, clamped bytes otherwise.
//   taps          per neighbour and pixel a 4 x 4 block T of taps around (ix, iy) = (qx >> 5, qy >> 5), columns ix - 1 .. ix + 2 and
//                 rows iy - 1 .. iy + 2, each CLAMPED to the plane.  The nine patch values are the bilinear sums of its nine 2 x 2
//                 sub-blocks with the ONE fraction (fa, fb) of the centre position.  Where a patch position is clamped by the
//                 definition (to 0 or 32 (size - 1), fraction 0), both taps of the sub-block along that axis are the same clamped
//                 pixel, and (32 - f) P + f P = 32 P is the definition's integer: the block with clamped taps IS the definition, so
//                 the two tap paths differ in their loads only.  Interior (the block lies in the plane): one (three) unaligned
//                 dword load(s) per row.  Border: every tap clamped before it becomes an address.  The choice is per lane and pixel.
//                 A position that is not usable is replaced by (0, 0) before the taps and gets weight 0.
//   bilinear      separable in integers: 12 C row sums (32 - fa) T + fa T', then 9 C column sums, + 512 >> 10: the same integer as
//                 VALUE of "affine frame warp", because nothing rounds before the shift.  The taps stay packed as loaded: a row sum
//                 is ONE v_dot4_u32_u8 on the four bytes from a tap on, the weights at bytes 0 and C.  The values are packed into
//                 bytes as they are made and meet the centre's packed patch in v_sad_u8 (what that bought).
//   weights       the 256-entry table travels in the kernel arguments and is staged in LDS (512 B), indexed per lane by m_k.
//   division      out = (2 num + den) / (2 den) <= 255: q = (int)((float)n * rcp((float)d)) is off by at most one (n < 2^20 and
//                 d < 2^12 are exact floats, and the quotient's error is far below 1), and one exact integer remainder puts it right.
//   stats         per lane, summed per wave by shuffles, per block in LDS, and one 64-bit atomic per non-zero entry and block.
#include <math.h>
#include <string.h>

#include "ofx_internal.h"
#include "warp_pixel.h"

namespace {

constexpr int kThreads = 256, kQuad = kWarpQuad;
constexpr int kMaxSize = 1 << 16;
constexpr float kMaxDisp = 1048576.0f;
constexpr int kStats = 8;
constexpr int kBins = 5; // not usable k = 0, 1 (16 bits each) | k = 2, 3 | zero-weight pixels | sum |out - c| | sum of weights

struct TempNb {
    const uint8_t *plane;
    const float *field;
    int pitch, pad;
};
struct TempItem {
    const uint8_t *centre;
    uint8_t *dst;
    unsigned long long *stats;
    int centre_pitch, dst_pitch, w, h, channels, n_nb;
    unsigned quads_per_row, quads;
    TempNb nb[OFX_TEMPORAL_MAX_NEIGHBOURS];
};
// The table travels by value in the kernel arguments; a single item gets the small one (a 16-item table is 2.4 KB to write).
template <int N> struct TempArgs {
    TempItem item[N];
    uint32_t weights[128]; // uint16 [256]
    int wc, pad;
};
using TempTable = TempArgs<OFX_STREAM_MAX_BATCH>;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
    return v;
}

// byte i of packed words
__device__ __forceinline__ uint32_t byte_at(const uint32_t *p, int i) { return (p[i >> 2] >> (8 * (i & 3))) & 0xFFu; }
// the four bytes from byte i on of n packed words (zeros beyond them)
__device__ __forceinline__ uint32_t bytes_at(const uint32_t *p, int n, int i)
{
    const uint32_t lo = p[i >> 2], hi = (i >> 2) + 1 < n ? p[(i >> 2) + 1] : 0u;
    return (i & 3) ? __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(i & 3)) : lo;
}

// the quad g of the item; acc: the lane's five stats words (see kBins)
template <int C> __device__ __forceinline__ void temporal_quad(const TempItem &it, unsigned g, const uint16_t *wt, int wc, unsigned *acc)
{
    const int w = it.w, h = it.h;
    const int y = (int)(g / it.quads_per_row), x0 = kQuad * (int)(g - (unsigned)y * it.quads_per_row);
    const int xmax = 32 * (w - 1), ymax = 32 * (h - 1);
    const bool whole = x0 + kQuad <= w;

    // the centre's patch rows y - 1 .. y + 1, columns x0 - 1 .. x0 + 4, clamped: 6 C bytes per row, packed, zeros behind them
    constexpr int kCpWords = (6 * C + 3) / 4 + 1;
    uint32_t cp[3][kCpWords];
    const bool cp_inside = x0 >= 1 && x0 + kQuad <= w - 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint8_t *row = it.centre + (size_t)clampi(y + r - 1, 0, h - 1) * (size_t)it.centre_pitch;
#pragma unroll
        for (int d = 0; d < kCpWords; ++d) cp[r][d] = 0u;
        if (cp_inside) {
            __builtin_memcpy(cp[r], row + C * (x0 - 1), 6 * C);
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int xx = clampi(x0 - 1 + i, 0, w - 1);
#pragma unroll
                for (int ch = 0; ch < C; ++ch) cp[r][(C * i + ch) >> 2] |= (uint32_t)row[C * xx + ch] << (8 * ((C * i + ch) & 3));
            }
        }
    }
    // pixel j's patch row r, its 3 C bytes packed for v_sad_u8 (the bytes behind them zero, as in the neighbour's packed values)
    constexpr int kRowWords = (3 * C + 3) / 4;
    uint32_t cpw[kQuad][3][kRowWords];
#pragma unroll
    for (int j = 0; j < kQuad; ++j)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int d = 0; d < kRowWords; ++d) {
                const uint32_t v = bytes_at(cp[r], kCpWords, C * j + 4 * d);
                cpw[j][r][d] = 3 * C - 4 * d >= 4 ? v : v & (0xFFFFFFFFu >> (8 * (4 - (3 * C - 4 * d))));
            }
    int num[kQuad][C], den[kQuad];
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
        den[j] = wc;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) num[j][ch] = __mul24(wc, (int)byte_at(cp[1], C * (j + 1) + ch));
    }

    unsigned long long nu = 0; // pixels where neighbour k is not usable, 16 bits per k
    for (int k = 0; k < it.n_nb; ++k) { // (wave-uniform bound)
        const TempNb &nb = it.nb[k];
        const float *fp = nb.field + 2 * ((size_t)y * (size_t)w + (size_t)x0);
        float uv[2 * kQuad];
        if (whole && ((uintptr_t)fp & 15) == 0) {
            const float4 a = reinterpret_cast<const float4 *>(fp)[0], b = reinterpret_cast<const float4 *>(fp)[1];
            uv[0] = a.x, uv[1] = a.y, uv[2] = a.z, uv[3] = a.w, uv[4] = b.x, uv[5] = b.y, uv[6] = b.z, uv[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < kQuad; ++j) {
                float2 a = make_float2(0.0f, 0.0f);
                if (x0 + j < w) a = reinterpret_cast<const float2 *>(fp)[j];
                uv[2 * j] = a.x, uv[2 * j + 1] = a.y;
            }
        }
        unsigned unusable = 0;
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
            if (x0 + j >= w) continue;
            const float u = uv[2 * j], v = uv[2 * j + 1];
            const bool defined = fabsf(u) <= kMaxDisp && fabsf(v) <= kMaxDisp; // (false for a NaN or an infinity)
            // |32 u| <= 2^25: the sums fit 32 bits
            const int qx = 32 * (x0 + j) + (defined ? (int)rintf(32.0f * u) : 0), qy = 32 * y + (defined ? (int)rintf(32.0f * v) : 0);
            const bool usable = defined && qx >= 0 && qx <= xmax && qy >= 0 && qy <= ymax;
            unusable += usable ? 0u : 1u;
            const int cx = usable ? qx : 0, cy = usable ? qy : 0; // (in 0 .. 32 (size - 1) either way)
            const int ix = cx >> 5, fa = cx & 31, iy = cy >> 5, fb = cy & 31;
            uint32_t T[4][C + 1]; // rows iy - 1 .. iy + 2, the 4 C bytes of the columns ix - 1 .. ix + 2, and a zero word
            if (ix >= 1 && ix + 2 <= w - 1 && iy >= 1 && iy + 2 <= h - 1) {
                const uint8_t *p = nb.plane + (size_t)(iy - 1) * (size_t)nb.pitch + (size_t)(C * (ix - 1));
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    __builtin_memcpy(T[r], p + (size_t)r * (size_t)nb.pitch, 4 * C);
                    T[r][C] = 0u;
                }
            } else {
                int xs[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) xs[i] = C * clampi(ix - 1 + i, 0, w - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint8_t *row = nb.plane + (size_t)clampi(iy - 1 + r, 0, h - 1) * (size_t)nb.pitch;
#pragma unroll
                    for (int d = 0; d <= C; ++d) T[r][d] = 0u;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int ch = 0; ch < C; ++ch) T[r][(C * i + ch) >> 2] |= (uint32_t)row[xs[i] + ch] << (8 * ((C * i + ch) & 3));
                }
            }
            // row sums (32 - fa) T(e) + fa T(e + C): one v_dot4_u32_u8 on the four bytes from e on, the weights at bytes 0 and C
            const uint32_t wrow = (uint32_t)(32 - fa) | (uint32_t)fa << (8 * C);
            uint32_t H[4][3 * C];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int e = 0; e < 3 * C; ++e)
                    H[r][e] = C == 1 ? __builtin_amdgcn_udot4(T[r][0], wrow << (8 * e), 0u, false) : __builtin_amdgcn_udot4(bytes_at(T[r], C + 1, e), wrow, 0u, false);
            // column sums, rounded: the nine values per channel, packed like cpw for v_sad_u8
            const uint32_t fb0 = (uint32_t)(32 - fb), fb1 = (uint32_t)fb;
            uint32_t sad = 0u;
            int n0[C];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                uint32_t packed[kRowWords];
#pragma unroll
                for (int d = 0; d < kRowWords; ++d) packed[d] = 0u;
#pragma unroll
                for (int e = 0; e < 3 * C; ++e) {
                    const uint32_t val = (__umul24(fb0, H[r][e]) + __umul24(fb1, H[r + 1][e]) + 512u) >> 10; // (at most 255)
                    packed[e >> 2] |= val << (8 * (e & 3));
                    if (r == 1 && e >= C && e < 2 * C) n0[e - C] = (int)val;
                }
#pragma unroll
                for (int d = 0; d < kRowWords; ++d) sad = __builtin_amdgcn_sad_u8(packed[d], cpw[j][r][d], sad);
            }
            const uint32_t m = C == 1 ? (sad + 4u) / 9u : (sad + 13u) / 27u;
            const int wk = usable ? (int)wt[m < 255u ? m : 255u] : 0;
            den[j] += wk;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) num[j][ch] += __mul24(wk, n0[ch]);
        }
        nu += (unsigned long long)unusable << (16 * k);
    }
    acc[0] += (unsigned)nu, acc[1] += (unsigned)(nu >> 32);

    uint8_t out[kQuad][C];
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
        const int d = 2 * den[j];
        const float r = __builtin_amdgcn_rcpf((float)d);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const int n = 2 * num[j][ch] + den[j];
            int q = (int)((float)n * r); // (off by at most one)
            const int rem = n - __mul24(q, d);
            q += rem >= d ? 1 : rem < 0 ? -1 : 0;
            out[j][ch] = (uint8_t)q;
            if (x0 + j < w) {
                const int c = (int)byte_at(cp[1], C * (j + 1) + ch);
                acc[3] += (unsigned)(q < c ? c - q : q - c);
            }
        }
        if (x0 + j < w) {
            acc[2] += den[j] == wc ? 1u : 0u;
            acc[4] += (unsigned)(den[j] - wc);
        }
    }
    uint8_t *d = it.dst + (size_t)y * (size_t)it.dst_pitch + (size_t)(C * x0);
    if (whole && ((uintptr_t)d & 3) == 0) {
        const uint8_t *b = &out[0][0];
#pragma unroll
        for (int k = 0; k < C; ++k)
            reinterpret_cast<uint32_t *>(d)[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < kQuad; ++j)
            if (x0 + j < w) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) d[C * j + ch] = out[j][ch];
            }
    }
}

template <int N> __global__ __launch_bounds__(kThreads) void temporal_filter_kernel(const TempArgs<N> A)
{
    const TempItem &it = A.item[blockIdx.y];
    const unsigned base = blockIdx.x * kThreads;
    if (base >= it.quads) return; // (block-uniform: the grid is sized for the launch's largest item)
    __shared__ uint32_t wtab[128];
    __shared__ unsigned block_bins[kBins];
    if (threadIdx.x < 128) wtab[threadIdx.x] = A.weights[threadIdx.x];
    if (threadIdx.x < kBins) block_bins[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned g = base + threadIdx.x;
    unsigned acc[kBins] = {0u, 0u, 0u, 0u, 0u};
    if (g < it.quads) {
        if (it.channels == 3)
            temporal_quad<3>(it, g, reinterpret_cast<const uint16_t *>(wtab), A.wc, acc);
        else
            temporal_quad<1>(it, g, reinterpret_cast<const uint16_t *>(wtab), A.wc, acc);
    }
    if (it.stats == nullptr) return; // (block-uniform)
    // a wave's 16-bit fields hold at most 64 * 4, a block's 1024; sum |out - c| of a block is below 2^20, the weights' 2^21
#pragma unroll
    for (int e = 0; e < kBins; ++e) {
        const unsigned s = wave_sum(acc[e]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&block_bins[e], s);
    }
    __syncthreads();
    // (the stats were zeroed on the stream before the launch)
    if (threadIdx.x < kStats) {
        const int e = (int)threadIdx.x;
        unsigned long long v;
        if (e == 0)
            v = blockIdx.x == 0 ? (unsigned long long)it.w * (unsigned long long)it.h : 0ull;
        else if (e <= 4)
            v = (block_bins[(e - 1) >> 1] >> (16 * ((e - 1) & 1))) & 0xFFFFu;
        else
            v = block_bins[e - 3];
        if (v) atomicAdd(&it.stats[e], v);
    }
}

template <int N> void launch(const TempTable &T, int n, unsigned max_quads, hipStream_t st)
{
    static thread_local TempArgs<N> A;
    for (int i = 0; i < N; ++i) A.item[i] = T.item[i];
    memcpy(A.weights, T.weights, sizeof A.weights);
    A.wc = T.wc, A.pad = 0;
    hipLaunchKernelGGL((temporal_filter_kernel<N>), dim3((max_quads + kThreads - 1) / kThreads, n), dim3(kThreads), 0, st, A);
}

struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const void *p, int rows, int pitch, int row_bytes) { return {(uintptr_t)p, (uintptr_t)p + (size_t)(rows - 1) * (size_t)pitch + (size_t)row_bytes}; }
inline bool apart(Span a, Span b) { return a.hi <= b.lo || b.hi <= a.lo; }
inline bool plane_fits(int rows, int pitch, int row_bytes) { return (size_t)(rows - 1) * (size_t)pitch + (size_t)row_bytes < ((size_t)1 << 31); }

} // namespace

extern "C" int ofx_temporal_filter(const ofx_temporal_desc *items, int n, const ofx_temporal_params *prm, void *stream)
{
    const char *who = "ofx_temporal_filter";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_REQUIRE(prm != nullptr, "%s: prm is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    for (int e = 0; e < 256; ++e) OFX_REQUIRE(prm->weights[e] <= 256, "%s: weights[%d] = %d is above 256", who, e, (int)prm->weights[e]);
    OFX_REQUIRE(prm->centre_weight >= 1 && prm->centre_weight <= 256, "%s: centre_weight = %d is not in 1 .. 256", who, prm->centre_weight);
    OFX_REQUIRE(prm->reserved == 0, "%s: reserved = %d is not 0", who, prm->reserved);
    static thread_local TempTable A;
    memset(&A, 0, sizeof A);
    unsigned max_quads = 0;
    for (int i = 0; i < n; ++i) {
        const ofx_temporal_desc &d = items[i];
        OFX_REQUIRE(d.n_neighbours >= 1 && d.n_neighbours <= OFX_TEMPORAL_MAX_NEIGHBOURS, "%s: item %d: n_neighbours = %d is not in 1 .. %d", who, i,
                    d.n_neighbours, OFX_TEMPORAL_MAX_NEIGHBOURS);
        OFX_REQUIRE(d.d_centre != nullptr, "%s: item %d: d_centre is null", who, i);
        OFX_REQUIRE(d.d_dst != nullptr, "%s: item %d: d_dst is null", who, i);
        OFX_REQUIRE(d.channels == 1 || d.channels == 3, "%s: item %d: channels = %d is not 1 or 3", who, i, d.channels);
        OFX_REQUIRE(d.w >= 1 && d.w <= kMaxSize && d.h >= 1 && d.h <= kMaxSize, "%s: item %d: the size %d x %d is not in 1 .. 2^16", who, i, d.w, d.h);
        OFX_REQUIRE((long long)d.w * d.h < (1ll << 28), "%s: item %d: w * h = %lld is not below 2^28", who, i, (long long)d.w * d.h);
        const int row = d.channels * d.w;
        OFX_REQUIRE(d.centre_pitch >= row, "%s: item %d: centre_pitch = %d is below %d", who, i, d.centre_pitch, row);
        OFX_REQUIRE(d.dst_pitch >= row, "%s: item %d: dst_pitch = %d is below %d", who, i, d.dst_pitch, row);
        OFX_REQUIRE(plane_fits(d.h, d.centre_pitch, row), "%s: item %d: the centre plane has 2^31 bytes or more", who, i);
        OFX_REQUIRE(plane_fits(d.h, d.dst_pitch, row), "%s: item %d: the destination plane has 2^31 bytes or more", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_stats & 7) == 0, "%s: item %d: d_stats must be 8-byte aligned", who, i);
        const Span dst = span_of(d.d_dst, d.h, d.dst_pitch, row);
        OFX_REQUIRE(apart(span_of(d.d_centre, d.h, d.centre_pitch, row), dst), "%s: item %d: d_centre and d_dst overlap", who, i);
        OFX_REQUIRE(d.d_stats == nullptr || apart(Span{(uintptr_t)d.d_stats, (uintptr_t)d.d_stats + kStats * sizeof(int64_t)}, dst),
                    "%s: item %d: d_stats and d_dst overlap", who, i);
        TempItem &it = A.item[i];
        for (int k = 0; k < d.n_neighbours; ++k) {
            const ofx_temporal_neighbour &s = d.neighbour[k];
            OFX_REQUIRE(s.d_plane != nullptr, "%s: item %d: neighbour %d: d_plane is null", who, i, k);
            OFX_REQUIRE(s.d_field != nullptr, "%s: item %d: neighbour %d: d_field is null", who, i, k);
            OFX_REQUIRE(s.pitch >= row, "%s: item %d: neighbour %d: pitch = %d is below %d", who, i, k, s.pitch, row);
            OFX_REQUIRE(plane_fits(d.h, s.pitch, row), "%s: item %d: neighbour %d: the plane has 2^31 bytes or more", who, i, k);
            OFX_REQUIRE(((uintptr_t)s.d_field & 7) == 0, "%s: item %d: neighbour %d: d_field must be 8-byte aligned", who, i, k);
            OFX_REQUIRE(apart(span_of(s.d_plane, d.h, s.pitch, row), dst), "%s: item %d: neighbour %d: d_plane and d_dst overlap", who, i, k);
            OFX_REQUIRE(apart(Span{(uintptr_t)s.d_field, (uintptr_t)s.d_field + (size_t)d.w * (size_t)d.h * 8}, dst),
                        "%s: item %d: neighbour %d: d_field and d_dst overlap", who, i, k);
            it.nb[k].plane = s.d_plane, it.nb[k].field = s.d_field, it.nb[k].pitch = s.pitch;
        }
        it.centre = d.d_centre, it.dst = d.d_dst, it.stats = reinterpret_cast<unsigned long long *>(d.d_stats);
        it.centre_pitch = d.centre_pitch, it.dst_pitch = d.dst_pitch, it.w = d.w, it.h = d.h, it.channels = d.channels, it.n_nb = d.n_neighbours;
        it.quads_per_row = (unsigned)ofx_div_up(d.w, kQuad);
        it.quads = it.quads_per_row * (unsigned)d.h; // (below 2^28)
        max_quads = it.quads > max_quads ? it.quads : max_quads;
    }
    memcpy(A.weights, prm->weights, sizeof A.weights);
    A.wc = prm->centre_weight;
    hipStream_t st = ofx_stream(stream);
    for (int i = 0; i < n; ++i)
        if (items[i].d_stats) OFX_TRY(ofx_zero_words(items[i].d_stats, kStats, st));
    if (n == 1)
        launch<1>(A, n, max_quads, st);
    else
        launch<OFX_STREAM_MAX_BATCH>(A, n, max_quads, st);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
