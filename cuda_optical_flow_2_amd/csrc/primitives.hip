// API-compat primitives: generic (any mask / window) device counterparts of the reference kernels that the fused
// flow path does not use directly.  They exist so that gpu::conv_*, gpu::srm_*, gpu::inverse_matrix*,
// gpu::grayscale_avg and gpu::bilinear_filter (OptFlowGpu.cuh:5-35) have bit-exact device implementations.
// They are plain one-thread-per-pixel kernels with coalesced rows; the hot path lives in lk_level.hip.
//
// Built with -ffp-contract=off: the reference's CPU build rounds every product and sum separately, and the
// per-tap truncation of the integer convolutions depends on that.
#include <math.h>

#include "ofx_internal.h"
#include "bilateral_common.h"

namespace {

constexpr int kMaxTaps = 81; // masks up to 9x9 travel as kernel arguments

struct MaskArg {
    float m[kMaxTaps];
    int mw, mh;
};

int make_mask(const float *h_mask, int mw, int mh, MaskArg *out, const char *who)
{
    OFX_REQUIRE(h_mask != nullptr, "%s: mask is null", who);
    OFX_REQUIRE(mw > 0 && mh > 0 && mw * mh <= kMaxTaps, "%s: mask %dx%d unsupported (at most %d taps)", who, mw, mh, kMaxTaps);
    for (int i = 0; i < mw * mh; ++i) out->m[i] = h_mask[i];
    out->mw = mw;
    out->mh = mh;
    return OFX_OK;
}

// OptFlowGpu.cu:47-60 / OptFlowCPU.cpp:27-28
__global__ __launch_bounds__(256) void gray_kernel(const uint8_t *src3, uint8_t *dst3, size_t n)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint8_t *s = src3 + 3 * p;
    const uint8_t g = (uint8_t)(((int)s[0] + (int)s[1] + (int)s[2]) / 3);
    uint8_t *d = dst3 + 3 * p;
    d[0] = d[1] = d[2] = g;
}

// The same, sixteen pixels = 48 bytes = three 16-byte pieces per thread (4-byte aligned images): the byte-per-instruction form above
// spends 18 us on a 4K frame whose 50 MB take 10 us at the part's copy rate.  A piece's sixteen bytes hold the channels of 5 1/3
// pixels; the sums are formed on the 12 dwords in registers and every output byte is its pixel's average.
__global__ __launch_bounds__(256) void gray_x16_kernel(const uint32_t *src, uint32_t *dst, size_t n16)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n16) return;
    const uint4 *s = reinterpret_cast<const uint4 *>(src + 12 * t);
    const uint4 a = s[0], b = s[1], c = s[2];
    const uint32_t in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    uint32_t out[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) { // four pixels in three dwords
        const uint32_t d0 = in[3 * q], d1 = in[3 * q + 1], d2 = in[3 * q + 2];
        const uint32_t g0 = ((d0 & 0xffu) + ((d0 >> 8) & 0xffu) + ((d0 >> 16) & 0xffu)) / 3u;
        const uint32_t g1 = ((d0 >> 24) + (d1 & 0xffu) + ((d1 >> 8) & 0xffu)) / 3u;
        const uint32_t g2 = (((d1 >> 16) & 0xffu) + (d1 >> 24) + (d2 & 0xffu)) / 3u;
        const uint32_t g3 = (((d2 >> 8) & 0xffu) + ((d2 >> 16) & 0xffu) + (d2 >> 24)) / 3u;
        out[3 * q] = g0 * 0x010101u | (g1 << 24);
        out[3 * q + 1] = g1 * 0x0101u | (g2 * 0x01010000u);
        out[3 * q + 2] = g2 | (g3 * 0x01010100u);
    }
    uint4 *d = reinterpret_cast<uint4 *>(dst + 12 * t);
    d[0] = uint4{out[0], out[1], out[2], out[3]};
    d[1] = uint4{out[4], out[5], out[6], out[7]};
    d[2] = uint4{out[8], out[9], out[10], out[11]};
}

// int accumulator, float add, truncation after every tap (OptFlowCPU.cpp:62,102 == OptFlowGpu.cu:137-139,414)
__device__ __forceinline__ int acc_trunc(int acc, int px, float m) { return (int)((float)acc + (float)px * m); }

// OptFlowGpu.cu:108-147 (FLOAT_ACC=false) and :282-342 (FLOAT_ACC=true, the "tiled" variant's arithmetic)
template <bool FLOAT_ACC>
__global__ __launch_bounds__(256) void conv_3ch_kernel(const uint8_t *src3, uint8_t *dst3, int w, int h, const MaskArg M)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int ox = M.mw >> 1, oy = M.mh >> 1;
    int ia[3] = {0, 0, 0};
    float fa[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < M.mh; ++i) {
        const int ty = y - oy + i;
        if (ty < 0 || ty >= h) continue;
        for (int j = 0; j < M.mw; ++j) {
            const int tx = x - ox + j;
            if (tx < 0 || tx >= w) continue;
            const uint8_t *s = src3 + 3 * ((size_t)ty * w + tx);
            const float m = M.m[i * M.mw + j];
            if constexpr (FLOAT_ACC) {
                fa[0] += (float)s[0] * m;
                fa[1] += (float)s[1] * m;
                fa[2] += (float)s[2] * m;
            } else {
                ia[0] = acc_trunc(ia[0], s[0], m);
                ia[1] = acc_trunc(ia[1], s[1], m);
                ia[2] = acc_trunc(ia[2], s[2], m);
            }
        }
    }
    uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
    if constexpr (FLOAT_ACC) {
        d[0] = (uint8_t)(int)fa[0];
        d[1] = (uint8_t)(int)fa[1];
        d[2] = (uint8_t)(int)fa[2];
    } else {
        d[0] = (uint8_t)ia[0];
        d[1] = (uint8_t)ia[1];
        d[2] = (uint8_t)ia[2];
    }
}

// OptFlowGpu.cu:380-425 (u8 out) and :1040-1090 (f32 out)
template <bool F32_OUT>
__global__ __launch_bounds__(256) void conv_3ch_1ch_kernel(const uint8_t *src3, int w, int h, void *dst, const MaskArg M)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int ox = M.mw >> 1, oy = M.mh >> 1;
    int ia = 0;
    float fa = 0.f;
    for (int i = 0; i < M.mh; ++i) {
        const int ty = y - oy + i;
        if (ty < 0 || ty >= h) continue;
        for (int j = 0; j < M.mw; ++j) {
            const int tx = x - ox + j;
            if (tx < 0 || tx >= w) continue;
            const float m = M.m[i * M.mw + j];
            const int px = src3[3 * ((size_t)ty * w + tx)];
            if constexpr (F32_OUT) {
                if (m == 0.0f) continue; // OptFlowGpu.cu:1075
                fa += (float)px * m;
            } else {
                ia = acc_trunc(ia, px, m);
            }
        }
    }
    if constexpr (F32_OUT)
        static_cast<float *>(dst)[(size_t)y * w + x] = fa;
    else
        static_cast<uint8_t *>(dst)[(size_t)y * w + x] = (uint8_t)ia;
}

// The same correlation, four adjacent output pixels per thread (round 4).  The kernel above spends ~170 instructions per pixel on
// byte addresses and bounds tests around nine byte loads (64 / 56 us per 4K plane).  Here a thread fetches, per mask row, the 24
// bytes that hold channel 0 of its 4 + MW - 1 source pixels as six dwords (unaligned: through a buffer resource), converts the
// bytes where they lie (v_cvt_f32_ubyteN) and feeds four accumulators in the reference's tap order.  A tap outside the image is
// skipped by the reference; here it enters as pixel value 0, which leaves the float accumulator unchanged (+-0 added to a sum that
// cannot be -0) and the truncating int accumulator too as long as it stays below 2^24 (the host checks the mask: sum |m| * 255).
// Threads whose window touches the image's left or right edge take the loop of the kernel above.
// MH > 0: the mask's height at compile time (square masks: the reference's 3x3 and 5x5).  The loads of a thread's kConvRows + MH - 1
// source rows are then ALL issued before the first is used (one memory round trip per thread instead of one per mask row); a row
// outside the image is fetched through the resource's range check and enters as zeros, which is the reference's skip by the argument
// above; every output pixel still receives its taps in the reference's row-major order.  Measured at 4K, 3x3 (second session of round
// 4): 24.0-25.7 us against 27.7-27.9 row by row (u8), 25.0 against 26.2 (float).  kConvRows = 4 (four output rows per thread from six
// source rows: half the loads per pixel, a quarter of the waves) was built too and is SLOWER, 40-41 us: the launch is bound neither
// by its load count nor by the rate at which waves start.  0: M.mh at run time, row by row.
constexpr int kConvRows = 1;
template <bool F32_OUT, int MW, int MH = 0>
__global__ __launch_bounds__(256) void conv_3ch_1ch_x4_kernel(const uint8_t *src3, int w, int h, void *dst, const MaskArg M)
{
    constexpr int NP = 4 + MW - 1;              // source pixels per row
    constexpr int ND = (3 * (NP - 1) + 1 + 3) / 4; // dwords that hold their channel-0 bytes
    constexpr int RPT = MH > 0 ? kConvRows : 1; // output rows per thread
    const int x0 = 4 * ((int)blockIdx.x * 64 + ((int)threadIdx.x & 63)), y0 = ((int)blockIdx.y * 4 + ((int)threadIdx.x >> 6)) * RPT;
    if (x0 >= w || y0 >= h) return;
    const int ox = MW >> 1, oy = M.mh >> 1;
    const bool inner = x0 - ox >= 0 && x0 + NP - ox <= w && x0 + 4 <= w && (3ll * ((long long)w * h) >= 3ll * ((long long)(h - 1) * w + x0 - ox) + 4 * ND);
    if (!inner) { // the image's edges: pixel by pixel, as conv_3ch_1ch_kernel
        for (int y = y0; y < min(y0 + RPT, h); ++y)
        for (int x = x0; x < min(x0 + 4, w); ++x) {
            int ia = 0;
            float fa = 0.f;
            for (int i = 0; i < M.mh; ++i) {
                const int ty = y - oy + i;
                if (ty < 0 || ty >= h) continue;
                for (int j = 0; j < MW; ++j) {
                    const int tx = x - ox + j;
                    if (tx < 0 || tx >= w) continue;
                    const float m = M.m[i * MW + j];
                    const int px = src3[3 * ((size_t)ty * w + tx)];
                    if constexpr (F32_OUT) {
                        if (m == 0.0f) continue;
                        fa += (float)px * m;
                    } else {
                        ia = acc_trunc(ia, px, m);
                    }
                }
            }
            if constexpr (F32_OUT) static_cast<float *>(dst)[(size_t)y * w + x] = fa;
            else static_cast<uint8_t *>(dst)[(size_t)y * w + x] = (uint8_t)ia;
        }
        return;
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src3), 0, 3 * w * h, 0x00027000);
    const uint32_t b0 = 3u * (uint32_t)(x0 - ox);
    int ia[4] = {0, 0, 0, 0};
    float fa[4] = {0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] const int y = y0;
    auto put = [&](int yy) {
        if constexpr (F32_OUT) {
            float *d = static_cast<float *>(dst) + (size_t)yy * w + x0;
            if (((uintptr_t)d & 15) == 0) *reinterpret_cast<float4 *>(d) = float4{fa[0], fa[1], fa[2], fa[3]}; // (one 16-byte store per lane)
            else d[0] = fa[0], d[1] = fa[1], d[2] = fa[2], d[3] = fa[3];
        } else {
            uint8_t *d = static_cast<uint8_t *>(dst) + (size_t)yy * w + x0;
            const uint32_t pk = ((uint32_t)ia[0] & 0xffu) | (((uint32_t)ia[1] & 0xffu) << 8) | (((uint32_t)ia[2] & 0xffu) << 16) | ((uint32_t)ia[3] << 24);
            if (((uintptr_t)d & 3) == 0) *reinterpret_cast<uint32_t *>(d) = pk;
            else d[0] = (uint8_t)ia[0], d[1] = (uint8_t)ia[1], d[2] = (uint8_t)ia[2], d[3] = (uint8_t)ia[3];
        }
    };
    if constexpr (MH > 0) {
        constexpr int NR = RPT + MH - 1;
        uint32_t dw[NR][ND];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int ty = y0 - oy + i;
            const int ro = (uint32_t)ty < (uint32_t)h ? ty * w * 3 : (int)0x80000000; // (outside the image: beyond the resource, reads 0)
#pragma unroll
            for (int k = 0; k < ND; ++k) dw[i][k] = __builtin_amdgcn_raw_buffer_load_b32(rs, b0 + 4u * (uint32_t)k, ro, 0);
        }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            if (y0 + r >= h) break; // (uniform over the wave)
#pragma unroll
            for (int j = 0; j < 4; ++j) ia[j] = 0, fa[j] = 0.f;
#pragma unroll
            for (int i = 0; i < MH; ++i) {
                float px[NP];
#pragma unroll
                for (int j = 0; j < NP; ++j) px[j] = (float)((dw[r + i][(3 * j) >> 2] >> (8 * ((3 * j) & 3))) & 0xffu); // (v_cvt_f32_ubyteN)
#pragma unroll
                for (int q = 0; q < MW; ++q) {
                    const float m = M.m[i * MW + q];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (F32_OUT) fa[j] += px[j + q] * m;
                        else ia[j] = (int)((float)ia[j] + px[j + q] * m);
                    }
                }
            }
            put(y0 + r);
        }
        return;
    }
    for (int i = 0; i < M.mh; ++i) {
        const int ty = y - oy + i;
        if (ty < 0 || ty >= h) continue; // (uniform over the wave: one row per wave)
        const int ro = ty * w * 3;
        uint32_t dw[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) dw[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, b0 + 4u * (uint32_t)k, ro, 0);
        float px[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) px[j] = (float)((dw[(3 * j) >> 2] >> (8 * ((3 * j) & 3))) & 0xffu); // (v_cvt_f32_ubyteN)
#pragma unroll
        for (int q = 0; q < MW; ++q) {
            const float m = M.m[i * MW + q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (F32_OUT) fa[j] += px[j + q] * m;
                else ia[j] = (int)((float)ia[j] + px[j + q] * m);
            }
        }
    }
    put(y);
}

// OptFlowGpu.cu:1463-1502 / :1549-1588: window clipped at the border, taps in row-major order
template <typename TIn, typename TAcc>
__global__ __launch_bounds__(256) void srm_kernel(const TIn *a, const TIn *b, int w, int h, int ww, int wh, TAcc *dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int ox = ww >> 1, oy = wh >> 1;
    TAcc acc = 0;
    for (int p = 0; p < wh; ++p) {
        const int ty = y - oy + p;
        if (ty < 0 || ty >= h) continue;
        for (int q = 0; q < ww; ++q) {
            const int tx = x - ox + q;
            if (tx < 0 || tx >= w) continue;
            const size_t t = (size_t)ty * w + tx;
            acc += (TAcc)a[t] * (TAcc)b[t];
        }
    }
    dst[(size_t)y * w + x] = acc;
}

// 2x2 solves.  variant 0: OptFlowGpu.cu:1737-1754, 1: OptFlowCPU.cpp:369-382 (c unscaled), 2: OptFlowCPU.cpp:293-304
template <typename T>
__global__ __launch_bounds__(256) void solve_kernel(const T *sxx, const T *syy, const T *sxy, const T *sxt, const T *syt,
                                                    float *flow, size_t n, int variant)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float u, v;
    if (variant == OFX_SOLVE_F32) {
        float a = (float)sxx[p], b = (float)sxy[p], c = b, d = (float)syy[p];
        const float pre = 1 / (a * d - b * c);
        a *= pre;
        b *= pre;
        c *= pre;
        d *= pre;
        u = -d * (float)sxt[p] + b * (float)syt[p];
        v = c * (float)sxt[p] - a * (float)syt[p];
    } else {
        double a = (double)sxx[p], b = (double)sxy[p], c = b, d = (double)syy[p];
        const double xt = (double)sxt[p], yt = (double)syt[p];
        const double pre = 1 / (a * d - b * c);
        a *= pre;
        b *= pre;
        if (variant == OFX_SOLVE_F64) c *= pre;
        d *= pre;
        u = (float)(-d * xt + b * yt);
        v = (float)(c * xt - a * yt);
    }
    reinterpret_cast<float2 *>(flow)[p] = make_float2(u, v);
}

// Bilateral filter (the reference calls it bilinear_filter): OptFlowGpu.cu:1984-2048 / OptFlowCPU.cpp:401-465.
// The range weight depends only on the integer grey difference k in [-255,255], so the host evaluates
// 1/(2 pi sB^2) * pow(e, -k^2/(2 sB^2)) with libm for k^2 of 0..255 -- the very expression the CPU path evaluates
// per tap -- and the kernel looks it up: identical doubles, no transcendental on the device.
//
// The arithmetic is the reference's, operation for operation and in its tap order (row-major over the window, double
// accumulators, (src * nb) * ns) -- that is what makes the output bit-identical, and it is what the kernel costs: 81 taps
// of 7 (grey image) to 15 (colour) double-precision instructions per pixel at 9x9.  What the kernel removes is everything
// else: a block stages its (64 + ww - 1) x (4 + wh - 1) neighbourhood in LDS once -- the grey value as a ready-made byte
// offset into the range table, pixels outside the image as a sentinel whose offsets land on zero entries, so that skipped
// taps become additions of +0.0 (exact no-ops on these non-negative sums) and the tap loop has no bounds tests -- the
// range table sits in LDS as a function of the SIGNED difference (no abs), the spatial weights arrive as scalars, and a
// block whose pixels all have three equal channels (main.cu:240 filters the grey image) accumulates one channel.

constexpr int kBilTileW = 64, kBilTileH = 4;

template <int WW>
__global__ __launch_bounds__(256) void bilateral_tiled_kernel(const uint8_t *src3, const uint8_t *gray3, uint8_t *dst3, int w, int h, int wh,
                                                              const BilateralArg B)
{
    constexpr int R = WW >> 1, TW = kBilTileW + 2 * R;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    double *lut = reinterpret_cast<double *>(smem);                                   // kBilLut doubles
    uint32_t *spx = reinterpret_cast<uint32_t *>(smem + kBilLut * sizeof(double));    // [rows][TW]: s0 | s1 << 8 | s2 << 16
    const int ry = wh >> 1, rows = kBilTileH + 2 * ry;
    uint16_t *gof = reinterpret_cast<uint16_t *>(spx + (size_t)rows * TW);            // [rows][TW]: 8 * grey value (or sentinel)
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kBilTileW, y0 = (int)blockIdx.y * kBilTileH;

    for (int i = tid; i < kBilLut; i += 256) {
        const int d = i - 255; // signed grey difference
        lut[i] = (d >= -255 && d <= 255) ? B.range[d < 0 ? -d : d] : 0.0;
    }
    int grey_only = 1;
    for (int i = tid; i < rows * TW; i += 256) {
        const int tx = x0 - R + i % TW, ty = y0 - ry + i / TW;
        uint32_t px = 0u;
        uint16_t go = (uint16_t)(8 * kBilSentinel);
        if (tx >= 0 && tx < w && ty >= 0 && ty < h) {
            const size_t q = 3 * ((size_t)ty * w + tx);
            const uint32_t s0 = src3[q], s1 = src3[q + 1], s2 = src3[q + 2];
            px = s0 | (s1 << 8) | (s2 << 16);
            go = (uint16_t)(8 * (int)gray3[q]);
            grey_only &= (s0 == s1 && s1 == s2) ? 1 : 0;
        }
        spx[i] = px;
        gof[i] = go;
    }
    grey_only = __syncthreads_and(grey_only); // (also orders the tile and the table before the taps)

    const int lx = tid & 63, ly = tid >> 6, x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    // byte offset of table entry (g - f0 + 255) = gof - f0off, f0off = 8 * (f0 - 255)  (may be negative: signed arithmetic)
    const int f0off = (int)gof[(ly + ry) * TW + lx + R] - 8 * 255;
    const uint8_t *lut_b = reinterpret_cast<const uint8_t *>(lut);
    double wsum = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (grey_only) {
        for (int m = 0; m < wh; ++m) {
            const uint32_t *prow = spx + (ly + m) * TW + lx;
            const uint16_t *grow = gof + (ly + m) * TW + lx;
#pragma unroll
            for (int n = 0; n < WW; ++n) {
                const double nb = *reinterpret_cast<const double *>(lut_b + ((int)grow[n] - f0off));
                const double ns = B.spatial[m * WW + n];
                wsum += nb * ns;
                a0 += (double)(prow[n] & 0xffu) * nb * ns;
            }
        }
        a1 = a2 = a0;
    } else {
        for (int m = 0; m < wh; ++m) {
            const uint32_t *prow = spx + (ly + m) * TW + lx;
            const uint16_t *grow = gof + (ly + m) * TW + lx;
#pragma unroll
            for (int n = 0; n < WW; ++n) {
                const double nb = *reinterpret_cast<const double *>(lut_b + ((int)grow[n] - f0off));
                const double ns = B.spatial[m * WW + n];
                const uint32_t px = prow[n];
                wsum += nb * ns;
                a0 += (double)(px & 0xffu) * nb * ns;
                a1 += (double)((px >> 8) & 0xffu) * nb * ns;
                a2 += (double)((px >> 16) & 0xffu) * nb * ns;
            }
        }
    }
    uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
    d[0] = (uint8_t)(int)(a0 / wsum);
    d[1] = (uint8_t)(int)(a1 / wsum);
    d[2] = (uint8_t)(int)(a2 / wsum);
}

// ---- the bit-exact filter of an image that is its own grey image (main.cu:240: src == gray, one pointer), round 4 -----------------
// bilateral_tiled_kernel reads the LDS three times per tap (the source pixel, the grey offset, the 8-byte table entry) for its
// seven double-precision operations, and the LDS is what bounds it.  With src == gray and every channel equal -- checked per tile while
// loading -- the pixel value IS the grey value: the tile holds one int per pixel, a lane owns a 2 x 2 block of pixels and reads a
// tile row's WW + 1 values as 8-byte pieces that serve both of its output rows, and the tap is v_lshl_add_u32 (the table address),
// ds_read_b64 (nb), v_cvt_f64_u32, and the reference's five double operations in the reference's order (wsum += nb * ns;
// a += ((double)px * nb) * ns, row-major over the window: OptFlowCPU.cpp:437-452): 1.1 LDS reads per tap instead of 3.
// Out-of-image taps: the sentinel grey value's table entries are +0.0, additions of +0.0 to these non-negative sums are exact no-ops
// (as in bilateral_tiled_kernel).  A tile whose channels differ takes a slow pixel-by-pixel path with the channels out of global memory.

template <int WW>
__global__ __launch_bounds__(kExThreads) void bilateral_exact_own_kernel(const uint8_t *img3, uint8_t *dst3, int w, int h, const BilateralArg B)
{
    constexpr int R = WW >> 1, TW = kExTileW + 2 * R, NG = (TW + 3) / 4, TWP = NG * 4, ROWS = kExTileH + 2 * R;
    __shared__ __attribute__((aligned(16))) double lut[kBilLut];
    __shared__ __attribute__((aligned(16))) int gt[ROWS * TWP]; // grey value, or kBilSentinel
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kExTileW, y0 = (int)blockIdx.y * kExTileH;
    const int bytes = 3 * w * h; // (below 2 GB: the launcher)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(img3), 0, bytes, 0x00027000);
    for (int i = tid; i < kBilLut; i += kExThreads) {
        const int d = i - 255; // signed grey difference
        lut[i] = (d >= -255 && d <= 255) ? B.range[d < 0 ? -d : d] : 0.0;
    }
    uint32_t colour = 0u;
    for (int i = tid; i < ROWS * NG; i += kExThreads) {
        const int gr = i / NG, gc = i - gr * NG, ty = y0 - R + gr, tx = x0 - R + 4 * gc;
        int g[4] = {kBilSentinel, kBilSentinel, kBilSentinel, kBilSentinel};
        if (ty >= 0 && ty < h && tx + 3 >= 0 && tx < w) {
            const int off = 3 * (ty * w + tx);
            if (off >= 0 && off + 12 <= bytes) { // twelve bytes = four pixels in three dwords (as bilateral_lut_kernel)
                const uint32_t a = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0), b = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4, 0, 0),
                               c = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 8, 0, 0);
                colour |= (a ^ __builtin_amdgcn_perm(a, a, 0x03000000u)) | (b ^ __builtin_amdgcn_perm(b, a, 0x06060303u)) |
                          (c ^ __builtin_amdgcn_perm(c, b, 0x05050502u));
                const int v[4] = {(int)(a & 0xffu), (int)(a >> 24), (int)((b >> 16) & 0xffu), (int)((c >> 8) & 0xffu)};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (tx + k >= 0 && tx + k < w) g[k] = v[k];
            } else {
                for (int k = 0; k < 4; ++k)
                    if (tx + k >= 0 && tx + k < w) {
                        const uint8_t *q = img3 + 3 * ((size_t)ty * w + tx + k);
                        colour |= (uint32_t)(q[0] ^ q[1]) | (uint32_t)(q[0] ^ q[2]);
                        g[k] = (int)q[0];
                    }
            }
        }
        *reinterpret_cast<int4 *>(gt + gr * TWP + 4 * gc) = int4{g[0], g[1], g[2], g[3]};
    }
    const int grey = __syncthreads_and(colour == 0u ? 1 : 0);
    const int lane = tid & 63, wv = tid >> 6;
    const uint8_t *lut_b = reinterpret_cast<const uint8_t *>(lut);
    if (!grey) { // channels differ: pixel by pixel, the channels out of global memory, the reference's order
        for (int t = 0; t < 8; ++t) {
            const int lx = 2 * lane + (t & 1), ly = 4 * wv + (t >> 1), x = x0 + lx, y = y0 + ly;
            if (x >= w || y >= h) continue;
            const int g0 = gt[(ly + R) * TWP + lx + R];
            double wsum = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int m = 0; m < WW; ++m)
                for (int n = 0; n < WW; ++n) {
                    const int gq = gt[(ly + m) * TWP + lx + n];
                    if (gq == kBilSentinel) continue; // outside the image (OptFlowCPU.cpp:432 skips the tap)
                    const double nb = lut[gq - g0 + 255], ns = B.spatial[m * WW + n];
                    const uint8_t *q = img3 + 3 * ((size_t)(y - R + m) * w + (x - R + n));
                    wsum += nb * ns;
                    a0 += (double)q[0] * nb * ns;
                    a1 += (double)q[1] * nb * ns;
                    a2 += (double)q[2] * nb * ns;
                }
            uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
            d[0] = (uint8_t)(int)(a0 / wsum);
            d[1] = (uint8_t)(int)(a1 / wsum);
            d[2] = (uint8_t)(int)(a2 / wsum);
        }
        return;
    }
#pragma unroll 1
    for (int pr = 0; pr < 2; ++pr) {
        const int ly = 4 * wv + 2 * pr; // output rows ly, ly + 1 of the tile
        const int g00 = gt[(ly + R) * TWP + 2 * lane + R], g01 = gt[(ly + R) * TWP + 2 * lane + 1 + R], g10 = gt[(ly + 1 + R) * TWP + 2 * lane + R],
                  g11 = gt[(ly + 1 + R) * TWP + 2 * lane + 1 + R];
        // byte offset of table entry (g - g_0 + 255) = 8 g + base
        const int b00 = 8 * (255 - g00), b01 = 8 * (255 - g01), b10 = 8 * (255 - g10), b11 = 8 * (255 - g11);
        double acc0[4] = {0.0, 0.0, 0.0, 0.0}, acc1[4] = {0.0, 0.0, 0.0, 0.0}; // per output row: wsum A, a A, wsum B, a B
#pragma unroll 1
        for (int t = 0; t <= WW; ++t) { // tile row ly + t: tap row t of output row ly, tap row t - 1 of output row ly + 1
            const int2 *grow = reinterpret_cast<const int2 *>(gt + (ly + t) * TWP + 2 * lane);
            int v[WW + 1];
#pragma unroll
            for (int k = 0; k < (WW + 1) / 2; ++k) {
                const int2 q = grow[k];
                v[2 * k] = q.x;
                v[2 * k + 1] = q.y;
            }
            if (t < WW) exact_row_taps<WW>(v, b00, b01, lut_b, B.spatial + (t < WW ? t : 0) * WW, acc0);
            if (t > 0) exact_row_taps<WW>(v, b10, b11, lut_b, B.spatial + (t > 0 ? t - 1 : 0) * WW, acc1);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + ly + r, xA = x0 + 2 * lane;
            if (y >= h || xA >= w) continue;
            const double(&acc)[4] = r ? acc1 : acc0;
            const uint32_t bA = (uint32_t)(uint8_t)(int)(acc[1] / acc[0]), bB = (uint32_t)(uint8_t)(int)(acc[3] / acc[2]);
            uint8_t *d = dst3 + 3 * ((size_t)y * w + xA);
            if (xA + 1 < w) {
                uint16_t *d2 = reinterpret_cast<uint16_t *>(d);
                d2[0] = (uint16_t)(bA * 0x0101u), d2[1] = (uint16_t)(bA | (bB << 8)), d2[2] = (uint16_t)(bB * 0x0101u);
            } else {
                d[0] = (uint8_t)bA, d[1] = (uint8_t)bA, d[2] = (uint8_t)bA;
            }
        }
    }
}

template <int WW>
int launch_bilateral_exact_own(const uint8_t *d_img3, uint8_t *d_dst3, int w, int h, const BilateralArg &B, hipStream_t st)
{
    hipLaunchKernelGGL(bilateral_exact_own_kernel<WW>, dim3(ofx_div_up(w, kExTileW), ofx_div_up(h, kExTileH)), dim3(kExThreads), 0, st, d_img3, d_dst3, w,
                       h, B);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// ---- the same filter within SURVEY 8c's tolerance for this stage (+-1 LSB), opt-in ---------------------------------------------
// The exact kernel above is bound by its definition: 81 taps x 7-15 double-precision operations per pixel in the reference's
// order, each weight an 8-byte LDS gather.  This one keeps the filter and drops the order: float accumulators, the range weight
// evaluated instead of looked up, and for a grey image (main.cu:240 filters the grey frame) the quotient written around the
// centre value:
//     w(q) = ns(q) * nb(g_q - g_0) = exp2( c * d^2 + log2 ns(q) ),  d = g_q - g_0,  c = -log2(e) / (2 sB^2)
//     out  = trunc( sum g_q w / sum w ) = trunc( g_0 + sum d w / sum w )
// (both normalisation constants cancel in the quotient).  Per tap: one LDS read, a subtraction, a square, a fused multiply-add,
// v_exp_f32, two accumulations -- 6 VALU operations against the exact kernel's 7 doubles and a gather.  The float arithmetic
// moves the quotient by ~1e-4 grey levels at most, so the truncated byte differs from the reference's by at most one where
// the quotient lies that close to an integer (tests/test_gpu_surface.py asserts +-1 on every size and window of the exact
// kernel's test).  Pixels outside the image are stored as a grey value of -1e6 (kBilFastOutside): d^2 = 1e12, so their weight
// underflows to exactly 0 for every sigma_b the entry point lets through (<= 2e4: c * d^2 <= -1800; beyond, the exact kernel runs).
constexpr float kBilFastOutside = -1.0e6f; // (exactly representable next to 0 .. 255: the differences stay exact)
struct BilateralFastArg {
    float log2_spatial[kMaxBilateral * kMaxBilateral]; // log2 of the normalised spatial weights
    float c;                                           // -log2(e) / (2 sigma_b^2)
};

template <int WW>
__global__ __launch_bounds__(256) void bilateral_fast_kernel(const uint8_t *src3, const uint8_t *gray3, uint8_t *dst3, int w, int h, int wh,
                                                             const BilateralFastArg B)
{
    constexpr int R = WW >> 1, TW = kBilTileW + 2 * R;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int ry = wh >> 1, rows = kBilTileH + 2 * ry;
    float *gf = reinterpret_cast<float *>(smem);                                   // [rows][TW]: grey value (or kBilFastOutside)
    uint32_t *spx = reinterpret_cast<uint32_t *>(gf + (size_t)rows * TW);           // [rows][TW]: s0 | s1 << 8 | s2 << 16
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kBilTileW, y0 = (int)blockIdx.y * kBilTileH;
    int grey_src = 1; // every pixel of the tile: three equal channels that are the grey value itself (src == gray, main.cu:240)
    for (int i = tid; i < rows * TW; i += 256) {
        const int tx = x0 - R + i % TW, ty = y0 - ry + i / TW;
        uint32_t px = 0u;
        float g = kBilFastOutside;
        if (tx >= 0 && tx < w && ty >= 0 && ty < h) {
            const size_t q = 3 * ((size_t)ty * w + tx);
            const uint32_t s0 = src3[q], s1 = src3[q + 1], s2 = src3[q + 2], gq = gray3[q];
            px = s0 | (s1 << 8) | (s2 << 16);
            g = (float)gq;
            grey_src &= (s0 == gq && s1 == gq && s2 == gq) ? 1 : 0;
        }
        gf[i] = g;
        spx[i] = px;
    }
    grey_src = __syncthreads_and(grey_src);
    const int lx = tid & 63, ly = tid >> 6, x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const float g0 = gf[(ly + ry) * TW + lx + R];
    float wsum = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (grey_src) {
        for (int m = 0; m < wh; ++m) {
            const float *grow = gf + (ly + m) * TW + lx;
#pragma unroll
            for (int n = 0; n < WW; ++n) {
                const float d = grow[n] - g0;
                const float wgt = __builtin_amdgcn_exp2f(__builtin_fmaf(d * d, B.c, B.log2_spatial[m * WW + n]));
                wsum += wgt;
                a0 = __builtin_fmaf(d, wgt, a0);
            }
        }
        a0 = g0 + a0 / wsum;
        a1 = a2 = a0;
    } else {
        for (int m = 0; m < wh; ++m) {
            const float *grow = gf + (ly + m) * TW + lx;
            const uint32_t *prow = spx + (ly + m) * TW + lx;
#pragma unroll
            for (int n = 0; n < WW; ++n) {
                const float d = grow[n] - g0;
                const float wgt = __builtin_amdgcn_exp2f(__builtin_fmaf(d * d, B.c, B.log2_spatial[m * WW + n]));
                const uint32_t px = prow[n];
                wsum += wgt;
                a0 = __builtin_fmaf((float)(px & 0xffu), wgt, a0);
                a1 = __builtin_fmaf((float)((px >> 8) & 0xffu), wgt, a1);
                a2 = __builtin_fmaf((float)((px >> 16) & 0xffu), wgt, a2);
            }
        }
        a0 /= wsum;
        a1 /= wsum;
        a2 /= wsum;
    }
    uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
    d[0] = (uint8_t)(int)a0;
    d[1] = (uint8_t)(int)a1;
    d[2] = (uint8_t)(int)a2;
}

// The square window with a separable spatial mask (a normalised Gaussian is one: ns(m, n) = a_m * a_n), every tap unrolled: the
// column factors enter the exponent (log2 a_n, one scalar per column, loaded once), the row factor multiplies a row's partial
// sums.  The generic kernel above reloads nine spatial weights and waits for them in every row: 169 us per 4K frame against
// this one's ~100.
struct BilateralSepArg {
    float log2_col[kMaxBilateral]; // log2 a_n
    float row[kMaxBilateral];      // a_m
    float c;                       // -log2(e) / (2 sigma_b^2)
};

template <int WW>
__global__ __launch_bounds__(256) void bilateral_fast_sep_kernel(const uint8_t *src3, const uint8_t *gray3, uint8_t *dst3, int w, int h,
                                                                 const BilateralSepArg B)
{
    constexpr int R = WW >> 1, TW = kBilTileW + 2 * R, ROWS = kBilTileH + 2 * R;
    __shared__ float gf[ROWS * TW];
    __shared__ uint32_t spx[ROWS * TW];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kBilTileW, y0 = (int)blockIdx.y * kBilTileH;
    int grey_src = 1;
    for (int i = tid; i < ROWS * TW; i += 256) {
        const int tx = x0 - R + i % TW, ty = y0 - R + i / TW;
        uint32_t px = 0u;
        float g = kBilFastOutside;
        if (tx >= 0 && tx < w && ty >= 0 && ty < h) {
            const size_t q = 3 * ((size_t)ty * w + tx);
            const uint32_t s0 = src3[q], s1 = src3[q + 1], s2 = src3[q + 2], gq = gray3[q];
            px = s0 | (s1 << 8) | (s2 << 16);
            g = (float)gq;
            grey_src &= (s0 == gq && s1 == gq && s2 == gq) ? 1 : 0;
        }
        gf[i] = g;
        spx[i] = px;
    }
    grey_src = __syncthreads_and(grey_src);
    const int lx = tid & 63, ly = tid >> 6, x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const float g0 = gf[(ly + R) * TW + lx + R];
    float wsum = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (grey_src) {
#pragma unroll
        for (int m = 0; m < WW; ++m) {
            const float *grow = gf + (ly + m) * TW + lx;
            float ws = 0.0f, as = 0.0f;
#pragma unroll
            for (int n = 0; n < WW; ++n) {
                const float d = grow[n] - g0;
                const float wgt = __builtin_amdgcn_exp2f(__builtin_fmaf(d * d, B.c, B.log2_col[n]));
                ws += wgt;
                as = __builtin_fmaf(d, wgt, as);
            }
            wsum = __builtin_fmaf(B.row[m], ws, wsum);
            a0 = __builtin_fmaf(B.row[m], as, a0);
        }
        a0 = g0 + a0 / wsum;
        a1 = a2 = a0;
    } else {
#pragma unroll
        for (int m = 0; m < WW; ++m) {
            const float *grow = gf + (ly + m) * TW + lx;
            const uint32_t *prow = spx + (ly + m) * TW + lx;
            float ws = 0.0f, r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
#pragma unroll
            for (int n = 0; n < WW; ++n) {
                const float d = grow[n] - g0;
                const float wgt = __builtin_amdgcn_exp2f(__builtin_fmaf(d * d, B.c, B.log2_col[n]));
                const uint32_t px = prow[n];
                ws += wgt;
                r0 = __builtin_fmaf((float)(px & 0xffu), wgt, r0);
                r1 = __builtin_fmaf((float)((px >> 8) & 0xffu), wgt, r1);
                r2 = __builtin_fmaf((float)((px >> 16) & 0xffu), wgt, r2);
            }
            wsum = __builtin_fmaf(B.row[m], ws, wsum);
            a0 = __builtin_fmaf(B.row[m], r0, a0);
            a1 = __builtin_fmaf(B.row[m], r1, a1);
            a2 = __builtin_fmaf(B.row[m], r2, a2);
        }
        a0 /= wsum;
        a1 /= wsum;
        a2 /= wsum;
    }
    uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
    d[0] = (uint8_t)(int)a0;
    d[1] = (uint8_t)(int)a1;
    d[2] = (uint8_t)(int)a2;
}

// ---- the same +-1 LSB filter with the range weight LOOKED UP in an LDS table (round 4) ------------------------
// bilateral_fast_sep_kernel pays, per tap, six vector instructions of which one is a transcendental (10.1 ns per tap and wave,
// tools/ubench/lds_rates.hip "tap: exponential").  The range weight only depends on the integer |d| = |g_q - g_0|, so a table per
// window column n -- tab[n][i] = a_n * range(i), i = |d| -- turns the tap into: v_sub_f32 (d4 = 4 g_q - 4 g_0: the tile holds 4 g as
// floats, so that ...), v_cvt_u32_f32 |d4| (... the conversion IS the byte offset into the table), ds_read_b32 with the column's
// offset as the instruction's immediate, v_add_f32, v_fma_f32: four vector instructions, none of them slow, and one LDS read.
// (ds_bpermute_b32 out of a table held across the lanes was measured first: 10 ns per permute and SIMD, slower than the
// exponential it replaces -- profiles/r04_ablation.txt batch 9.)  An out-of-image tap is stored as 4 * -256, which puts its |d| at
// 256 ... 511: the table's upper half, all zeros -- no compare, no clamp.  A lane owns a 2 x 2 block of pixels: a tile row's ten
// values arrive as five 8-byte LDS reads and serve the taps of both of its rows.  The tile is loaded four pixels = three dwords at a
// time.  For what main.cu:240 filters: the grey image as its own source (src == gray, one pointer), every channel equal -- checked
// per tile while loading; a tile that fails takes a slow pixel-by-pixel path, still within the tolerance.  No condition on sigma_b:
// the table covers every |d| a byte image has.

template <int WW, int EVERY>
__global__ __launch_bounds__(kLutThreads) void bilateral_lut_kernel(const uint8_t *img3, uint8_t *dst3, int w, int h, const BilateralLutArg B)
{
    constexpr int R = WW >> 1, TW = kLutTileW + 2 * R, NG = (TW + 3) / 4, TWP = NG * 4, ROWS = kLutTileH + 2 * R;
    __shared__ __attribute__((aligned(16))) float g4[ROWS * TWP]; // 4 * grey value, or kLutOutside
    __shared__ __attribute__((aligned(16))) float tab[WW * kLutEntries];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kLutTileW, y0 = (int)blockIdx.y * kLutTileH;
    const int bytes = 3 * w * h; // (below 2 GB: launch_bilateral_lut)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(img3), 0, bytes, 0x00027000);
    uint32_t colour = 0u;
    for (int i = tid; i < ROWS * NG; i += kLutThreads) {
        const int gr = i / NG, gc = i - gr * NG, ty = y0 - R + gr, tx = x0 - R + 4 * gc;
        float g[4] = {kLutOutside, kLutOutside, kLutOutside, kLutOutside};
        if (ty >= 0 && ty < h && tx + 3 >= 0 && tx < w) {
            const int off = 3 * (ty * w + tx);
            if (off >= 0 && off + 12 <= bytes) { // twelve bytes = four pixels in three dwords (a pixel left of column 0 is the end of the row above)
                const uint32_t a = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0), b = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4, 0, 0),
                               c = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 8, 0, 0);
                // what the dwords would hold with every channel equal to channel 0 (of pixels that are real pixels, in the image or a row off)
                colour |= (a ^ __builtin_amdgcn_perm(a, a, 0x03000000u)) | (b ^ __builtin_amdgcn_perm(b, a, 0x06060303u)) |
                          (c ^ __builtin_amdgcn_perm(c, b, 0x05050502u));
                const float v[4] = {(float)(a & 0xffu), (float)(a >> 24), (float)((b >> 16) & 0xffu), (float)((c >> 8) & 0xffu)};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (tx + k >= 0 && tx + k < w) g[k] = 4.0f * v[k];
            } else { // the image's first and last bytes
                for (int k = 0; k < 4; ++k)
                    if (tx + k >= 0 && tx + k < w) {
                        const uint8_t *q = img3 + 3 * ((size_t)ty * w + tx + k);
                        colour |= (uint32_t)(q[0] ^ q[1]) | (uint32_t)(q[0] ^ q[2]);
                        g[k] = 4.0f * (float)q[0];
                    }
            }
        }
        *reinterpret_cast<float4 *>(g4 + gr * TWP + 4 * gc) = float4{g[0], g[1], g[2], g[3]};
    }
    {
        const float rg = tid < 256 ? B.range[tid] : 0.0f; // 512 threads: one entry each, times every column's a_n
#pragma unroll
        for (int n = 0; n < WW; ++n) tab[n * kLutEntries + tid] = B.row[n] * rg;
    }
    const int grey = __syncthreads_and(colour == 0u ? 1 : 0);
    const int lane = tid & 63, wv = tid >> 6;
    if (!grey) { // a tile whose channels differ: the exponential, pixel by pixel, the channels out of global memory
        for (int t = 0; t < 8; ++t) {
            const int lx = 2 * lane + (t & 1), ly = 4 * wv + (t >> 1), x = x0 + lx, y = y0 + ly;
            if (x >= w || y >= h) continue;
            const float g0 = 0.25f * g4[(ly + R) * TWP + lx + R];
            float wsum = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            for (int m = 0; m < WW; ++m) {
                float ws = 0.0f, r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
                for (int n = 0; n < WW; ++n) {
                    const float gq = g4[(ly + m) * TWP + lx + n];
                    if (gq < 0.0f) continue; // outside the image
                    const float d = 0.25f * gq - g0;
                    const float wgt = __builtin_amdgcn_exp2f(__builtin_fmaf(d * d, B.c, B.log2_col[n]));
                    const uint8_t *q = img3 + 3 * ((size_t)(y - R + m) * w + (x - R + n));
                    ws += wgt;
                    r0 = __builtin_fmaf((float)q[0], wgt, r0);
                    r1 = __builtin_fmaf((float)q[1], wgt, r1);
                    r2 = __builtin_fmaf((float)q[2], wgt, r2);
                }
                wsum = __builtin_fmaf(B.row[m], ws, wsum);
                a0 = __builtin_fmaf(B.row[m], r0, a0);
                a1 = __builtin_fmaf(B.row[m], r1, a1);
                a2 = __builtin_fmaf(B.row[m], r2, a2);
            }
            uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
            d[0] = (uint8_t)(int)(a0 / wsum);
            d[1] = (uint8_t)(int)(a1 / wsum);
            d[2] = (uint8_t)(int)(a2 / wsum);
        }
        return;
    }
    const char *tabb = reinterpret_cast<const char *>(tab);
#pragma unroll 1
    for (int pr = 0; pr < 2; ++pr) {
        const int ly = 4 * wv + 2 * pr; // output rows ly, ly + 1 of the tile
        const float2 c0 = *reinterpret_cast<const float2 *>(g4 + (ly + R) * TWP + 2 * lane + R - (R & 1)),
                     c0b = *reinterpret_cast<const float2 *>(g4 + (ly + R) * TWP + 2 * lane + R + (R & 1)),
                     c1 = *reinterpret_cast<const float2 *>(g4 + (ly + 1 + R) * TWP + 2 * lane + R - (R & 1)),
                     c1b = *reinterpret_cast<const float2 *>(g4 + (ly + 1 + R) * TWP + 2 * lane + R + (R & 1));
        const float g00 = (R & 1) ? c0.y : c0.x, g01 = (R & 1) ? c0b.x : c0.y, g10 = (R & 1) ? c1.y : c1.x, g11 = (R & 1) ? c1b.x : c1.y;
        float acc0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc1[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // per output row: wsum A, a A, wsum B, a B
#pragma unroll 1
        for (int t = 0; t <= WW; ++t) { // tile row ly + t: tap row t of output row ly, tap row t - 1 of output row ly + 1
            const float2 *grow = reinterpret_cast<const float2 *>(g4 + (ly + t) * TWP + 2 * lane); // (TWP and 2 * lane are even: 8-byte aligned)
            float v[WW + 1];
#pragma unroll
            for (int k = 0; k < (WW + 1) / 2; ++k) {
                const float2 q = grow[k];
                v[2 * k] = q.x;
                v[2 * k + 1] = q.y;
            }
            if (t < WW) lut_row_taps<WW, EVERY>(v, g00, g01, tabb, B.row[t < WW ? t : 0], acc0, B);
            if (t > 0) lut_row_taps<WW, EVERY>(v, g10, g11, tabb, B.row[t > 0 ? t - 1 : 0], acc1, B);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + ly + r, xA = x0 + 2 * lane;
            if (y >= h || xA >= w) continue;
            const float(&acc)[4] = r ? acc1 : acc0;
            const float gA = r ? g10 : g00, gB = r ? g11 : g01;
            const uint32_t bA = (uint32_t)(int)(0.25f * (gA + acc[1] / acc[0])), bB = (uint32_t)(int)(0.25f * (gB + acc[3] / acc[2])); // g_0 + sum d w / sum w
            uint8_t *d = dst3 + 3 * ((size_t)y * w + xA);
            if (xA + 1 < w) {
                uint16_t *d2 = reinterpret_cast<uint16_t *>(d); // (two-byte stores at any byte address: unaligned access is on for global memory)
                d2[0] = (uint16_t)(bA * 0x0101u), d2[1] = (uint16_t)(bA | (bB << 8)), d2[2] = (uint16_t)(bB * 0x0101u);
            } else {
                d[0] = (uint8_t)bA, d[1] = (uint8_t)bA, d[2] = (uint8_t)bA;
            }
        }
    }
}

template <int WW>
int launch_bilateral_lut(const uint8_t *d_img3, uint8_t *d_dst3, int w, int h, const BilateralLutArg &B, hipStream_t st)
{
    static const int split = [] { const char *e = getenv("OFX_LUT_SPLIT"); return e ? atoi(e) : OFX_LUT_SPLIT_DEFAULT; }();
    // (a computed column gives an out-of-image tap, 256 grey levels or more away, its zero weight by underflow: sigma_b <= ~17)
    const int use = (double)B.c * 65536.0 <= -150.0 ? split : split / 10 * 10;
    const dim3 grid(ofx_div_up(w, kLutTileW), ofx_div_up(h, kLutTileH));
#define OFX_LUT_CASE(S) case S: hipLaunchKernelGGL((bilateral_lut_kernel<WW, S>), grid, dim3(kLutThreads), 0, st, d_img3, d_dst3, w, h, B); break;
    switch (use) {
        OFX_LUT_CASE(0) OFX_LUT_CASE(2) OFX_LUT_CASE(10)
    default: hipLaunchKernelGGL((bilateral_lut_kernel<WW, 12>), grid, dim3(kLutThreads), 0, st, d_img3, d_dst3, w, h, B); break;
    }
#undef OFX_LUT_CASE
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

template <int WW>
int launch_bilateral_fast_sep(const uint8_t *d_src3, const uint8_t *d_gray3, uint8_t *d_dst3, int w, int h, const BilateralSepArg &B, hipStream_t st)
{
    hipLaunchKernelGGL(bilateral_fast_sep_kernel<WW>, dim3(ofx_div_up(w, kBilTileW), ofx_div_up(h, kBilTileH)), dim3(256), 0, st, d_src3, d_gray3,
                       d_dst3, w, h, B);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

template <int WW>
int launch_bilateral_fast(const uint8_t *d_src3, const uint8_t *d_gray3, uint8_t *d_dst3, int w, int h, int wh, const BilateralFastArg &B,
                          hipStream_t st)
{
    const int rows = kBilTileH + 2 * (wh >> 1), tw = kBilTileW + 2 * (WW >> 1);
    const size_t lds = (size_t)rows * tw * (sizeof(float) + sizeof(uint32_t)) + 16;
    hipLaunchKernelGGL(bilateral_fast_kernel<WW>, dim3(ofx_div_up(w, kBilTileW), ofx_div_up(h, kBilTileH)), dim3(256), lds, st, d_src3,
                       d_gray3, d_dst3, w, h, wh, B);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// any window the tiled kernel is not instantiated for: one thread per pixel, taps tested one by one
__global__ __launch_bounds__(256) void bilateral_kernel(const uint8_t *src3, const uint8_t *gray3, uint8_t *dst3, int w, int h,
                                                        int ww, int wh, const BilateralArg B)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int ox = ww >> 1, oy = wh >> 1;
    const int f0 = gray3[3 * ((size_t)y * w + x)];
    double wsum = 0, acc[3] = {0, 0, 0};
    for (int m = 0; m < wh; ++m) {
        const int ty = y - oy + m;
        if (ty < 0 || ty >= h) continue;
        for (int n = 0; n < ww; ++n) {
            const int tx = x - ox + n;
            if (tx < 0 || tx >= w) continue;
            const size_t q = (size_t)ty * w + tx;
            int k = (int)gray3[3 * q] - f0;
            k = k < 0 ? -k : k;
            const double nb = B.range[k];
            const double ns = B.spatial[m * ww + n];
            wsum += nb * ns;
            acc[0] += (double)src3[3 * q] * nb * ns;
            acc[1] += (double)src3[3 * q + 1] * nb * ns;
            acc[2] += (double)src3[3 * q + 2] * nb * ns;
        }
    }
    uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
    d[0] = (uint8_t)(int)(acc[0] / wsum);
    d[1] = (uint8_t)(int)(acc[1] / wsum);
    d[2] = (uint8_t)(int)(acc[2] / wsum);
}

template <int WW>
int launch_bilateral_tiled(const uint8_t *d_src3, const uint8_t *d_gray3, uint8_t *d_dst3, int w, int h, int wh, const BilateralArg &B,
                           hipStream_t st)
{
    const int rows = kBilTileH + 2 * (wh >> 1), tw = kBilTileW + 2 * (WW >> 1);
    const size_t lds = (size_t)kBilLut * sizeof(double) + (size_t)rows * tw * (sizeof(uint32_t) + sizeof(uint16_t)) + 16;
    hipLaunchKernelGGL(bilateral_tiled_kernel<WW>, dim3(ofx_div_up(w, kBilTileW), ofx_div_up(h, kBilTileH)), dim3(256), lds, st, d_src3,
                       d_gray3, d_dst3, w, h, wh, B);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// ---- the remaining functions of namespace cpu (OptFlowCpu.hpp), so that the cpu:: call surface runs on the device too ------

// cpu::sub_arr, OptFlowCPU.cpp:11-17: byte-wise difference, wrapping modulo 256
__global__ __launch_bounds__(256) void sub_u8_kernel(const uint8_t *a, const uint8_t *b, size_t n, uint8_t *dst)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) dst[p] = (uint8_t)(a[p] - b[p]);
}

// cpu::srm_3ch, OptFlowCPU.cpp:202-238: window sum of products per channel.  Its bounds test is `cx > w || cy > h`
// (:222), so a tap one past the right edge reads the first pixel of the next row (pos = cy*w + w) and a tap one past the
// bottom edge reads beyond the image; kept as the reference has it for every position that exists (pos < w*h); taps
// past the end of the buffer -- which the reference reads as whatever follows the allocation -- contribute nothing.
__global__ __launch_bounds__(256) void srm_3ch_kernel(const uint8_t *a3, const uint8_t *b3, int w, int h, int ww, int wh, int32_t *dst3)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int ox = ww >> 1, oy = wh >> 1;
    const size_t n = (size_t)w * (size_t)h;
    int acc[3] = {0, 0, 0};
    for (int p = 0; p < wh; ++p) {
        const int cy = y - oy + p;
        if (cy < 0 || cy > h) continue;
        for (int q = 0; q < ww; ++q) {
            const int cx = x - ox + q;
            if (cx < 0 || cx > w) continue;
            const size_t t = (size_t)cy * w + cx;
            if (t >= n) continue;
            acc[0] += (int)a3[3 * t] * (int)b3[3 * t];
            acc[1] += (int)a3[3 * t + 1] * (int)b3[3 * t + 1];
            acc[2] += (int)a3[3 * t + 2] * (int)b3[3 * t + 2];
        }
    }
    int32_t *d = dst3 + 3 * ((size_t)y * w + x);
    d[0] = acc[0];
    d[1] = acc[1];
    d[2] = acc[2];
}

// cpu::downscale_gaussian, OptFlowCPU.cpp:112-148, with the caller's mask (gpu::gauss_pyramid ignores its mask argument,
// cpu::gauss_pyramid honours it): dst(x,y) = (uchar) sum mask[p][q] * src(2x - mw/2 + q, 2y - mh/2 + p), taps outside the
// (2w x 2h) source skipped, float accumulators in tap order, x86's float -> int -> low byte conversion
__global__ __launch_bounds__(256) void downscale_mask_3ch_kernel(const uint8_t *src3, uint8_t *dst3, int w, int h, const MaskArg M)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int pw = w << 1, ph = h << 1;
    const int sx = (x << 1) - (M.mw >> 1), sy = (y << 1) - (M.mh >> 1);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int p = 0; p < M.mh; ++p) {
        const int cy = sy + p;
        if (cy < 0 || cy >= ph) continue;
        for (int q = 0; q < M.mw; ++q) {
            const int cx = sx + q;
            if (cx < 0 || cx >= pw) continue;
            const uint8_t *s = src3 + 3 * ((size_t)cy * pw + cx);
            const float m = M.m[p * M.mw + q];
            acc[0] += m * (float)s[0];
            acc[1] += m * (float)s[1];
            acc[2] += m * (float)s[2];
        }
    }
    uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
    d[0] = (uint8_t)(int)acc[0];
    d[1] = (uint8_t)(int)acc[1];
    d[2] = (uint8_t)(int)acc[2];
}

// cpu::shift_back_pyramid on the 3-channel image, OptFlowCPU.cpp:241-282.  dst arrives holding whatever the caller's
// buffer held; the first w*h BYTES are overwritten with the source's (the memcpy of :247), then every pixel whose target
// (int)(x + u), (int)(y + v) lies inside the image takes that pixel's three bytes, the others are left alone.
// Two passes (the copy first), because the per-pixel pass reads src only and writes dst only.
__global__ __launch_bounds__(256) void shift_3ch_kernel(const uint8_t *src3, uint8_t *dst3, int w, int h, const float *uv)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const float u = uv[0], v = uv[1];
    // `int new_pos_x = j + u` converts the float sum; x86 turns NaN and out-of-range values into INT_MIN, which the range
    // test rejects -- the same pixels are rejected here by testing the float before converting it
    const float tx = (float)x + u, ty = (float)y + v;
    if (!(tx > -1.0f && tx < (float)w && ty > -1.0f && ty < (float)h)) return;
    const int nx = (int)tx, ny = (int)ty;
    const uint8_t *s = src3 + 3 * ((size_t)ny * w + nx);
    uint8_t *d = dst3 + 3 * ((size_t)y * w + x);
    d[0] = s[0];
    d[1] = s[1];
    d[2] = s[2];
}

inline dim3 grid2d(int w, int h) { return dim3(ofx_div_up(w, 256), h); }

// conv_3ch_1ch_x4_kernel: masks 2 .. 5 wide with finite taps whose int accumulator stays exactly representable in float; images
// below 2 GB.  OFX_CONV_X4=0: the pixel-by-pixel kernel.
bool conv_x4_ok(const MaskArg &M, int w, int h)
{
    static const bool on = [] { const char *e = getenv("OFX_CONV_X4"); return !e || atoi(e) != 0; }();
    if (!on || M.mw < 2 || M.mw > 5 || w < 16 || 3ll * w * h >= (1ll << 31)) return false;
    double sum = 0.0;
    for (int i = 0; i < M.mw * M.mh; ++i) {
        if (!(fabs((double)M.m[i]) < 1e30)) return false;
        sum += fabs((double)M.m[i]);
    }
    return sum * 255.0 < 16777216.0;
}

template <bool F32_OUT>
int launch_conv_x4(const uint8_t *d_src3, int w, int h, void *d_dst, const MaskArg &M, hipStream_t st)
{
    const dim3 grid(ofx_div_up(w, 256), ofx_div_up(h, 4));
    static const bool rows_at_once = [] { const char *e = getenv("OFX_CONV_ROWS"); return !e || atoi(e) != 0; }(); // (0: row by row)
    const dim3 grid_r(ofx_div_up(w, 256), ofx_div_up(h, 4 * kConvRows));
    if (rows_at_once && M.mw == 3 && M.mh == 3) {
        hipLaunchKernelGGL((conv_3ch_1ch_x4_kernel<F32_OUT, 3, 3>), grid_r, dim3(256), 0, st, d_src3, w, h, d_dst, M);
    } else if (rows_at_once && M.mw == 5 && M.mh == 5) {
        hipLaunchKernelGGL((conv_3ch_1ch_x4_kernel<F32_OUT, 5, 5>), grid_r, dim3(256), 0, st, d_src3, w, h, d_dst, M);
    } else
    switch (M.mw) {
    case 2: hipLaunchKernelGGL((conv_3ch_1ch_x4_kernel<F32_OUT, 2>), grid, dim3(256), 0, st, d_src3, w, h, d_dst, M); break;
    case 3: hipLaunchKernelGGL((conv_3ch_1ch_x4_kernel<F32_OUT, 3>), grid, dim3(256), 0, st, d_src3, w, h, d_dst, M); break;
    case 4: hipLaunchKernelGGL((conv_3ch_1ch_x4_kernel<F32_OUT, 4>), grid, dim3(256), 0, st, d_src3, w, h, d_dst, M); break;
    default: hipLaunchKernelGGL((conv_3ch_1ch_x4_kernel<F32_OUT, 5>), grid, dim3(256), 0, st, d_src3, w, h, d_dst, M); break;
    }
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

} // namespace

extern "C" int ofx_sub_u8(const uint8_t *d_a, const uint8_t *d_b, size_t n, uint8_t *d_dst, void *stream)
{
    OFX_REQUIRE(d_a && d_b && d_dst, "ofx_sub_u8: null pointer");
    if (n == 0) return OFX_OK;
    hipLaunchKernelGGL(sub_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ofx_stream(stream), d_a, d_b, n, d_dst);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_srm_3ch_u8(const uint8_t *d_a3, const uint8_t *d_b3, int w, int h, int ww, int wh, int32_t *d_dst3, void *stream)
{
    OFX_REQUIRE(d_a3 && d_b3 && d_dst3 && w > 0 && h > 0 && ww > 0 && wh > 0, "ofx_srm_3ch_u8: bad arguments");
    hipLaunchKernelGGL(srm_3ch_kernel, grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_a3, d_b3, w, h, ww, wh, d_dst3);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_downscale_mask_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int dw, int dh, const float *h_mask, int mw, int mh,
                                      void *stream)
{
    OFX_REQUIRE(d_src3 && d_dst3 && dw > 0 && dh > 0, "ofx_downscale_mask_3ch: bad arguments");
    MaskArg M;
    OFX_TRY(make_mask(h_mask, mw, mh, &M, "ofx_downscale_mask_3ch"));
    hipLaunchKernelGGL(downscale_mask_3ch_kernel, grid2d(dw, dh), dim3(256), 0, ofx_stream(stream), d_src3, d_dst3, dw, dh, M);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_shift_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int w, int h, const float *d_uv, void *stream)
{
    OFX_REQUIRE(d_src3 && d_dst3 && d_uv && w > 0 && h > 0, "ofx_shift_3ch: bad arguments");
    OFX_REQUIRE(d_src3 != d_dst3, "ofx_shift_3ch: in-place shift is not defined");
    OFX_HIP(hipMemcpyAsync(d_dst3, d_src3, (size_t)w * (size_t)h, hipMemcpyDeviceToDevice, ofx_stream(stream))); // w*h BYTES, :247
    hipLaunchKernelGGL(shift_3ch_kernel, grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_src3, d_dst3, w, h, d_uv);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// utils::generate_gaussian_kernel, OptFlowUtils.cpp:68-114 (host side, double)
extern "C" void ofx_generate_gaussian_kernel(double sigma_s, int ks, double *dst)
{
    if (ks == -1) ks = (int)(2.0 * M_PI * sigma_s);
    if (ks % 2 == 0) ks += 1;
    const int c = ks >> 1;
    const double s2 = sigma_s * sigma_s;
    for (int i = 0; i < ks; ++i)
        for (int j = 0; j < ks; ++j) {
            const double m = (double)(i > c ? i - c : c - i), n = (double)(j > c ? j - c : c - j);
            dst[i * ks + j] = 1.0 / (2.0 * M_PI * s2) * pow(M_E, -0.5 * (n * n + m * m) / s2);
        }
    double sum = 0;
    for (int i = 0; i < ks * ks; ++i) sum += dst[i];
    for (int i = 0; i < ks * ks; ++i) dst[i] /= sum;
}

extern "C" int ofx_grayscale_avg_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int w, int h, void *stream)
{
    OFX_REQUIRE(d_src3 && d_dst3 && w > 0 && h > 0, "ofx_grayscale_avg_3ch: bad arguments");
    const size_t n = (size_t)w * (size_t)h;
    size_t done = 0;
    if ((((uintptr_t)d_src3 | (uintptr_t)d_dst3) & 15) == 0 && n >= 16) { // sixteen pixels per thread; the last n % 16 pixels below
        const size_t n16 = n / 16;
        hipLaunchKernelGGL(gray_x16_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, ofx_stream(stream), reinterpret_cast<const uint32_t *>(d_src3),
                           reinterpret_cast<uint32_t *>(d_dst3), n16);
        OFX_HIP(hipGetLastError());
        done = 16 * n16;
    }
    if (done < n) {
        hipLaunchKernelGGL(gray_kernel, dim3((unsigned)((n - done + 255) / 256)), dim3(256), 0, ofx_stream(stream), d_src3 + 3 * done, d_dst3 + 3 * done,
                           n - done);
        OFX_HIP(hipGetLastError());
    }
    return OFX_OK;
}

extern "C" int ofx_conv_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int w, int h, const float *h_mask, int mw, int mh,
                            int float_acc, void *stream)
{
    OFX_REQUIRE(d_src3 && d_dst3 && w > 0 && h > 0, "ofx_conv_3ch: bad arguments");
    MaskArg M;
    OFX_TRY(make_mask(h_mask, mw, mh, &M, "ofx_conv_3ch"));
    if (float_acc)
        hipLaunchKernelGGL(conv_3ch_kernel<true>, grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_src3, d_dst3, w, h, M);
    else
        hipLaunchKernelGGL(conv_3ch_kernel<false>, grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_src3, d_dst3, w, h, M);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_conv_3ch_1ch_u8(const uint8_t *d_src3, int w, int h, uint8_t *d_dst, const float *h_mask, int mw, int mh,
                                   void *stream)
{
    OFX_REQUIRE(d_src3 && d_dst && w > 0 && h > 0, "ofx_conv_3ch_1ch_u8: bad arguments");
    MaskArg M;
    OFX_TRY(make_mask(h_mask, mw, mh, &M, "ofx_conv_3ch_1ch_u8"));
    if (conv_x4_ok(M, w, h)) return launch_conv_x4<false>(d_src3, w, h, (void *)d_dst, M, ofx_stream(stream));
    hipLaunchKernelGGL(conv_3ch_1ch_kernel<false>, grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_src3, w, h, (void *)d_dst, M);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_conv_3ch_1ch_f32(const uint8_t *d_src3, int w, int h, float *d_dst, const float *h_mask, int mw, int mh,
                                    void *stream)
{
    OFX_REQUIRE(d_src3 && d_dst && w > 0 && h > 0, "ofx_conv_3ch_1ch_f32: bad arguments");
    MaskArg M;
    OFX_TRY(make_mask(h_mask, mw, mh, &M, "ofx_conv_3ch_1ch_f32"));
    if (conv_x4_ok(M, w, h)) return launch_conv_x4<true>(d_src3, w, h, (void *)d_dst, M, ofx_stream(stream));
    hipLaunchKernelGGL(conv_3ch_1ch_kernel<true>, grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_src3, w, h, (void *)d_dst, M);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// srm_march.hip: the same sums on the march (sliding integer windows / products formed once); OFX_E_UNSUPPORTED = not their shape
int ofx_srm_u8_march(const uint8_t *d_a, const uint8_t *d_b, int w, int h, int ww, int wh, int32_t *d_dst, hipStream_t st);
int ofx_srm_f32_march(const float *d_a, const float *d_b, int w, int h, int ww, int wh, float *d_dst, hipStream_t st);
static bool srm_march_on()
{
    static const bool on = [] { const char *e = getenv("OFX_SRM_MARCH"); return !e || atoi(e) != 0; }();
    return on;
}

extern "C" int ofx_srm_u8(const uint8_t *d_a, const uint8_t *d_b, int w, int h, int ww, int wh, int32_t *d_dst, void *stream)
{
    OFX_REQUIRE(d_a && d_b && d_dst && w > 0 && h > 0 && ww > 0 && wh > 0, "ofx_srm_u8: bad arguments");
    if (srm_march_on()) {
        const int rc = ofx_srm_u8_march(d_a, d_b, w, h, ww, wh, d_dst, ofx_stream(stream));
        if (rc != OFX_E_UNSUPPORTED) return rc;
    }
    hipLaunchKernelGGL((srm_kernel<uint8_t, int32_t>), grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_a, d_b, w, h, ww, wh, d_dst);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_srm_f32(const float *d_a, const float *d_b, int w, int h, int ww, int wh, float *d_dst, void *stream)
{
    OFX_REQUIRE(d_a && d_b && d_dst && w > 0 && h > 0 && ww > 0 && wh > 0, "ofx_srm_f32: bad arguments");
    if (srm_march_on()) {
        const int rc = ofx_srm_f32_march(d_a, d_b, w, h, ww, wh, d_dst, ofx_stream(stream));
        if (rc != OFX_E_UNSUPPORTED) return rc;
    }
    hipLaunchKernelGGL((srm_kernel<float, float>), grid2d(w, h), dim3(256), 0, ofx_stream(stream), d_a, d_b, w, h, ww, wh, d_dst);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_solve_i32(const int32_t *d_sxx, const int32_t *d_syy, const int32_t *d_sxy, const int32_t *d_sxt,
                             const int32_t *d_syt, float *d_flow, int w, int h, int variant, void *stream)
{
    OFX_REQUIRE(d_sxx && d_syy && d_sxy && d_sxt && d_syt && d_flow && w > 0 && h > 0, "ofx_solve_i32: bad arguments");
    OFX_REQUIRE(variant >= 0 && variant <= 2, "ofx_solve_i32: bad variant %d", variant);
    const size_t n = (size_t)w * (size_t)h;
    hipLaunchKernelGGL(solve_kernel<int32_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ofx_stream(stream), d_sxx, d_syy,
                       d_sxy, d_sxt, d_syt, d_flow, n, variant);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_solve_f32(const float *d_sxx, const float *d_syy, const float *d_sxy, const float *d_sxt, const float *d_syt,
                             float *d_flow, int w, int h, void *stream)
{
    OFX_REQUIRE(d_sxx && d_syy && d_sxy && d_sxt && d_syt && d_flow && w > 0 && h > 0, "ofx_solve_f32: bad arguments");
    const size_t n = (size_t)w * (size_t)h;
    hipLaunchKernelGGL(solve_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ofx_stream(stream), d_sxx, d_syy,
                       d_sxy, d_sxt, d_syt, d_flow, n, (int)OFX_SOLVE_F64);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// Process-wide switch of the host-pointer wrappers gpu::bilinear_filter / cpu::bilinear_filter_3ch (their signatures are the
// reference's and carry no mode): 0 = the bit-exact kernel (default), 1 = ofx_bilateral_3ch_fast.  Environment
// OFX_BILATERAL_FAST=1 sets the initial value.
static int g_bilateral_fast = [] { const char *e = getenv("OFX_BILATERAL_FAST"); return e && atoi(e) > 0 ? 1 : 0; }();
extern "C" int ofx_bilateral_wrappers_fast(int on)
{
    const int before = g_bilateral_fast;
    if (on >= 0) g_bilateral_fast = on ? 1 : 0;
    return before;
}

extern "C" int ofx_bilateral_3ch_fast(const uint8_t *d_src3, const uint8_t *d_gray3, uint8_t *d_dst3, int w, int h, int ww, int wh,
                                      double sigma_s, double sigma_b, void *stream)
{
    OFX_REQUIRE(d_src3 && d_gray3 && d_dst3 && w > 0 && h > 0, "ofx_bilateral_3ch_fast: bad arguments");
    OFX_REQUIRE(ww > 0 && wh > 0 && (ww & 1) && (wh & 1) && ww <= kMaxBilateral && wh <= ww && sigma_b > 0.0 && sigma_s > 0.0,
                "ofx_bilateral_3ch_fast: window %dx%d unsupported (odd ww <= %d, odd wh <= ww)", ww, wh, kMaxBilateral);
    // (with a very wide range Gaussian the sentinel of the out-of-image taps would no longer underflow to a zero weight)
    if (sigma_b > 2.0e4) return ofx_bilateral_3ch(d_src3, d_gray3, d_dst3, w, h, ww, wh, sigma_s, sigma_b, stream);
    static thread_local BilateralFastArg B;
    double sp[kMaxBilateral * kMaxBilateral];
    ofx_generate_gaussian_kernel(sigma_s, ww, sp);
    for (int i = 0; i < ww * ww; ++i) B.log2_spatial[i] = (float)log2(sp[i]);
    B.c = (float)(-M_LOG2E / (2.0 * sigma_b * sigma_b));
    hipStream_t st = ofx_stream(stream);
    if (wh == ww) {
        // a square window whose mask is separable (ns(m, n) = a_m a_n with a_n = ns(c, n) / sqrt(ns(c, c)), c the centre --
        // checked, not assumed): the unrolled kernel
        static thread_local BilateralSepArg S;
        if (bilateral_sep_rows(sp, ww, S.row, S.log2_col)) {
            S.c = B.c;
            // the grey image as its own source (main.cu:240): the range weight out of an LDS table instead of the exponential
            // (OFX_BILATERAL_LUT=0: always the exponential)
            static const bool lut_on = [] { const char *e = getenv("OFX_BILATERAL_LUT"); return !e || atoi(e) != 0; }();
            if (lut_on && d_src3 == d_gray3 && 3ll * w * h + 16 < (1ll << 31)) {
                static thread_local BilateralLutArg T;
                for (int n = 0; n < ww; ++n) {
                    T.row[n] = S.row[n];
                    T.log2_col[n] = S.log2_col[n];
                }
                bilateral_lut_range(B.c, &T);
                switch (ww) {
                case 3: return launch_bilateral_lut<3>(d_gray3, d_dst3, w, h, T, st);
                case 5: return launch_bilateral_lut<5>(d_gray3, d_dst3, w, h, T, st);
                case 7: return launch_bilateral_lut<7>(d_gray3, d_dst3, w, h, T, st);
                case 9: return launch_bilateral_lut<9>(d_gray3, d_dst3, w, h, T, st);
                case 11: return launch_bilateral_lut<11>(d_gray3, d_dst3, w, h, T, st);
                default: return launch_bilateral_lut<13>(d_gray3, d_dst3, w, h, T, st);
                }
            }
            switch (ww) {
            case 3: return launch_bilateral_fast_sep<3>(d_src3, d_gray3, d_dst3, w, h, S, st);
            case 5: return launch_bilateral_fast_sep<5>(d_src3, d_gray3, d_dst3, w, h, S, st);
            case 7: return launch_bilateral_fast_sep<7>(d_src3, d_gray3, d_dst3, w, h, S, st);
            case 9: return launch_bilateral_fast_sep<9>(d_src3, d_gray3, d_dst3, w, h, S, st);
            case 11: return launch_bilateral_fast_sep<11>(d_src3, d_gray3, d_dst3, w, h, S, st);
            default: return launch_bilateral_fast_sep<13>(d_src3, d_gray3, d_dst3, w, h, S, st);
            }
        }
    }
    switch (ww) {
    case 3: return launch_bilateral_fast<3>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
    case 5: return launch_bilateral_fast<5>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
    case 7: return launch_bilateral_fast<7>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
    case 9: return launch_bilateral_fast<9>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
    case 11: return launch_bilateral_fast<11>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
    default: return launch_bilateral_fast<13>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
    }
}

extern "C" int ofx_bilateral_3ch(const uint8_t *d_src3, const uint8_t *d_gray3, uint8_t *d_dst3, int w, int h, int ww, int wh,
                                 double sigma_s, double sigma_b, void *stream)
{
    OFX_REQUIRE(d_src3 && d_gray3 && d_dst3 && w > 0 && h > 0, "ofx_bilateral_3ch: bad arguments");
    OFX_REQUIRE(ww > 0 && wh > 0 && (ww & 1) && ww <= kMaxBilateral && wh <= ww,
                "ofx_bilateral_3ch: window %dx%d unsupported (odd ww <= %d, wh <= ww; the spatial mask is ww x ww, "
                "OptFlowCPU.cpp:404)", ww, wh, kMaxBilateral);
    static thread_local BilateralArg B;
    bilateral_exact_tables(sigma_s, sigma_b, ww, &B);
    hipStream_t st = ofx_stream(stream);
    // the image as its own grey image, square window (main.cu:240): one LDS read per tap (OFX_BILATERAL_OWN=0: the general kernel)
    static const bool own_on = [] { const char *e = getenv("OFX_BILATERAL_OWN"); return !e || atoi(e) != 0; }();
    if (own_on && d_src3 == d_gray3 && wh == ww && 3ll * w * h + 16 < (1ll << 31)) {
        switch (ww) {
        case 3: return launch_bilateral_exact_own<3>(d_gray3, d_dst3, w, h, B, st);
        case 5: return launch_bilateral_exact_own<5>(d_gray3, d_dst3, w, h, B, st);
        case 7: return launch_bilateral_exact_own<7>(d_gray3, d_dst3, w, h, B, st);
        case 9: return launch_bilateral_exact_own<9>(d_gray3, d_dst3, w, h, B, st);
        case 11: return launch_bilateral_exact_own<11>(d_gray3, d_dst3, w, h, B, st);
        case 13: return launch_bilateral_exact_own<13>(d_gray3, d_dst3, w, h, B, st);
        default: break;
        }
    }
    if (wh == ww || (wh & 1)) { // (the tiled kernel centres the rows on wh / 2 like the reference; any wh <= ww works)
        switch (ww) {
        case 3: return launch_bilateral_tiled<3>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
        case 5: return launch_bilateral_tiled<5>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
        case 7: return launch_bilateral_tiled<7>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
        case 9: return launch_bilateral_tiled<9>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
        case 11: return launch_bilateral_tiled<11>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
        case 13: return launch_bilateral_tiled<13>(d_src3, d_gray3, d_dst3, w, h, wh, B, st);
        default: break;
        }
    }
    hipLaunchKernelGGL(bilateral_kernel, grid2d(w, h), dim3(256), 0, st, d_src3, d_gray3, d_dst3, w, h, ww, wh, B);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
