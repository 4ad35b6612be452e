// Perspective frame warp (the definition: "perspective frame warp" in include/ofx.h): a u8 frame of 1 or 3 interleaved channels
// resampled through a float64 [9] inverse homography.  The position of an output pixel is three float64 dot products, ONE
// reciprocal and two products, each rounded once (the build has -ffp-contract=off: nothing below is fused), then rounded to the
// tracker's 1/32 px lattice; from there on the pixel is ofx_warp_affine's (warp_pixel.h), so the result is the same bits on any
// device.  ONE launch for up to OFX_STREAM_MAX_BATCH items of any sizes: a lane makes four adjacent output pixels of a row -- X, Y
// and W of each from its own x, never by accumulation, the geometry of a pixel once for all its channels, every tap clamped before
// it becomes an address -- and stores them as dwords where the address allows and the quad is whole, as bytes otherwise.  The
// pixels out of range or undefined are counted per lane, summed per wave and per block, and leave as one integer atomic per block.
// Also here: the host-only helpers ofx_homography_compose, _invert, _normalize and _from_affine.
#include <math.h>
#include <string.h>

#include "ofx_internal.h"
#include "warp_pixel.h"

namespace {

constexpr int kThreads = 256, kQuad = kWarpQuad;
constexpr int kMaxSize = 1 << 16;
constexpr double kMaxPos = 1099511627776.0; // 2^40: a position beyond it, in 1/32 px, is UNDEFINED

struct PerspItem {
    const uint8_t *src;
    uint8_t *dst;
    unsigned long long *outside;
    double m[9];
    int src_pitch, sw, sh, dst_pitch, w, h, channels, border, fill;
    unsigned quads_per_row, quads;
};
struct PerspArgs {
    PerspItem item[OFX_STREAM_MAX_BATCH];
};

template <int C> __device__ __forceinline__ unsigned persp_quad(const PerspItem &it, unsigned g)
{
    const int y = (int)(g / it.quads_per_row), x0 = kQuad * (int)(g - (unsigned)y * it.quads_per_row);
    const double yd = (double)y;
    auto pos = [&](int k, long long &qx, long long &qy) {
        const double xd = (double)(x0 + k);
        const double X = (it.m[0] * xd + it.m[1] * yd) + it.m[2], Y = (it.m[3] * xd + it.m[4] * yd) + it.m[5], W = (it.m[6] * xd + it.m[7] * yd) + it.m[8];
        const double r = 1.0 / W;
        const double fx = (X * r) * 32.0, fy = (Y * r) * 32.0; // (ldexp(., 5): the product by 2^5 is exact, or infinite as ldexp's)
        const bool defined = W > 0.0 && fabs(fx) <= kMaxPos && fabs(fy) <= kMaxPos; // (false for a NaN or an infinity)
        qx = defined ? __double2ll_rn(fx) : 0ll, qy = defined ? __double2ll_rn(fy) : 0ll; // (ties to even; 0: any address stays in the source)
        return defined;
    };
    return warp_quad_at<C>(it, y, x0, pos);
}

__global__ __launch_bounds__(kThreads) void warp_persp_kernel(const PerspArgs A)
{
    const PerspItem &it = A.item[blockIdx.y];
    const unsigned base = blockIdx.x * kThreads;
    if (base >= it.quads) return; // (block-uniform: the grid is sized for the launch's largest item)
    __shared__ unsigned block_out;
    if (threadIdx.x == 0) block_out = 0u;
    __syncthreads();
    const unsigned g = base + threadIdx.x;
    unsigned out = 0;
    if (g < it.quads) out = it.channels == 3 ? persp_quad<3>(it, g) : persp_quad<1>(it, g);
    if (it.outside == nullptr) return; // (block-uniform)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) out += __shfl_xor(out, s, 64);
    if ((threadIdx.x & 63) == 0 && out) atomicAdd(&block_out, out);
    __syncthreads();
    if (threadIdx.x == 0 && block_out) atomicAdd(it.outside, (unsigned long long)block_out); // (zeroed on the stream before the launch)
}

} // namespace

extern "C" int ofx_warp_perspective(const ofx_warp_persp_desc *items, int n, void *stream)
{
    const char *who = "ofx_warp_perspective";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    static thread_local PerspArgs A;
    memset(&A, 0, sizeof A);
    unsigned max_quads = 0;
    for (int i = 0; i < n; ++i) {
        const ofx_warp_persp_desc &d = items[i];
        OFX_REQUIRE(d.d_src != nullptr && d.d_dst != nullptr, "%s: item %d: d_src or d_dst is null", who, i);
        OFX_REQUIRE(d.channels == 1 || d.channels == 3, "%s: item %d: channels = %d is not 1 or 3", who, i, d.channels);
        OFX_REQUIRE(d.border == OFX_BORDER_CONSTANT || d.border == OFX_BORDER_REPLICATE, "%s: item %d: border = %d is not 0 or 1", who, i, d.border);
        OFX_REQUIRE(d.fill >= 0 && d.fill <= 255, "%s: item %d: fill = %d is not in 0 .. 255", who, i, d.fill);
        OFX_REQUIRE(d.w >= 1 && d.w <= kMaxSize && d.h >= 1 && d.h <= kMaxSize, "%s: item %d: the size %d x %d is not in 1 .. 2^16", who, i, d.w, d.h);
        OFX_REQUIRE(d.sw >= 1 && d.sw <= kMaxSize && d.sh >= 1 && d.sh <= kMaxSize, "%s: item %d: the source size %d x %d is not in 1 .. 2^16", who, i, d.sw,
                    d.sh);
        OFX_REQUIRE(d.dst_pitch >= d.channels * d.w, "%s: item %d: dst_pitch = %d is below %d", who, i, d.dst_pitch, d.channels * d.w);
        OFX_REQUIRE(d.src_pitch >= d.channels * d.sw, "%s: item %d: src_pitch = %d is below %d", who, i, d.src_pitch, d.channels * d.sw);
        for (int k = 0; k < 9; ++k) {
            const double lim = (k == 2 || k == 5) ? 1048576.0 : (k == 6 || k == 7) ? 1.0 : 16.0;
            OFX_REQUIRE(__builtin_isfinite(d.model[k]) && fabs(d.model[k]) <= lim, "%s: item %d: model[%d] is not finite or above %s in magnitude", who, i, k,
                        lim == 16.0 ? "16" : lim == 1.0 ? "1" : "2^20");
        }
        const uintptr_t s0 = (uintptr_t)d.d_src, s1 = s0 + (size_t)(d.sh - 1) * (size_t)d.src_pitch + (size_t)(d.channels * d.sw);
        const uintptr_t t0 = (uintptr_t)d.d_dst, t1 = t0 + (size_t)(d.h - 1) * (size_t)d.dst_pitch + (size_t)(d.channels * d.w);
        OFX_REQUIRE(s1 <= t0 || t1 <= s0, "%s: item %d: d_src and d_dst overlap", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_outside & 7) == 0, "%s: item %d: d_outside must be 8-byte aligned", who, i);
        PerspItem &it = A.item[i];
        it.src = d.d_src, it.dst = d.d_dst, it.outside = reinterpret_cast<unsigned long long *>(d.d_outside);
        for (int k = 0; k < 9; ++k) it.m[k] = d.model[k];
        it.src_pitch = d.src_pitch, it.sw = d.sw, it.sh = d.sh, it.dst_pitch = d.dst_pitch, it.w = d.w, it.h = d.h;
        it.channels = d.channels, it.border = d.border, it.fill = d.fill;
        it.quads_per_row = (unsigned)ofx_div_up(d.w, kQuad);
        it.quads = it.quads_per_row * (unsigned)d.h; // (at most 2^14 * 2^16)
        max_quads = it.quads > max_quads ? it.quads : max_quads;
    }
    hipStream_t st = ofx_stream(stream);
    for (int i = 0; i < n; ++i)
        if (items[i].d_outside) OFX_TRY(ofx_zero_words(items[i].d_outside, 1, st));
    hipLaunchKernelGGL(warp_persp_kernel, dim3((max_quads + kThreads - 1) / kThreads, n), dim3(kThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_homography_compose(const double *m2, const double *m1, double *out)
{
    OFX_REQUIRE(m2 != nullptr && m1 != nullptr && out != nullptr, "ofx_homography_compose: m2, m1 or out is null");
    double r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[3 * i + j] = (m2[3 * i] * m1[j] + m2[3 * i + 1] * m1[3 + j]) + m2[3 * i + 2] * m1[6 + j];
    memcpy(out, r, sizeof r);
    return OFX_OK;
}

extern "C" int ofx_homography_invert(const double *m, double *out)
{
    OFX_REQUIRE(m != nullptr && out != nullptr, "ofx_homography_invert: m or out is null");
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double c0 = e * i - f * h, c1 = f * g - d * i, c2 = d * h - e * g;
    const double det = (a * c0 + b * c1) + c * c2;
    OFX_REQUIRE(det != 0.0 && __builtin_isfinite(det), "ofx_homography_invert: the determinant is 0 or not finite");
    const double r[9] = {c0 / det, (c * h - b * i) / det, (b * f - c * e) / det, c1 / det, (a * i - c * g) / det, (c * d - a * f) / det,
                         c2 / det, (b * g - a * h) / det, (a * e - b * d) / det};
    memcpy(out, r, sizeof r);
    return OFX_OK;
}

extern "C" int ofx_homography_normalize(const double *m, double *out)
{
    OFX_REQUIRE(m != nullptr && out != nullptr, "ofx_homography_normalize: m or out is null");
    const double s = m[8];
    OFX_REQUIRE(s != 0.0 && __builtin_isfinite(s), "ofx_homography_normalize: entry 8 is 0 or not finite");
    for (int k = 0; k < 9; ++k) out[k] = m[k] / s;
    return OFX_OK;
}

extern "C" int ofx_homography_from_affine(const double *m6, double *out)
{
    OFX_REQUIRE(m6 != nullptr && out != nullptr, "ofx_homography_from_affine: m6 or out is null");
    const double r[9] = {m6[0], m6[1], m6[2], m6[3], m6[4], m6[5], 0.0, 0.0, 1.0};
    memcpy(out, r, sizeof r);
    return OFX_OK;
}
