// Affine frame warp (the definition: "affine frame warp" in include/ofx.h): a u8 frame of 1 or 3 interleaved channels resampled
// through a float64 [6] inverse map that the host quantises to 2^-21; positions are exact int64, on the tracker's 1/32 px lattice,
// the value is the tracker's bilinear sum, so the result is the same bits on any device.  ONE launch for up to
// OFX_STREAM_MAX_BATCH items of any sizes: a lane makes four adjacent output pixels of a row -- the geometry of a pixel once for all
// its channels, every tap clamped before it becomes an address -- and stores them as dwords where the address allows and the
// quad is whole, as bytes otherwise.  The pixels out of range are counted per lane, summed per wave and per block, and leave as
// one integer atomic per block.
#include <math.h>
#include <string.h>

#include "ofx_internal.h"
#include "warp_pixel.h"

namespace {

constexpr int kThreads = 256, kQuad = kWarpQuad;
constexpr int kMaxSize = 1 << 16;
constexpr int kShift = 21; // the model's fixed point; a position in 1/32 px is (.. + 2^15) >> 16

struct WarpItem {
    const uint8_t *src;
    uint8_t *dst;
    unsigned long long *outside;
    long long a, b, tx, c, d, ty;
    int src_pitch, sw, sh, dst_pitch, w, h, channels, border, fill;
    unsigned quads_per_row, quads;
};
struct WarpArgs {
    WarpItem item[OFX_STREAM_MAX_BATCH];
};

template <int C> __device__ __forceinline__ unsigned warp_quad(const WarpItem &it, unsigned g)
{
    const int y = (int)(g / it.quads_per_row), x0 = kQuad * (int)(g - (unsigned)y * it.quads_per_row);
    long long px = it.a * x0 + it.b * y + it.tx + 32768, py = it.c * x0 + it.d * y + it.ty + 32768;
    auto pos = [&it, px, py](int, long long &qx, long long &qy) mutable {
        qx = px >> 16, qy = py >> 16;
        px += it.a, py += it.c;
        return true;
    };
    return warp_quad_at<C>(it, y, x0, pos);
}

__global__ __launch_bounds__(kThreads) void warp_affine_kernel(const WarpArgs A)
{
    const WarpItem &it = A.item[blockIdx.y];
    const unsigned base = blockIdx.x * kThreads;
    if (base >= it.quads) return; // (block-uniform: the grid is sized for the launch's largest item)
    __shared__ unsigned block_out;
    if (threadIdx.x == 0) block_out = 0u;
    __syncthreads();
    const unsigned g = base + threadIdx.x;
    unsigned out = 0;
    if (g < it.quads) out = it.channels == 3 ? warp_quad<3>(it, g) : warp_quad<1>(it, g);
    if (it.outside == nullptr) return; // (block-uniform)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) out += __shfl_xor(out, s, 64);
    if ((threadIdx.x & 63) == 0 && out) atomicAdd(&block_out, out);
    __syncthreads();
    if (threadIdx.x == 0 && block_out) atomicAdd(it.outside, (unsigned long long)block_out); // (zeroed on the stream before the launch)
}

} // namespace

extern "C" int ofx_warp_affine(const ofx_warp_affine_desc *items, int n, void *stream)
{
    const char *who = "ofx_warp_affine";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    static thread_local WarpArgs A;
    memset(&A, 0, sizeof A);
    unsigned max_quads = 0;
    for (int i = 0; i < n; ++i) {
        const ofx_warp_affine_desc &d = items[i];
        OFX_REQUIRE(d.d_src != nullptr && d.d_dst != nullptr, "%s: item %d: d_src or d_dst is null", who, i);
        OFX_REQUIRE(d.channels == 1 || d.channels == 3, "%s: item %d: channels = %d is not 1 or 3", who, i, d.channels);
        OFX_REQUIRE(d.border == OFX_BORDER_CONSTANT || d.border == OFX_BORDER_REPLICATE, "%s: item %d: border = %d is not 0 or 1", who, i, d.border);
        OFX_REQUIRE(d.fill >= 0 && d.fill <= 255, "%s: item %d: fill = %d is not in 0 .. 255", who, i, d.fill);
        OFX_REQUIRE(d.w >= 1 && d.w <= kMaxSize && d.h >= 1 && d.h <= kMaxSize, "%s: item %d: the size %d x %d is not in 1 .. 2^16", who, i, d.w, d.h);
        OFX_REQUIRE(d.sw >= 1 && d.sw <= kMaxSize && d.sh >= 1 && d.sh <= kMaxSize, "%s: item %d: the source size %d x %d is not in 1 .. 2^16", who, i, d.sw,
                    d.sh);
        OFX_REQUIRE(d.dst_pitch >= d.channels * d.w, "%s: item %d: dst_pitch = %d is below %d", who, i, d.dst_pitch, d.channels * d.w);
        OFX_REQUIRE(d.src_pitch >= d.channels * d.sw, "%s: item %d: src_pitch = %d is below %d", who, i, d.src_pitch, d.channels * d.sw);
        long long q[6];
        for (int k = 0; k < 6; ++k) {
            const double lim = (k == 2 || k == 5) ? 1048576.0 : 16.0;
            OFX_REQUIRE(__builtin_isfinite(d.model[k]) && fabs(d.model[k]) <= lim, "%s: item %d: model[%d] is not finite or above %s in magnitude", who, i, k,
                        lim == 16.0 ? "16" : "2^20");
            q[k] = llrint(ldexp(d.model[k], kShift)); // (ties to even: the default rounding mode)
        }
        const uintptr_t s0 = (uintptr_t)d.d_src, s1 = s0 + (size_t)(d.sh - 1) * (size_t)d.src_pitch + (size_t)(d.channels * d.sw);
        const uintptr_t t0 = (uintptr_t)d.d_dst, t1 = t0 + (size_t)(d.h - 1) * (size_t)d.dst_pitch + (size_t)(d.channels * d.w);
        OFX_REQUIRE(s1 <= t0 || t1 <= s0, "%s: item %d: d_src and d_dst overlap", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_outside & 7) == 0, "%s: item %d: d_outside must be 8-byte aligned", who, i);
        WarpItem &it = A.item[i];
        it.src = d.d_src, it.dst = d.d_dst, it.outside = reinterpret_cast<unsigned long long *>(d.d_outside);
        it.a = q[0], it.b = q[1], it.tx = q[2], it.c = q[3], it.d = q[4], it.ty = q[5];
        it.src_pitch = d.src_pitch, it.sw = d.sw, it.sh = d.sh, it.dst_pitch = d.dst_pitch, it.w = d.w, it.h = d.h;
        it.channels = d.channels, it.border = d.border, it.fill = d.fill;
        it.quads_per_row = (unsigned)ofx_div_up(d.w, kQuad);
        it.quads = it.quads_per_row * (unsigned)d.h; // (at most 2^14 * 2^16)
        max_quads = it.quads > max_quads ? it.quads : max_quads;
    }
    hipStream_t st = ofx_stream(stream);
    for (int i = 0; i < n; ++i)
        if (items[i].d_outside) OFX_TRY(ofx_zero_words(items[i].d_outside, 1, st));
    hipLaunchKernelGGL(warp_affine_kernel, dim3((max_quads + kThreads - 1) / kThreads, n), dim3(kThreads), 0, st, A);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
