// The stream pipeline's output stage (ofx_session_stream_compose): the dense field of main.cu:138-147 for every pair one
// call of the pipeline completes, in ONE launch, into the caller's ring.
//
// Same arithmetic as compose_flow_kernel (pyramid.hip) and orc_compose_flow, bit for bit: coarsest level first, a float
// accumulator updated through a double product, u = (float)((double)u + 2^s * (double)f).  2^s * f is exact in double, so the
// only roundings are the double sum and its conversion back to float, as there.
//
// Shape: the slot is one flat array of w * rows float2.  A thread takes G pixel PAIRS (2q, 2q+1), 256 pairs apart, so every
// store is a dwordx4 and one wave instruction writes 1 KB contiguous (eight whole 128-B lines).  Level `level` is read the same
// way (dwordx4, each byte once).  When the level's width is even -- every level but the coarsest, which the session requires
// even -- both pixels of a pair sit on one row at an even column, so they share ONE coarse pixel at every k > level: one dwordx2
// per coarse level per pair, and the sum over the coarse levels is formed once for both.  An odd width (the coarsest level
// composed on its own) takes the general path: rows and columns per pixel, dwordx2 loads.
#include "ofx_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPairsPerThread = 4; // G

__device__ __forceinline__ float acc(float u, double m, float f) { return (float)((double)u + m * (double)f); }

template <bool kEven>
__global__ __launch_bounds__(kThreads) void compose_ring_kernel(const ofx_compose_batch A)
{
    const int b = blockIdx.y;
    const unsigned W = (unsigned)A.w, n_px = A.n_px;
    const int L = A.levels, lvl = A.level, y0 = A.own0[lvl];
    const float *src0 = A.lv[b][lvl];
    float *dst = A.dst[b];
    const unsigned q0 = blockIdx.x * (kThreads * kPairsPerThread) + threadIdx.x;
#pragma unroll
    for (int g = 0; g < kPairsPerThread; ++g) {
        const unsigned q = q0 + (unsigned)g * kThreads, n = 2 * q;
        if (n >= n_px) break;
        const bool two = kEven || n + 1 < n_px; // (an even width makes w * rows even)
        float u0, v0, u1, v1;
        if (kEven) {
            // both pixels on row y, columns x and x + 1 with x even
            const unsigned y = n / W, x = n - y * W;
            float cu = 0.0f, cv = 0.0f;
            for (int k = L - 1; k > lvl; --k) {
                const int sc = k - lvl;
                const size_t pos = (size_t)(((int)y + y0) >> sc) - (size_t)A.own0[k];
                const float2 f = reinterpret_cast<const float2 *>(A.lv[b][k])[pos * (W >> sc) + (x >> sc)];
                const double m = (double)(1 << sc);
                cu = acc(cu, m, f.x);
                cv = acc(cv, m, f.y);
            }
            const float4 f = reinterpret_cast<const float4 *>(src0)[q];
            u0 = acc(cu, 1.0, f.x), v0 = acc(cv, 1.0, f.y);
            u1 = acc(cu, 1.0, f.z), v1 = acc(cv, 1.0, f.w);
        } else {
            float r[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned j = two ? n + i : n; // (the lone last pixel computes itself twice)
                const unsigned y = j / W, x = j - y * W;
                float u = 0.0f, v = 0.0f;
                for (int k = L - 1; k >= lvl; --k) {
                    const int sc = k - lvl;
                    const size_t pos = (size_t)(((int)y + y0) >> sc) - (size_t)A.own0[k];
                    const float2 f = reinterpret_cast<const float2 *>(A.lv[b][k])[pos * (W >> sc) + (x >> sc)];
                    const double m = (double)(1 << sc);
                    u = acc(u, m, f.x);
                    v = acc(v, m, f.y);
                }
                r[i][0] = u, r[i][1] = v;
            }
            u0 = r[0][0], v0 = r[0][1], u1 = r[1][0], v1 = r[1][1];
        }
        if (two)
            reinterpret_cast<float4 *>(dst)[q] = make_float4(u0, v0, u1, v1);
        else
            reinterpret_cast<float2 *>(dst)[n] = make_float2(u0, v0);
    }
}

} // namespace

int ofx_compose_batch_launch(const ofx_compose_batch *a, void *stream)
{
    OFX_REQUIRE(a && a->n >= 1 && a->n <= OFX_STREAM_MAX_BATCH && a->w > 0 && a->rows >= 0 && a->level >= 0 && a->level < a->levels &&
                    a->levels <= OFX_MAX_LEVELS,
                "ofx_compose_batch_launch: bad arguments");
    OFX_REQUIRE((size_t)a->w * (size_t)a->rows == (size_t)a->n_px && a->n_px < (1u << 31), "ofx_compose_batch_launch: bad pixel count");
    if (a->n_px == 0) return OFX_OK;
    const bool even = (a->w & 1) == 0;
    for (int i = 0; i < a->n; ++i) {
        OFX_REQUIRE(a->dst[i] && ((uintptr_t)a->dst[i] & 15) == 0, "ofx_compose_batch_launch: slot %d must be 16-byte aligned", i);
        for (int k = a->level; k < a->levels; ++k) OFX_REQUIRE(a->lv[i][k], "ofx_compose_batch_launch: pair %d level %d is null", i, k);
        // (the dwordx4 reads of level `level`)
        OFX_REQUIRE(!even || ((uintptr_t)a->lv[i][a->level] & 15) == 0, "ofx_compose_batch_launch: level %d of pair %d not 16-byte aligned",
                    a->level, i);
    }
    const unsigned pairs = (a->n_px + 1) / 2, per_block = kThreads * kPairsPerThread;
    dim3 grid((pairs + per_block - 1) / per_block, a->n);
    if (even)
        hipLaunchKernelGGL(compose_ring_kernel<true>, grid, dim3(kThreads), 0, ofx_stream(stream), *a);
    else
        hipLaunchKernelGGL(compose_ring_kernel<false>, grid, dim3(kThreads), 0, ofx_stream(stream), *a);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
