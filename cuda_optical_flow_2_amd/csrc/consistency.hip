// The forward-backward consistency check (ofx_flow_consistency, ofx_flow_consistency_batch): for every pixel of n pairs, in ONE
// launch, the class the definition "forward-backward consistency" in include/ofx.h gives it -- consistent, inconsistent, leaves
// the frame, undefined -- the squared round-trip error e, and the pair's three counts.  Every float32 operation below is the
// definition's, in its order; the build compiles with -ffp-contract=off, so nothing is fused.
//
// The march is quad_stage.h's, over fwd; the taps come from bwd.  A pixel of class 2 or 3 -- and a pixel past the row's ragged
// end -- gets tap offsets beyond the resource: the unit returns zeros nobody looks at.
//
// The two taps of a tap row are the 16 adjacent bytes at 8 * (y * w + x0), 8-byte aligned only: one 16-byte load -- EXCEPT in
// the last column.  At x0 == w - 1 the definition's right tap is the pixel itself (x1 == x0); the 8 bytes behind it belong to
// the next row, or to nothing, and must not reach the blend: fx is 0 there, but 0 * (NaN - b00) is NaN.  So a lane proves
// x0 < w - 1 for its four pixels and then takes eight 16-byte loads; any other lane takes sixteen 8-byte loads, the right tap
// AT column x1.  (A wave with such a lane runs both branches in turn; only waves whose vectors reach the last column have
// one.)  The last row needs no such care: row y1 = min(y0 + 1, h - 1) is part of the address, so b10 is b00 there by itself.
//
// The classes of a quad leave as one dword where the mask and its pitch are 4-byte aligned and the quad is whole, else as
// bytes; e as four floats where err is 16-byte aligned and w a multiple of 4, else one by one.  The counts: per-thread
// counters, then the block reduction described in quad_stage.h into the pair's slot.
#include <string.h>

#include "quad_stage.h"

namespace {

using namespace quad;

constexpr uint32_t kInfBits = 0x7f800000u;

__global__ __launch_bounds__(kThreads) void consistency_kernel(const ofx_consistency_batch A, const int mask_dwords, const int err_quads)
{
    __shared__ uint32_t red[kThreads / 64][3];
    const int b = blockIdx.y;
    const int w = A.w, h = A.h, wmax = w - 1, hmax = h - 1;
    const int bytes = w * h * 8;
    const __amdgpu_buffer_rsrc_t rs_fwd = rsrc(A.fwd[b], bytes), rs_bwd = rsrc(A.bwd[b], bytes);
    uint8_t *mask = A.mask[b];
    float *err = A.err[b];
    unsigned long long *stats = A.stats[b];
    const float wmaxf = (float)wmax, hmaxf = (float)hmax, scale = A.scale, alpha = A.alpha, beta = A.beta;
    const uint32_t qrow = quads_per_row(w), n_quads = qrow * (uint32_t)h;

    uint32_t n1 = 0, n2 = 0, n3 = 0;
    int y, x0, y_next, x0_next;
    float f[8], f_next[8];
    bool have = place(qrow, n_quads, 0, y, x0), have_next = false;
    load_field(rs_fwd, w, have, y, x0, f);
#pragma unroll
    for (int g = 0; g < kQuads; ++g) {
        if (!have) break;
        // the next quad's fwd goes out before this quad's taps: its latency runs under them
        have_next = g + 1 < kQuads && place(qrow, n_quads, g + 1, y_next, x0_next);
        load_field(rs_fwd, w, have_next, y_next, x0_next, f_next);
        const int npx = w - x0 < 4 ? w - x0 : 4;
        const float yf = (float)y;
        // steps 1 to 4
        float fx[4], fy[4];
        uint32_t cls[4], off0[4], off1[4], offr0[4], offr1[4];
        bool wide = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float px = (float)(x0 + k) + scale * f[2 * k], py = yf + scale * f[2 * k + 1];
            const bool ok = __builtin_fabsf(px) <= 1e9f && __builtin_fabsf(py) <= 1e9f; // (a NaN fails)
            const bool gone = px < 0.0f || px > wmaxf || py < 0.0f || py > hmaxf;
            cls[k] = !ok ? OFX_FB_UNDEFINED : gone ? OFX_FB_LEAVES : OFX_FB_CONSISTENT;
            const bool live = ok && !gone && k < npx;
            const float sx = live ? px : 0.0f, sy = live ? py : 0.0f;
            const int xi = (int)sx, yi = (int)sy;
            fx[k] = sx - (float)xi, fy[k] = sy - (float)yi;
            const int x1 = min(xi + 1, wmax), y1 = min(yi + 1, hmax);
            off0[k] = live ? 8u * (uint32_t)(yi * w + xi) : kNowhere, off1[k] = live ? 8u * (uint32_t)(y1 * w + xi) : kNowhere;
            offr0[k] = live ? 8u * (uint32_t)(yi * w + x1) : kNowhere, offr1[k] = live ? 8u * (uint32_t)(y1 * w + x1) : kNowhere;
            wide = wide && (!live || xi < wmax);
        }
        // the taps: per pixel (b00.u, b00.v, b01.u, b01.v) and (b10.u, b10.v, b11.u, b11.v)
        f32x4 ta[4], tb[4];
        if (wide) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ta[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_bwd, off0[k], 0, 0));
                tb[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_bwd, off1[k], 0, 0));
            }
        } else {
            f32x2 l0[4], r0[4], l1[4], r1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                l0[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_bwd, off0[k], 0, 0));
                r0[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_bwd, offr0[k], 0, 0));
                l1[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_bwd, off1[k], 0, 0));
                r1[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_bwd, offr1[k], 0, 0));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ta[k][0] = l0[k][0], ta[k][1] = l0[k][1], ta[k][2] = r0[k][0], ta[k][3] = r0[k][1];
                tb[k][0] = l1[k][0], tb[k][1] = l1[k][1], tb[k][2] = r1[k][0], tb[k][3] = r1[k][1];
            }
        }
        // the taps have arrived: steps 5 (the blend, per component) to 7
        uint32_t out = 0;
        float e4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float u = f[2 * k], v = f[2 * k + 1];
            const float ru = blend(ta[k][0], ta[k][2], tb[k][0], tb[k][2], fx[k], fy[k]);
            const float rv = blend(ta[k][1], ta[k][3], tb[k][1], tb[k][3], fx[k], fy[k]);
            const float du = u + ru, dv = v + rv;
            const float e = du * du + dv * dv;
            const float m = (u * u + v * v) + (ru * ru + rv * rv);
            const float thr = alpha * m + beta;
            uint32_t c = cls[k];
            if (c == OFX_FB_CONSISTENT) c = !(__builtin_fabsf(e) <= 3.402823466e+38f) ? OFX_FB_UNDEFINED : e <= thr ? OFX_FB_CONSISTENT : OFX_FB_INCONSISTENT;
            e4[k] = c <= OFX_FB_INCONSISTENT ? e : __builtin_bit_cast(float, kInfBits);
            out |= c << (8 * k);
            if (k < npx) n1 += c == OFX_FB_INCONSISTENT, n2 += c == OFX_FB_LEAVES, n3 += c == OFX_FB_UNDEFINED;
        }
        if (mask) store_quad_u8(mask + (size_t)y * (size_t)A.mask_pitch + (size_t)x0, out, npx, mask_dwords);
        if (err) {
            float *d = err + (size_t)y * (size_t)w + (size_t)x0;
            if (err_quads) { // (w is a multiple of 4: every quad is whole)
                f32x4 q;
                q[0] = e4[0], q[1] = e4[1], q[2] = e4[2], q[3] = e4[3];
                *reinterpret_cast<f32x4 *>(d) = q;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < npx) d[k] = e4[k];
            }
        }
        have = have_next, y = y_next, x0 = x0_next;
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = f_next[k];
    }
    if (!stats) return; // (block-uniform)
    // the block reduction (the rule: quad_stage.h), written out: behind a function the kernel's other instructions come out in another order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n1 += __shfl_xor(n1, o);
        n2 += __shfl_xor(n2, o);
        n3 += __shfl_xor(n3, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = n1, red[threadIdx.x >> 6][1] = n2, red[threadIdx.x >> 6][2] = n3;
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < kThreads / 64; ++i) s += red[i][threadIdx.x];
        if (s) atomicAdd(stats + 1 + threadIdx.x, s);
    } else if (threadIdx.x == 3 && blockIdx.x == 0) {
        atomicAdd(stats, (unsigned long long)w * (unsigned long long)h);
    }
}

} // namespace

int ofx_consistency_batch_launch(const ofx_consistency_batch *a, void *stream)
{
    const char *who = "ofx_consistency_batch_launch";
    OFX_REQUIRE(a, "%s: bad arguments", who);
    OFX_TRY(check_batch(who, a->n, a->w, a->h, 1, {}, {a->fwd, a->bwd}, a->stats));
    OFX_REQUIRE(__builtin_isfinite(a->scale), "%s: the scale must be finite", who);
    OFX_REQUIRE(__builtin_isfinite(a->alpha) && a->alpha >= 0.0f && __builtin_isfinite(a->beta) && a->beta >= 0.0f,
                "%s: alpha and beta must be finite and >= 0", who);
    bool mask_dwords = (a->mask_pitch & 3) == 0, err_quads = (a->w & 3) == 0;
    for (int i = 0; i < a->n; ++i) {
        OFX_REQUIRE(a->mask[i] || a->err[i] || a->stats[i], "%s: pair %d has no output", who, i);
        OFX_REQUIRE(((uintptr_t)a->err[i] & 3) == 0, "%s: pair %d: err must be 4-byte aligned", who, i);
        OFX_REQUIRE(!a->mask[i] || a->mask_pitch >= a->w, "%s: the mask's row pitch %d is below the width %d", who, a->mask_pitch, a->w);
        mask_dwords = mask_dwords && ((uintptr_t)a->mask[i] & 3) == 0;
        err_quads = err_quads && ((uintptr_t)a->err[i] & 15) == 0;
    }
    OFX_TRY(zero_stats(a->stats, a->n, 4, stream)); // (everything is checked)
    hipLaunchKernelGGL(consistency_kernel, grid(a->w, a->h, a->n), dim3(kThreads), 0, ofx_stream(stream), *a, (int)mask_dwords, (int)err_quads);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_flow_consistency_batch(const float *const *d_fwd, const float *const *d_bwd, int n, int w, int h, float scale, float alpha,
                                          float beta, uint8_t *const *d_mask, int mask_pitch, float *const *d_err, int64_t *const *d_stats,
                                          void *stream)
{
    const char *who = "ofx_flow_consistency_batch";
    OFX_REQUIRE(d_fwd && d_bwd, "%s: null field array", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    OFX_REQUIRE(d_mask || d_err || d_stats, "%s: no output asked for", who);
    static thread_local ofx_consistency_batch cb;
    memset(&cb, 0, sizeof cb);
    cb.n = n, cb.w = w, cb.h = h, cb.scale = scale, cb.alpha = alpha, cb.beta = beta, cb.mask_pitch = d_mask ? mask_pitch : 0;
    for (int i = 0; i < n; ++i) {
        OFX_REQUIRE((!d_mask || d_mask[i]) && (!d_err || d_err[i]) && (!d_stats || d_stats[i]), "%s: pair %d: a null entry in an output array", who, i);
        cb.fwd[i] = d_fwd[i], cb.bwd[i] = d_bwd[i];
        cb.mask[i] = d_mask ? d_mask[i] : nullptr;
        cb.err[i] = d_err ? d_err[i] : nullptr;
        cb.stats[i] = d_stats ? reinterpret_cast<unsigned long long *>(d_stats[i]) : nullptr;
    }
    return ofx_consistency_batch_launch(&cb, stream); // (checks every argument before it enqueues anything)
}

extern "C" int ofx_flow_consistency(const float *d_fwd, const float *d_bwd, int w, int h, float scale, float alpha, float beta, uint8_t *d_mask,
                                    int mask_pitch, float *d_err, int64_t *d_stats, void *stream)
{
    OFX_REQUIRE(d_mask || d_err || d_stats, "ofx_flow_consistency: no output asked for");
    return ofx_flow_consistency_batch(&d_fwd, &d_bwd, 1, w, h, scale, alpha, beta, d_mask ? &d_mask : nullptr, mask_pitch, d_err ? &d_err : nullptr,
                                      d_stats ? &d_stats : nullptr, stream);
}
