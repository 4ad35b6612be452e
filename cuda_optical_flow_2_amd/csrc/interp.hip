// The pixel displacement (ofx_flow_displacement, the stream pipeline's ofx_session_stream_displacement) and frame interpolation
// (ofx_interpolate_frames, ofx_interpolate_frames_batch).  The definitions are the comment blocks "pixel displacement" and "frame
// interpolation" in include/ofx.h; every float32 operation below is the definition's, in its order, and the build compiles with
// -ffp-contract=off, so nothing is fused.
//
// Displacement: elementwise, blockIdx.y = pair, floorf(uv) once per thread.  Where every flow and destination of the launch is
// 16-byte aligned a thread moves two pixels per 16-byte load and store, and an odd last pixel goes by 8 bytes; otherwise every
// pixel goes by 8 bytes (the fields are 8-byte aligned by contract).
//
// Interpolation: the march is quad_stage.h's, over two fields.  A quad's Dab and Dba arrive as four 16-byte buffer loads ONCE and
// the thread then loops over the launch's times with the fields in registers: per pair the launch reads 16 B/px of fields whatever
// the number of frames it writes, and the tap bytes come from two planes that stay cache-resident across the passes.  A pixel past
// the row's ragged end gets offsets beyond the resource and loads zeros nobody looks at, and the sampling position is clamped (or
// the pixel's own) before it becomes an offset, so no field value, however wild, reads outside a plane.
//
// The two taps of a tap row are the 2 adjacent bytes at y * pitch + x0: one 16-bit load -- EXCEPT in the last column, where the
// definition's right tap is the pixel itself (x1 == x0) and the byte behind it belongs to the row's padding, the next row, or
// nothing (the lk_body_warp.h / motion_ring.hip rule).  So a lane proves x0 < w - 1 for its four pixels on both sides and then
// takes sixteen 16-bit loads per time; any other lane takes thirty-two byte loads, the right tap AT column x1.  (A wave with such
// a lane runs both branches in turn; only waves whose positions reach the last column have one.)  All taps of a time are issued
// before the first is used.
//
// A quad of a frame leaves as one dword where the quad is whole and every destination, dst_pitch and the time stride are 4-byte
// aligned, else as bytes.  The counts: a thread keeps one packed counter per time (8 bits per class: at most 16 pixels a thread)
// in its own LDS word, touched only for a quad that has a pixel of class 1, 2 or 3; at the end each time's counters go through
// the block reduction into the time's slot, all times under one barrier.
//
// interp_kernel shares its first and its last part with interp3.hip's kernel, as text: interp_part_prologue.h (the resources and
// the geometry of one side of one pixel, with the planes' bytes per pixel as this file's constant kBpp) and interp_part_reduce.h
// (the counts); the host side of both units is interp_host.h.
#include <string.h>

#include "interp_host.h"

namespace {

using namespace quad;

constexpr int kBpp = 1;                                // interpolation: the planes' bytes per pixel (interp_part_prologue.h)
constexpr InterpNames kNames = {"d_a", "d_b", "d_dst"}; // ... and their names in the entry points' messages
constexpr int kVecs = 4;                               // displacement: 16-byte (or 8-byte) items per thread, kThreads apart

__global__ __launch_bounds__(kThreads) void displacement_kernel(const ofx_displacement_batch A, const int vec16)
{
    const int b = blockIdx.y;
    const float *flow = A.flow[b];
    float *dst = A.dst[b];
    const float scale = A.scale;
    float fu = 0.0f, fv = 0.0f; // (NULL: the first term is 0.0f, and the add is still performed)
    if (A.uv[b]) fu = __builtin_floorf(A.uv[b][0]), fv = __builtin_floorf(A.uv[b][1]);
    const uint32_t n_px = (uint32_t)A.w * (uint32_t)A.h;
    if (vec16) {
        const uint32_t n_vec = n_px >> 1;
#pragma unroll
        for (int g = 0; g < kVecs; ++g) {
            const uint32_t i = (blockIdx.x * kVecs + g) * kThreads + threadIdx.x;
            if (i >= n_vec) break;
            const f32x4 f = reinterpret_cast<const f32x4 *>(flow)[i];
            f32x4 d;
            d[0] = fu + scale * f[0], d[1] = fv + scale * f[1], d[2] = fu + scale * f[2], d[3] = fv + scale * f[3];
            reinterpret_cast<f32x4 *>(dst)[i] = d;
        }
        if ((n_px & 1u) && blockIdx.x == 0 && threadIdx.x == 0) { // the odd last pixel
            const f32x2 f = reinterpret_cast<const f32x2 *>(flow)[n_px - 1];
            f32x2 d;
            d[0] = fu + scale * f[0], d[1] = fv + scale * f[1];
            reinterpret_cast<f32x2 *>(dst)[n_px - 1] = d;
        }
    } else {
#pragma unroll
        for (int g = 0; g < kVecs; ++g) {
            const uint32_t i = (blockIdx.x * kVecs + g) * kThreads + threadIdx.x;
            if (i >= n_px) break;
            const f32x2 f = reinterpret_cast<const f32x2 *>(flow)[i];
            f32x2 d;
            d[0] = fu + scale * f[0], d[1] = fv + scale * f[1];
            reinterpret_cast<f32x2 *>(dst)[i] = d;
        }
    }
}

__global__ __launch_bounds__(kThreads) void interp_kernel(const ofx_interp_batch A, const int dwords)
{
#include "interp_part_prologue.h"

    int y, x0, y_next = 0, x0_next = 0;
    float f[16], f_next[16];
    bool have = place(qrow, n_quads, 0, y, x0), have_next = false;
    load_fields(have, y, x0, f);
#pragma nounroll
    for (int g = 0; g < kQuads; ++g) {
        if (!have) break;
        // the next quad's fields go out before this quad's taps: their latency runs under them
        have_next = g + 1 < kQuads && place(qrow, n_quads, g + 1, y_next, x0_next);
        load_fields(have_next, y_next, x0_next, f_next);
        const int npx = w - x0 < 4 ? w - x0 : 4;
        const float yf = (float)y;
        uint8_t *row = dst + (size_t)y * (size_t)A.dst_pitch + (size_t)x0;
#pragma nounroll
        for (int ti = 0; ti < nt; ++ti) {
            const float t = A.t[ti], c00 = A.c00[ti], c01 = A.c01[ti], c10 = A.c10[ti];
            // steps 1 to 5, up to the taps.  Index [0]: side a, [1]: side b
            float fx[2][4], fy[2][4];
            uint32_t o0[2][4], o1[2][4], dx[2][4], cls[4];
            bool wide = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float abx = f[2 * k], aby = f[2 * k + 1], bax = f[8 + 2 * k], bay = f[8 + 2 * k + 1];
                const float tax = c00 * abx + c01 * bax, tay = c00 * aby + c01 * bay;
                const float tbx = c10 * abx + c00 * bax, tby = c10 * aby + c00 * bay;
                const float xf = (float)(x0 + k);
                const bool live = k < npx;
                const bool ua = side(xf + tax, yf + tay, xf, yf, ap, live, o0[0][k], o1[0][k], dx[0][k], fx[0][k], fy[0][k]);
                const bool ub = side(xf + tbx, yf + tby, xf, yf, bp, live, o0[1][k], o1[1][k], dx[1][k], fx[1][k], fy[1][k]);
                cls[k] = ua ? (ub ? 0u : 1u) : (ub ? 2u : 3u);
                wide = wide && (!live || (dx[0][k] & dx[1][k]));
            }
            // the taps: per side and pixel (left, right) of the two tap rows in bytes 0 and 1
            uint32_t r0[2][4], r1[2][4];
            if (wide) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    r0[0][k] = __builtin_amdgcn_raw_buffer_load_b16(rs_a, o0[0][k], 0, 0);
                    r1[0][k] = __builtin_amdgcn_raw_buffer_load_b16(rs_a, o1[0][k], 0, 0);
                    r0[1][k] = __builtin_amdgcn_raw_buffer_load_b16(rs_b, o0[1][k], 0, 0);
                    r1[1][k] = __builtin_amdgcn_raw_buffer_load_b16(rs_b, o1[1][k], 0, 0);
                }
            } else {
                uint32_t l[2][2][4], r[2][2][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    l[0][0][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_a, o0[0][k], 0, 0);
                    r[0][0][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_a, o0[0][k] + dx[0][k], 0, 0);
                    l[0][1][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_a, o1[0][k], 0, 0);
                    r[0][1][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_a, o1[0][k] + dx[0][k], 0, 0);
                    l[1][0][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_b, o0[1][k], 0, 0);
                    r[1][0][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_b, o0[1][k] + dx[1][k], 0, 0);
                    l[1][1][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_b, o1[1][k], 0, 0);
                    r[1][1][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_b, o1[1][k] + dx[1][k], 0, 0);
                }
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int k = 0; k < 4; ++k) r0[s][k] = l[s][0][k] | (r[s][0][k] << 8), r1[s][k] = l[s][1][k] | (r[s][1][k] << 8);
            }
            // the taps have arrived: the blends of step 5, then step 6
            uint32_t out = 0, pk = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float V[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) V[s] = blend_u8(r0[s][k], r1[s][k], fx[s][k], fy[s][k]);
                const float mix = V[0] + t * (V[1] - V[0]);
                const float v = cls[k] == 1u ? V[0] : cls[k] == 2u ? V[1] : mix;
                out |= round_u8(v) << (8 * k);
                if (k < npx && cls[k]) pk += 1u << (8 * (cls[k] - 1u));
            }
            uint8_t *d = row + (size_t)ti * A.time_stride; // (store_quad_u8, written out: behind the function the time loop is scheduled otherwise)
            if (npx == 4 && dwords) {
                *reinterpret_cast<uint32_t *>(d) = out;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < npx) d[k] = (uint8_t)(out >> (8 * k));
            }
            if (stats && pk) cnt[ti][threadIdx.x] += pk;
        }
        have = have_next, y = y_next, x0 = x0_next;
#pragma unroll
        for (int k = 0; k < 16; ++k) f[k] = f_next[k];
    }
#include "interp_part_reduce.h"
}

} // namespace

int ofx_displacement_batch_launch(const ofx_displacement_batch *a, void *stream)
{
    const char *who = "ofx_displacement_batch_launch";
    OFX_REQUIRE(a && a->n >= 1 && a->n <= OFX_STREAM_MAX_BATCH, "%s: bad arguments", who);
    OFX_REQUIRE(a->w > 0 && a->h > 0, "%s: w = %d, h = %d must be positive", who, a->w, a->h);
    OFX_REQUIRE((size_t)a->w * (size_t)a->h < ((size_t)1 << 28), "%s: w * h = %d x %d is more than this build takes (2^28 pixels)", who, a->w, a->h);
    OFX_REQUIRE(__builtin_isfinite(a->scale), "%s: the scale must be finite", who);
    bool vec16 = true;
    for (int i = 0; i < a->n; ++i) {
        OFX_REQUIRE(a->flow[i], "%s: pair %d: d_flow is null", who, i);
        OFX_REQUIRE(a->dst[i], "%s: pair %d: d_dst is null", who, i);
        OFX_REQUIRE((((uintptr_t)a->flow[i] | (uintptr_t)a->dst[i]) & 7) == 0, "%s: pair %d: d_flow and d_dst must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)a->uv[i] & 3) == 0, "%s: pair %d: d_uv must be 4-byte aligned", who, i);
        vec16 = vec16 && (((uintptr_t)a->flow[i] | (uintptr_t)a->dst[i]) & 15) == 0;
    }
    const unsigned n_px = (unsigned)a->w * (unsigned)a->h, items = vec16 ? (n_px >> 1) : n_px, per_block = kThreads * kVecs;
    dim3 grid(items ? (items + per_block - 1) / per_block : 1, a->n); // (a single pixel on the 16-byte path: the odd-pixel thread alone)
    hipLaunchKernelGGL(displacement_kernel, grid, dim3(kThreads), 0, ofx_stream(stream), *a, (int)vec16);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_flow_displacement(const float *d_flow, int w, int h, const float *d_uv, float scale, float *d_dst, void *stream)
{
    static thread_local ofx_displacement_batch db;
    memset(&db, 0, sizeof db);
    db.n = 1, db.w = w, db.h = h, db.scale = scale;
    db.flow[0] = d_flow, db.uv[0] = d_uv, db.dst[0] = d_dst;
    return ofx_displacement_batch_launch(&db, stream); // (checks every argument before it enqueues anything)
}

int ofx_interp_batch_launch(const ofx_interp_batch *a, void *stream)
{
    return interp_launch("ofx_interp_batch_launch", interp_kernel, kBpp, kNames, a, stream);
}

extern "C" int ofx_interpolate_frames_batch(const uint8_t *const *d_a, const int *a_pitches, const uint8_t *const *d_b, const int *b_pitches, int n,
                                            int w, int h, const float *const *d_disp_ab, const float *const *d_disp_ba, const float *h_times,
                                            int n_times, uint8_t *const *d_dst, int dst_pitch, size_t time_stride_bytes, int64_t *const *d_stats,
                                            void *stream)
{
    static thread_local ofx_interp_batch ib;
    OFX_TRY(interp_fill_batch("ofx_interpolate_frames_batch", kNames, &ib, d_a, a_pitches, d_b, b_pitches, n, w, h, d_disp_ab, d_disp_ba, h_times,
                              n_times, d_dst, dst_pitch, time_stride_bytes, d_stats));
    return ofx_interp_batch_launch(&ib, stream); // (checks every argument before it enqueues anything)
}

extern "C" int ofx_interpolate_frames(const uint8_t *d_a, int a_pitch, const uint8_t *d_b, int b_pitch, int w, int h, const float *d_disp_ab,
                                      const float *d_disp_ba, const float *h_times, int n_times, uint8_t *d_dst, int dst_pitch,
                                      size_t time_stride_bytes, int64_t *d_stats, void *stream)
{
    const char *who = "ofx_interpolate_frames";
    OFX_REQUIRE(d_a && d_b, "%s: a null plane (d_a, d_b)", who);
    OFX_REQUIRE(d_disp_ab && d_disp_ba, "%s: a null field (d_disp_ab, d_disp_ba)", who);
    OFX_REQUIRE(d_dst, "%s: d_dst is null", who);
    return ofx_interpolate_frames_batch(&d_a, &a_pitch, &d_b, &b_pitch, 1, w, h, &d_disp_ab, &d_disp_ba, h_times, n_times, &d_dst, dst_pitch,
                                        time_stride_bytes, d_stats ? &d_stats : nullptr, stream);
}
