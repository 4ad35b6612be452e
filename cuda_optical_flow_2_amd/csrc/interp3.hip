// Colour frame interpolation (ofx_interpolate_frames_3ch, ofx_interpolate_frames_3ch_batch).  The definition is the comment block
// "colour frame interpolation" in include/ofx.h, which quotes "frame interpolation": every float32 operation below is that
// definition's, in its order, and the build compiles with -ffp-contract=off, so nothing is fused.
//
// The march is quad_stage.h's over two fields, as interp.hip's: blockIdx.y = pair, a thread owns four adjacent pixels, a quad's Dab
// and Dba arrive ONCE as four 16-byte buffer loads, the next quad's fields go out before this quad's taps, and the thread loops over
// the launch's times with the fields in registers.  What is new is that the geometry -- steps 1 to 4, the fractions and the class
// -- is worked out once per pixel and serves three channels: per pair the launch reads 16 B/px of fields and writes 3 B/px per
// time, where three grey launches read 48.
//
// A side's tap row is the 6 adjacent bytes at y * pitch + 3 * x0: the left pixel's three channels, then the right pixel's.
//   wide    a lane that has proved x0 < w - 1 for the live pixels of its unit on both sides fetches a tap row as one dword at the
//           tap's own byte (unaligned, through the buffer resource, as lk_body_warp.h does) plus one 16-bit load 4 bytes behind it.
//           3 * x0 + 5 <= 3 * w - 1: both lie wholly inside the row.
//   narrow  any other lane: the right tap is the pixel at column x1 = x0 + dx ITSELF (in the last column that is the left pixel
//           again), each pixel as a 16-bit and an 8-bit load, assembled into the wide form's two words.  No load begins in a plane's
//           last bytes and ends beyond them (the lk_body_warp.h / motion_ring.hip / interp.hip rule, three bytes wide).
// (A wave with a narrow lane runs both branches in turn; only waves whose positions reach the last column have one.)  Every plane
// and field goes through a resource of exactly its bytes, the sampling position is clamped (or the pixel's own) before it becomes an
// offset, and a pixel past the row's ragged end gets kNowhere (+ a few bytes: still beyond every plane) and loads zeros nobody
// looks at.
//
// Budget (gfx950: 512 registers per lane and SIMD, 4 waves up to 128, 3 waves from 136).  interp.hip sits at 122 with 16 tap
// registers per time.  Here a tap row is 2 registers, so a whole quad's taps would be 4 px x 2 sides x 2 rows x 2 = 32 registers
// on top of the 32 of the two quads' fields, 16 fractions and 12 blended values: beyond 128.  So the UNIT whose taps are in flight
// together is TWO PIXELS: 2 px x 2 sides x 2 rows x 2 = 16 tap registers (16 loads in flight, as in the grey kernel), 8 fractions,
// 8 offsets that die as the loads go out; a unit's six bytes are packed into the quad's three output dwords as they are made.
// Expected: fields 32 + taps 16 + fractions 8 + offsets 8 + out 3 + addresses and counters ~ 25 = ~ 92: 4 waves per SIMD with
// room, and no scratch.  LDS: 8 x 256 counters + 4 x 8 x 3 wave sums = 8576 bytes per block, no limit at 4 blocks per CU.  The
// compiler reports 128 VGPRs -- it allocates up to the 4-wave limit, not beyond it -- 4 waves per SIMD, no scratch (DESIGN.md
// section 4.14); the two units stay apart in the listing, each unit's sixteen wide loads together ahead of its blends.  The narrow
// form goes one SIDE at a time (sixteen loads in flight): with both sides together it set the kernel's peak, 142 registers and
// 3 waves, and forcing that version to 128 spilled 12 bytes per lane to scratch.
//
// A whole quad of a frame (12 bytes at row + 12 * (x0 / 4)) leaves as three dwords where every destination, dst_pitch and the time
// stride are 4-byte aligned, else as bytes.  The counts are interp.hip's: a packed per-time LDS word per thread (8 bits per class:
// at most 16 pixels a thread), one barrier, 64-bit atomics into slots the launch has zeroed on the stream.
#include <string.h>

#include "quad_stage.h"

namespace {

using namespace quad;

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));

// channel c of the left / of the right pixel of a tap row held as (dword at the tap's byte, the two bytes behind it)
__device__ __forceinline__ float tap_left(uint32_t d, int c) { return (float)((d >> (8 * c)) & 0xffu); }
__device__ __forceinline__ float tap_right(uint32_t d, uint32_t e, int c) { return c == 0 ? (float)(d >> 24) : (float)((e >> (8 * (c - 1))) & 0xffu); }

__global__ __launch_bounds__(kThreads) void interp3_kernel(const ofx_interp3_batch A, const int dwords)
{
    __shared__ uint32_t cnt[OFX_INTERP_MAX_TIMES][kThreads];
    __shared__ uint32_t red[kThreads / 64][OFX_INTERP_MAX_TIMES][3];
    const int b = blockIdx.y;
    const int w = A.w, h = A.h, wmax = w - 1, hmax = h - 1, nt = A.n_times;
    const int ap = A.a_pitch[b], bp = A.b_pitch[b];
    const __amdgpu_buffer_rsrc_t rs_a = rsrc(A.a[b], hmax * ap + 3 * w), rs_b = rsrc(A.b[b], hmax * bp + 3 * w);
    const __amdgpu_buffer_rsrc_t rs_ab = rsrc(A.dab[b], w * h * 8), rs_ba = rsrc(A.dba[b], w * h * 8);
    uint8_t *dst = A.dst[b];
    unsigned long long *stats = A.stats[b];
    const float wmaxf = (float)wmax, hmaxf = (float)hmax;
    const uint32_t qrow = quads_per_row(w), n_quads = qrow * (uint32_t)h;
    if (stats)
        for (int ti = 0; ti < nt; ++ti) cnt[ti][threadIdx.x] = 0; // (a thread's own words: no barrier needed)

    // a quad's two fields, Dab in f[0 .. 7] and Dba in f[8 .. 15]
    auto load_fields = [&](bool in, int y, int x0, float *f) {
        load_field(rs_ab, w, in, y, x0, f);
        load_field(rs_ba, w, in, y, x0, f + 8);
    };
    // steps 3 to 5 of one side of one pixel, up to the taps: the byte offsets of the left taps of its two tap rows, whether the
    // right taps are the next pixel (x0 < w - 1) or the same one, and the fractions.  Returns "usable".
    auto side = [&](float px, float py, float xf, float yf, int pitch, bool live, uint32_t &o0, uint32_t &o1, uint32_t &dx, float &fx,
                    float &fy) -> bool {
        const bool fin = __builtin_fabsf(px) <= 1e9f && __builtin_fabsf(py) <= 1e9f; // (a NaN fails)
        const bool usable = fin && px >= 0.0f && px <= wmaxf && py >= 0.0f && py <= hmaxf;
        const float sx = fin ? __builtin_amdgcn_fmed3f(px, 0.0f, wmaxf) : xf;
        const float sy = fin ? __builtin_amdgcn_fmed3f(py, 0.0f, hmaxf) : yf;
        const int xi = (int)sx, yi = (int)sy;
        fx = sx - (float)xi, fy = sy - (float)yi;
        const int y1 = min(yi + 1, hmax);
        o0 = live ? (uint32_t)(yi * pitch + 3 * xi) : kNowhere, o1 = live ? (uint32_t)(y1 * pitch + 3 * xi) : kNowhere;
        dx = xi < wmax ? 1u : 0u;
        return usable;
    };
    // one tap row: (the dword at o, the two bytes behind it) -- six bytes that lie inside the row when the right tap is the next pixel
    auto row_wide = [&](const __amdgpu_buffer_rsrc_t &rs, uint32_t o, uint32_t &d, uint32_t &e) {
        d = __builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0);
        e = __builtin_amdgcn_raw_buffer_load_b16(rs, o + 4u, 0, 0);
    };

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
        uint8_t *row = dst + (size_t)y * (size_t)A.dst_pitch + (size_t)(3 * x0);
#pragma nounroll
        for (int ti = 0; ti < nt; ++ti) {
            const float t = A.t[ti], c00 = A.c00[ti], c01 = A.c01[ti], c10 = A.c10[ti];
            uint32_t out[3] = {0u, 0u, 0u}, pk = 0; // byte 3 * k + c of the quad: channel c of pixel k
#pragma unroll
            for (int u = 0; u < 2; ++u) { // the unit: pixels 2u and 2u + 1
                // steps 1 to 5, up to the taps, once per pixel.  Index [0]: side a, [1]: side b
                float fx[2][2], fy[2][2];
                uint32_t o0[2][2], o1[2][2], dx[2][2], cls[2];
                bool wide = true;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int k = 2 * u + j;
                    const float abx = f[2 * k], aby = f[2 * k + 1], bax = f[8 + 2 * k], bay = f[8 + 2 * k + 1];
                    const float tax = c00 * abx + c01 * bax, tay = c00 * aby + c01 * bay;
                    const float tbx = c10 * abx + c00 * bax, tby = c10 * aby + c00 * bay;
                    const float xf = (float)(x0 + k);
                    const bool live = k < npx;
                    const bool ua = side(xf + tax, yf + tay, xf, yf, ap, live, o0[0][j], o1[0][j], dx[0][j], fx[0][j], fy[0][j]);
                    const bool ub = side(xf + tbx, yf + tby, xf, yf, bp, live, o0[1][j], o1[1][j], dx[1][j], fx[1][j], fy[1][j]);
                    cls[j] = ua ? (ub ? 0u : 1u) : (ub ? 2u : 3u);
                    wide = wide && (!live || (dx[0][j] & dx[1][j]));
                }
                // the taps of the unit, all issued before the first is used: per side and pixel the upper tap row in (d0, e0), the
                // lower in (d1, e1)
                uint32_t d0[2][2], e0[2][2], d1[2][2], e1[2][2];
                if (wide) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        row_wide(rs_a, o0[0][j], d0[0][j], e0[0][j]);
                        row_wide(rs_a, o1[0][j], d1[0][j], e1[0][j]);
                        row_wide(rs_b, o0[1][j], d0[1][j], e0[1][j]);
                        row_wide(rs_b, o1[1][j], d1[1][j], e1[1][j]);
                    }
                } else {
                    // one side at a time (its sixteen loads in flight together).  [tap row][pixel]: bytes 0 and 1 and byte 2 of the left
                    // pixel, of the pixel at column x1 likewise
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const __amdgpu_buffer_rsrc_t &rs = s ? rs_b : rs_a;
                        uint32_t l2[2][2], l1[2][2], r2[2][2], r1[2][2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const uint32_t step = 3u * dx[s][j];
                            l2[0][j] = __builtin_amdgcn_raw_buffer_load_b16(rs, o0[s][j], 0, 0);
                            l1[0][j] = __builtin_amdgcn_raw_buffer_load_b8(rs, o0[s][j] + 2u, 0, 0);
                            r2[0][j] = __builtin_amdgcn_raw_buffer_load_b16(rs, o0[s][j] + step, 0, 0);
                            r1[0][j] = __builtin_amdgcn_raw_buffer_load_b8(rs, o0[s][j] + step + 2u, 0, 0);
                            l2[1][j] = __builtin_amdgcn_raw_buffer_load_b16(rs, o1[s][j], 0, 0);
                            l1[1][j] = __builtin_amdgcn_raw_buffer_load_b8(rs, o1[s][j] + 2u, 0, 0);
                            r2[1][j] = __builtin_amdgcn_raw_buffer_load_b16(rs, o1[s][j] + step, 0, 0);
                            r1[1][j] = __builtin_amdgcn_raw_buffer_load_b8(rs, o1[s][j] + step + 2u, 0, 0);
                        }
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            d0[s][j] = l2[0][j] | (l1[0][j] << 16) | (r2[0][j] << 24), e0[s][j] = (r2[0][j] >> 8) | (r1[0][j] << 8);
                            d1[s][j] = l2[1][j] | (l1[1][j] << 16) | (r2[1][j] << 24), e1[s][j] = (r2[1][j] >> 8) | (r1[1][j] << 8);
                        }
                    }
                }
                // the taps have arrived: per channel the blends of step 5, then step 6, with the pixel's fractions and class
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int k = 2 * u + j;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float V[2];
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            V[s] = blend(tap_left(d0[s][j], c), tap_right(d0[s][j], e0[s][j], c), tap_left(d1[s][j], c),
                                         tap_right(d1[s][j], e1[s][j], c), fx[s][j], fy[s][j]);
                        const float mix = V[0] + t * (V[1] - V[0]);
                        const float v = cls[j] == 1u ? V[0] : cls[j] == 2u ? V[1] : mix;
                        const int byte = 3 * k + c;
                        out[byte >> 2] |= round_u8(v) << (8 * (byte & 3));
                    }
                    if (k < npx && cls[j]) pk += 1u << (8 * (cls[j] - 1u));
                }
            }
            uint8_t *d = row + (size_t)ti * A.time_stride;
            if (npx == 4 && dwords) {
                u32x3 v;
                v[0] = out[0], v[1] = out[1], v[2] = out[2];
                *reinterpret_cast<u32x3_a4 *>(d) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    if (i < 3 * npx) d[i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
            }
            if (stats && pk) cnt[ti][threadIdx.x] += pk;
        }
        have = have_next, y = y_next, x0 = x0_next;
#pragma unroll
        for (int k = 0; k < 16; ++k) f[k] = f_next[k];
    }
    if (!stats) return; // (block-uniform)
    // the block reduction (the rule: quad_stage.h), per time and written out as in interp_kernel
    for (int ti = 0; ti < nt; ++ti) {
        const uint32_t pk = cnt[ti][threadIdx.x];
        uint32_t n1 = pk & 0xffu, n2 = (pk >> 8) & 0xffu, n3 = (pk >> 16) & 0xffu;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n1 += __shfl_xor(n1, o);
            n2 += __shfl_xor(n2, o);
            n3 += __shfl_xor(n3, o);
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][ti][0] = n1, red[threadIdx.x >> 6][ti][1] = n2, red[threadIdx.x >> 6][ti][2] = n3;
    }
    __syncthreads();
    const int ti = threadIdx.x >> 2, c = threadIdx.x & 3; // thread 4 * ti + c: word c of time ti
    if (ti < nt) {
        if (c) {
            unsigned long long s = 0;
#pragma unroll
            for (int i = 0; i < kThreads / 64; ++i) s += red[i][ti][c - 1];
            if (s) atomicAdd(stats + 4 * ti + c, s);
        } else if (blockIdx.x == 0) {
            atomicAdd(stats + 4 * ti, (unsigned long long)w * (unsigned long long)h);
        }
    }
}

} // namespace

int ofx_interp3_batch_launch(const ofx_interp3_batch *a, void *stream)
{
    const char *who = "ofx_interp3_batch_launch";
    OFX_REQUIRE(a, "%s: bad arguments", who);
    // check_batch's rules with every pitch against 3 * w (w > 0 is asked first: 3 * w cannot overflow below 2^28 pixels)
    OFX_REQUIRE(a->n >= 1 && a->n <= OFX_STREAM_MAX_BATCH, "%s: bad arguments: n = %d pairs is not in 1 .. %d", who, a->n, OFX_STREAM_MAX_BATCH);
    OFX_REQUIRE(a->w > 0 && a->h > 0, "%s: w = %d, h = %d must be positive", who, a->w, a->h);
    OFX_REQUIRE((size_t)a->w * (size_t)a->h < ((size_t)1 << 28), "%s: w * h = %d x %d is more than this build takes (2^28 pixels)", who, a->w, a->h);
    const int w3 = 3 * a->w;
    OFX_REQUIRE(a->n_times >= 1 && a->n_times <= OFX_INTERP_MAX_TIMES, "%s: n_times = %d is not in 1 .. %d", who, a->n_times, OFX_INTERP_MAX_TIMES);
    for (int k = 0; k < a->n_times; ++k)
        OFX_REQUIRE(__builtin_isfinite(a->t[k]) && a->t[k] > 0.0f && a->t[k] < 1.0f, "%s: h_times[%d] = %g is not in (0, 1)", who, k, (double)a->t[k]);
    OFX_REQUIRE(a->dst_pitch >= w3, "%s: dst_pitch %d is below a row's 3 * w = %d bytes", who, a->dst_pitch, w3);
    OFX_REQUIRE(a->n_times == 1 || a->time_stride >= (size_t)a->h * (size_t)a->dst_pitch,
                "%s: time_stride_bytes %zu is below a frame's h * dst_pitch = %zu bytes", who, a->time_stride, (size_t)a->h * (size_t)a->dst_pitch);
    bool dwords = (a->dst_pitch & 3) == 0 && (a->n_times == 1 || (a->time_stride & 3) == 0);
    for (int i = 0; i < a->n; ++i) {
        OFX_REQUIRE(a->a[i] && a->b[i], "%s: pair %d: a null plane (d_a3, d_b3)", who, i);
        OFX_REQUIRE(a->dab[i] && a->dba[i], "%s: pair %d: a null field (d_disp_ab, d_disp_ba)", who, i);
        OFX_REQUIRE(a->dst[i], "%s: pair %d: d_dst3 is null", who, i);
        OFX_REQUIRE(a->a_pitch[i] >= w3 && a->b_pitch[i] >= w3, "%s: pair %d: a row pitch (%d, %d) below a row's 3 * w = %d bytes", who, i,
                    a->a_pitch[i], a->b_pitch[i], w3);
        OFX_REQUIRE((size_t)a->h * (size_t)a->a_pitch[i] < ((size_t)1 << 31) && (size_t)a->h * (size_t)a->b_pitch[i] < ((size_t)1 << 31),
                    "%s: pair %d: a plane of 2^31 bytes or more (h * pitch)", who, i);
        OFX_REQUIRE((((uintptr_t)a->dab[i] | (uintptr_t)a->dba[i]) & 7) == 0, "%s: pair %d: the fields (d_disp_ab, d_disp_ba) must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)a->stats[i] & 7) == 0, "%s: pair %d: d_stats must be 8-byte aligned", who, i);
        dwords = dwords && ((uintptr_t)a->dst[i] & 3) == 0;
    }
    OFX_TRY(zero_stats(a->stats, a->n, 4 * (size_t)a->n_times, stream)); // (everything is checked; a slot: four words per time)
    hipLaunchKernelGGL(interp3_kernel, grid(a->w, a->h, a->n), dim3(kThreads), 0, ofx_stream(stream), *a, (int)dwords);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_interpolate_frames_3ch_batch(const uint8_t *const *d_a3, const int *a_pitches, const uint8_t *const *d_b3, const int *b_pitches,
                                                int n, int w, int h, const float *const *d_disp_ab, const float *const *d_disp_ba,
                                                const float *h_times, int n_times, uint8_t *const *d_dst3, int dst_pitch, size_t time_stride_bytes,
                                                int64_t *const *d_stats, void *stream)
{
    const char *who = "ofx_interpolate_frames_3ch_batch";
    OFX_REQUIRE(d_a3 && d_b3 && a_pitches && b_pitches, "%s: null plane or pitch array (d_a3, d_b3, a_pitches, b_pitches)", who);
    OFX_REQUIRE(d_disp_ab && d_disp_ba, "%s: null field array (d_disp_ab, d_disp_ba)", who);
    OFX_REQUIRE(d_dst3, "%s: d_dst3 is null", who);
    OFX_REQUIRE(h_times, "%s: h_times is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    OFX_REQUIRE(n_times >= 1 && n_times <= OFX_INTERP_MAX_TIMES, "%s: n_times = %d is not in 1 .. %d", who, n_times, OFX_INTERP_MAX_TIMES);
    static thread_local ofx_interp3_batch ib;
    memset(&ib, 0, sizeof ib);
    ib.n = n, ib.w = w, ib.h = h, ib.n_times = n_times, ib.dst_pitch = dst_pitch, ib.time_stride = time_stride_bytes;
    for (int k = 0; k < n_times; ++k) { // the definition's host step, in float32
        const float t = h_times[k], omt = 1.0f - t;
        ib.t[k] = t, ib.c00[k] = -(omt * t), ib.c01[k] = t * t, ib.c10[k] = omt * omt;
    }
    for (int i = 0; i < n; ++i) {
        OFX_REQUIRE(d_a3[i] && d_b3[i] && d_disp_ab[i] && d_disp_ba[i] && d_dst3[i] && (!d_stats || d_stats[i]), "%s: pair %d: a null entry in an array", who, i);
        ib.a[i] = d_a3[i], ib.a_pitch[i] = a_pitches[i], ib.b[i] = d_b3[i], ib.b_pitch[i] = b_pitches[i];
        ib.dab[i] = d_disp_ab[i], ib.dba[i] = d_disp_ba[i], ib.dst[i] = d_dst3[i];
        ib.stats[i] = d_stats ? reinterpret_cast<unsigned long long *>(d_stats[i]) : nullptr;
    }
    return ofx_interp3_batch_launch(&ib, stream); // (checks every argument before it enqueues anything)
}

extern "C" int ofx_interpolate_frames_3ch(const uint8_t *d_a3, int a_pitch, const uint8_t *d_b3, int b_pitch, int w, int h, const float *d_disp_ab,
                                          const float *d_disp_ba, const float *h_times, int n_times, uint8_t *d_dst3, int dst_pitch,
                                          size_t time_stride_bytes, int64_t *d_stats, void *stream)
{
    const char *who = "ofx_interpolate_frames_3ch";
    OFX_REQUIRE(d_a3 && d_b3, "%s: a null plane (d_a3, d_b3)", who);
    OFX_REQUIRE(d_disp_ab && d_disp_ba, "%s: a null field (d_disp_ab, d_disp_ba)", who);
    OFX_REQUIRE(d_dst3, "%s: d_dst3 is null", who);
    return ofx_interpolate_frames_3ch_batch(&d_a3, &a_pitch, &d_b3, &b_pitch, 1, w, h, &d_disp_ab, &d_disp_ba, h_times, n_times, &d_dst3, dst_pitch,
                                            time_stride_bytes, d_stats ? &d_stats : nullptr, stream);
}
