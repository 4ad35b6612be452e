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
//
// The kernel's first and last part are interp_kernel's, as text: interp_part_prologue.h with kBpp = 3 and interp_part_reduce.h;
// the host side is interp_host.h's, with every pitch against 3 * w.
#include "interp_host.h"

namespace {

using namespace quad;

constexpr int kBpp = 3;                                    // the planes' bytes per pixel (interp_part_prologue.h)
constexpr InterpNames kNames = {"d_a3", "d_b3", "d_dst3"}; // ... and their names in the entry points' messages

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));

// channel c of the left / of the right pixel of a tap row held as (dword at the tap's byte, the two bytes behind it)
__device__ __forceinline__ float tap_left(uint32_t d, int c) { return (float)((d >> (8 * c)) & 0xffu); }
__device__ __forceinline__ float tap_right(uint32_t d, uint32_t e, int c) { return c == 0 ? (float)(d >> 24) : (float)((e >> (8 * (c - 1))) & 0xffu); }

__global__ __launch_bounds__(kThreads) void interp3_kernel(const ofx_interp3_batch A, const int dwords)
{
#include "interp_part_prologue.h"
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
#include "interp_part_reduce.h"
}

} // namespace

int ofx_interp3_batch_launch(const ofx_interp3_batch *a, void *stream)
{
    return interp_launch("ofx_interp3_batch_launch", interp3_kernel, kBpp, kNames, a, stream);
}

extern "C" int ofx_interpolate_frames_3ch_batch(const uint8_t *const *d_a3, const int *a_pitches, const uint8_t *const *d_b3, const int *b_pitches,
                                                int n, int w, int h, const float *const *d_disp_ab, const float *const *d_disp_ba,
                                                const float *h_times, int n_times, uint8_t *const *d_dst3, int dst_pitch, size_t time_stride_bytes,
                                                int64_t *const *d_stats, void *stream)
{
    static thread_local ofx_interp3_batch ib;
    OFX_TRY(interp_fill_batch("ofx_interpolate_frames_3ch_batch", kNames, &ib, d_a3, a_pitches, d_b3, b_pitches, n, w, h, d_disp_ab, d_disp_ba,
                              h_times, n_times, d_dst3, dst_pitch, time_stride_bytes, d_stats));
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
