// The quad march: what motion_ring.hip, consistency.hip, interp.hip, interp3.hip, prolong.hip and median.hip share ("the
// quad march").  Each of their kernels runs one block column per pair, item or level (blockIdx.y); a thread owns four adjacent
// pixels of a row (a quad) and takes kQuads quads, one after the other, kThreads apart in row-major order (median.hip: in tiles of
// its own).  A quad's 8-byte-per-pixel field comes as two 16-byte buffer loads, the NEXT quad's field goes out before this quad's
// taps so that its latency runs under them, and all tap loads of a quad are issued before the first is used.  Every load goes
// through a buffer resource of exactly the plane's or the field's bytes, and what must read as 0 is given the offset kNowhere beyond
// it: the unit returns 0, and no coordinate, however wild, reads outside a plane or a field.  The loop itself stays in each kernel
// (its unrolling is the kernel's choice); the parts it is made of, and the host side of a launch, are here.
//
// Parts that two kernels share but that are no function here are TEXT, included at the place of use: quad_part_warp.h (the fused
// warp) and quad_part_flow_store.h (the store of a quad's vectors) in prolong_kernel and median_march, interp_part_prologue.h and
// interp_part_reduce.h in interp_kernel and interp3_kernel.  Behind a function or template -- forced inline, arguments by value or
// by reference -- each of them came out of the compiler with the kernel around it in another order; as text, and with the bytes
// per pixel as a constant of the file, every kernel is the one it was (profiles/refactor_quad_parts.txt).  Host code has no such
// limit: interp_host.h holds the one builder and the one launch body of the two interpolation units.
#pragma once
#include <initializer_list>

#include "ofx_internal.h"

namespace quad {

constexpr int kThreads = 256;
constexpr int kQuads = 4;                      // quads (four pixels) per thread, kThreads apart in row-major order
constexpr uint32_t kNowhere = 0x80000000u;     // a buffer offset beyond every plane and field (both are < 2^31 bytes): loads 0

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// a raw buffer resource of exactly `bytes` bytes: a load at an offset beyond them returns 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *base, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00027000);
}

// quads per row of a w-wide image: the row's ragged end is a quad of its own, of w - x0 < 4 pixels
__device__ __forceinline__ uint32_t quads_per_row(int w) { return (uint32_t)(w + 3) >> 2; }

// the place (y, x0) of this thread's g-th quad; false: past the end of the image
__device__ __forceinline__ bool place(uint32_t qrow, uint32_t n_quads, int g, int &y, int &x0)
{
    const uint32_t q = (blockIdx.x * kQuads + g) * kThreads + threadIdx.x;
    y = (int)(q / qrow), x0 = 4 * (int)(q - (uint32_t)y * qrow);
    return q < n_quads;
}

// a quad's field (u, v of four pixels) by two 16-byte loads through a resource of the field's size: no branch for the row's ragged
// end (its last pixels get the next row's vectors, or zeros past the field: they are never looked at) nor for a quad past the end
__device__ __forceinline__ void load_field(const __amdgpu_buffer_rsrc_t &rs, int w, bool in, int y, int x0, float *f)
{
    const uint32_t o = in ? 8u * ((uint32_t)y * (uint32_t)w + (uint32_t)x0) : kNowhere;
    const f32x4 a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0));
    const f32x4 c = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 16, 0));
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = a[k], f[4 + k] = c[k];
}

// a quad of bytes (pixel k in byte k of `out`) leaves as one dword where the quad is whole and the caller has proved the address
// 4-byte aligned (`dwords`), else as its first n bytes.  (interp_kernel writes this out in its time loop, for the reason given at
// the reduction below.)
__device__ __forceinline__ void store_quad_u8(uint8_t *d, uint32_t out, int n, int dwords)
{
    if (n == 4 && dwords) {
        *reinterpret_cast<uint32_t *>(d) = out;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) d[k] = (uint8_t)(out >> (8 * k));
    }
}

// the bilinear blend of four taps, in the definitions' operation order (the build has -ffp-contract=off)
__device__ __forceinline__ float blend(float p00, float p01, float p10, float p11, float fx, float fy)
{
    const float a = p00 + fx * (p01 - p00);
    const float c = p10 + fx * (p11 - p10);
    return a + fy * (c - a);
}
// ... of byte taps: (left | right << 8) of the upper tap row in r0, of the lower in r1
__device__ __forceinline__ float blend_u8(uint32_t r0, uint32_t r1, float fx, float fy)
{
    return blend((float)(r0 & 0xffu), (float)((r0 >> 8) & 0xffu), (float)(r1 & 0xffu), (float)((r1 >> 8) & 0xffu), fx, fy);
}
// ... and a blend back to a byte: warp_row_finish's rounding
__device__ __forceinline__ uint32_t round_u8(float v) { return (uint32_t)(int)(v + 0.5f) & 0xffu; }

// The block's reduction of three 32-bit per-thread counters into a four-word stats slot -- the rule; motion_ring_kernel and
// consistency_kernel each write it out, the two interpolation kernels include interp_part_reduce.h: a wave reduction by __shfl_xor; lane 0 of each wave leaves the wave's three sums in LDS; after ONE __syncthreads()
// (interp_kernel: one for all its times) the thread that owns a counter adds the four waves' sums and sends one 64-bit atomicAdd to
// words 1 to 3 of the slot, a zero sum is not sent; word 0 gets w * h from one thread of block 0 alone.  The launch zeroes the slot
// on the stream first (zero_stats).  It is no function here because every form that was tried -- around the __shfl_xor loop alone
// even, by value or by reference -- changed the order or the register numbers of the kernels' other instructions
// (profiles/refactor_output_stages.txt).

// ---- the host side of a launch ----

// What a kernel requires of a plane it reads or writes through offsets: a row pitch of at least a row's bytes, and the plane below
// 2^31 bytes, so that every offset fits 31 bits and kNowhere lies beyond it.  `who` names the entry point, `noun` and i the pair,
// item or level, `what` the pitch (its argument's name, where it has one).
inline int check_plane(const char *who, const char *noun, int i, int h, const char *what, int pitch, int row_bytes, int w)
{
    OFX_REQUIRE(pitch >= row_bytes, "%s: %s %d: %s %d is below the %d bytes of a row of width %d", who, noun, i, what, pitch, row_bytes, w);
    OFX_REQUIRE((size_t)h * (size_t)pitch < ((size_t)1 << 31), "%s: %s %d: a plane of 2^31 bytes or more (h * pitch)", who, noun, i);
    return OFX_OK;
}

// What a fused warp (quad_part_warp.h) requires of its two byte planes of w x h pixels: check_plane's rules for both, and d_dst not
// overlapping d_src (a warp is out of place).  *dwords: a whole quad may leave as one dword (d_dst and dst_pitch 4-byte aligned).
inline int check_warp_planes(const char *who, const char *noun, int i, int w, int h, const uint8_t *d_src, int src_pitch, const uint8_t *d_dst,
                             int dst_pitch, int *dwords)
{
    OFX_TRY(check_plane(who, noun, i, h, "src_pitch", src_pitch, w, w));
    OFX_TRY(check_plane(who, noun, i, h, "dst_pitch", dst_pitch, w, w));
    const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (size_t)(h - 1) * (size_t)src_pitch + (size_t)w;
    const uintptr_t t0 = (uintptr_t)d_dst, t1 = t0 + (size_t)(h - 1) * (size_t)dst_pitch + (size_t)w;
    OFX_REQUIRE(t1 <= s0 || s1 <= t0, "%s: %s %d: d_dst overlaps d_src", who, noun, i);
    *dwords = (((uintptr_t)d_dst | (uintptr_t)dst_pitch) & 3) == 0;
    return OFX_OK;
}

// What the entry points require of a batch before anything is enqueued.  Per pair: check_plane's rules for every plane (pitches:
// one array per plane; bpp: the planes' bytes per pixel, a row is bpp * w bytes), every field (fields: one array per field) present
// and 8-byte aligned, the stats slot 8-byte aligned.  w * h < 2^28: a field is read through a buffer resource, 8 bytes per pixel,
// below 2^31 bytes (and bpp * w cannot overflow: w > 0 is asked first).
inline int check_batch(const char *who, int n, int w, int h, int bpp, std::initializer_list<const int *> pitches,
                       std::initializer_list<const float *const *> fields, unsigned long long *const *stats)
{
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: bad arguments: n = %d pairs is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    OFX_REQUIRE(w > 0 && h > 0, "%s: w = %d, h = %d must be positive", who, w, h);
    OFX_REQUIRE((size_t)w * (size_t)h < ((size_t)1 << 28), "%s: w * h = %d x %d is more than this build takes (2^28 pixels)", who, w, h);
    for (int i = 0; i < n; ++i) {
        for (const int *pitch : pitches) OFX_TRY(check_plane(who, "pair", i, h, "a row pitch", pitch[i], bpp * w, w));
        for (const float *const *field : fields) {
            OFX_REQUIRE(field[i], "%s: pair %d: a null field", who, i);
            OFX_REQUIRE(((uintptr_t)field[i] & 7) == 0, "%s: pair %d: the fields must be 8-byte aligned", who, i);
        }
        OFX_REQUIRE(((uintptr_t)stats[i] & 7) == 0, "%s: pair %d: the stats must be 8-byte aligned", who, i);
    }
    return OFX_OK;
}

// zero the pairs' stats slots (`words` 64-bit words each) on the stream, one launch per run of consecutive slots (a ring that
// wraps: two); a pair without a slot is skipped
inline int zero_stats(unsigned long long *const *stats, int n, size_t words, void *stream)
{
    for (int i = 0; i < n;) {
        int e = i + 1;
        if (!stats[i]) {
            i = e;
            continue;
        }
        while (e < n && stats[e] == stats[i] + words * (size_t)(e - i)) ++e;
        OFX_TRY(ofx_zero_words(stats[i], (size_t)(e - i) * words, ofx_stream(stream)));
        i = e;
    }
    return OFX_OK;
}

// the grid of a march over n pairs of w x h pixels
inline dim3 grid(int w, int h, int n)
{
    const unsigned quads = (unsigned)((w + 3) >> 2) * (unsigned)h, per_block = kThreads * kQuads;
    return dim3((quads + per_block - 1) / per_block, n);
}

} // namespace quad
