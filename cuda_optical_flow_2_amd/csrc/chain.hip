// The displacement chain (ofx_displacement_chain): the concatenation of 2 .. OFX_CHAIN_MAX_LINKS displacement fields of consecutive
// frame pairs into the field of the first frame -> the last, D_ac(x) = D_ab(x) + D_bc(x + D_ab(x)), for every pixel of n items in ONE
// launch.  The definition is the comment block "displacement chain" in include/ofx.h.  Every float32 operation below is the
// definition's, in its order; the build compiles with -ffp-contract=off, so nothing is fused.
//
// The march is quad_stage.h's, over link 0, one block column per item (the items differ in size and link count: the grid is the
// largest item's, and a block past its item's end returns).  The tap section is consistency.hip's steps 1 to 5 with scale 1, run
// once per further link around the accumulated vector: the two taps of a tap row are one 16-byte load where the lane has proved
// x0 < w - 1 for its four pixels, else two 8-byte loads with the right tap AT column x1 (the last column's right tap is the pixel
// itself; what lies behind it in memory must not reach the blend).  A pixel that has left the frame or lost its definition, and a
// pixel past the row's ragged end, gets tap offsets beyond the resource in every later link: the unit returns zeros nobody looks
// at.  The number of links is item-uniform, so the link loop's trip count is block-uniform; a wave none of whose pixels is still
// alive leaves the loop.
//
// In place on link 0: a quad's link-0 vectors are loaded by the thread that stores the quad, before the store (the NEXT quad's
// too: it is another quad).  The ragged end's load reads on into the next row, which another thread may have written already:
// those lanes are never looked at.  Links 1 .. L - 1 are gathered from anywhere and may not overlap the destination.
//
// The vectors leave by quad_part_flow_store.h, the classes by store_quad_u8, the counts by the block reduction described in
// quad_stage.h into the item's slot.
//
// Traffic: 8 B read per pixel and link, 8 B written, 1 B of mask.
#include <string.h>

#include "quad_stage.h"

namespace {

using namespace quad;

constexpr uint32_t kDeadBits = 0x7fc00000u; // both components of a vector of class 2 or 3

struct ChainItem {
    const float *link[OFX_CHAIN_MAX_LINKS];
    float *dst;
    uint8_t *mask;
    unsigned long long *stats;
    int w, h, n_links, mask_pitch, mask_dwords, pad;
};
struct ChainArgs {
    ChainItem it[OFX_STREAM_MAX_BATCH];
};

__global__ __launch_bounds__(kThreads) void chain_kernel(const ChainArgs A)
{
    __shared__ uint32_t red[kThreads / 64][3];
    const ChainItem &P = A.it[blockIdx.y];
    const int w = P.w, h = P.h, wmax = w - 1, hmax = h - 1, n_links = P.n_links;
    const int bytes = w * h * 8;
    const uint32_t qrow = quads_per_row(w), n_quads = qrow * (uint32_t)h;
    if (blockIdx.x * (uint32_t)(kQuads * kThreads) >= n_quads) return; // (block-uniform: the grid is the largest item's)
    const __amdgpu_buffer_rsrc_t rs_0 = rsrc(P.link[0], bytes), rs_f = rsrc(P.dst, bytes);
    uint8_t *mask = P.mask;
    unsigned long long *stats = P.stats;
    const float wmaxf = (float)wmax, hmaxf = (float)hmax;

    uint32_t n2 = 0, n3 = 0, n0 = 0;
    int y, x0, y_next, x0_next;
    float f[8], f_next[8];
    bool have = place(qrow, n_quads, 0, y, x0), have_next = false;
    load_field(rs_0, w, have, y, x0, f);
#pragma unroll
    for (int g = 0; g < kQuads; ++g) {
        if (!have) break;
        // the next quad's link 0 goes out before this quad's taps: its latency runs under them
        have_next = g + 1 < kQuads && place(qrow, n_quads, g + 1, y_next, x0_next);
        load_field(rs_0, w, have_next, y_next, x0_next, f_next);
        const int npx = w - x0 < 4 ? w - x0 : 4;
        const float yf = (float)y;
        // A_0; a pixel past the row's ragged end counts as gone from the start (it is neither stored nor counted)
        float fu[4], fv[4];
        uint32_t cls[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) fu[k] = f[2 * k], fv[k] = f[2 * k + 1], cls[k] = k < npx ? OFX_CHAIN_OK : OFX_CHAIN_LEAVES;
#pragma nounroll
        for (int j = 1; j < n_links; ++j) {
            const bool any = (cls[0] == OFX_CHAIN_OK) | (cls[1] == OFX_CHAIN_OK) | (cls[2] == OFX_CHAIN_OK) | (cls[3] == OFX_CHAIN_OK);
            if (__builtin_amdgcn_ballot_w64(any) == 0) break; // (wave-uniform: nobody here reads this link or a later one)
            const __amdgpu_buffer_rsrc_t rs_j = rsrc(P.link[j], bytes);
            // steps 1 to 4
            float fx[4], fy[4];
            uint32_t off0[4], off1[4], offr0[4], offr1[4];
            bool wide = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float px = (float)(x0 + k) + fu[k], py = yf + fv[k];
                const bool ok = __builtin_fabsf(px) <= 1e9f && __builtin_fabsf(py) <= 1e9f; // (a NaN fails)
                const bool gone = px < 0.0f || px > wmaxf || py < 0.0f || py > hmaxf;
                const bool alive = cls[k] == OFX_CHAIN_OK;
                const bool live = alive && ok && !gone;
                cls[k] = !alive ? cls[k] : !ok ? OFX_CHAIN_UNDEFINED : gone ? OFX_CHAIN_LEAVES : OFX_CHAIN_OK;
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
                    ta[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_j, off0[k], 0, 0));
                    tb[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_j, off1[k], 0, 0));
                }
            } else {
                f32x2 l0[4], r0[4], l1[4], r1[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    l0[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_j, off0[k], 0, 0));
                    r0[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_j, offr0[k], 0, 0));
                    l1[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_j, off1[k], 0, 0));
                    r1[k] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_j, offr1[k], 0, 0));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ta[k][0] = l0[k][0], ta[k][1] = l0[k][1], ta[k][2] = r0[k][0], ta[k][3] = r0[k][1];
                    tb[k][0] = l1[k][0], tb[k][1] = l1[k][1], tb[k][2] = r1[k][0], tb[k][3] = r1[k][1];
                }
            }
            // the taps have arrived: the blend, per component, and step 5
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float ru = blend(ta[k][0], ta[k][2], tb[k][0], tb[k][2], fx[k], fy[k]);
                const float rv = blend(ta[k][1], ta[k][3], tb[k][1], tb[k][3], fx[k], fy[k]);
                const float su = fu[k] + ru, sv = fv[k] + rv;
                const bool finite = __builtin_fabsf(su) <= 3.402823466e+38f && __builtin_fabsf(sv) <= 3.402823466e+38f; // (a NaN fails)
                if (cls[k] == OFX_CHAIN_OK) {
                    fu[k] = su, fv[k] = sv;
                    if (!finite) cls[k] = OFX_CHAIN_UNDEFINED;
                }
            }
        }
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = cls[k];
            if (c != OFX_CHAIN_OK) fu[k] = fv[k] = __builtin_bit_cast(float, kDeadBits);
            out |= c << (8 * k);
            if (k < npx) n2 += c == OFX_CHAIN_LEAVES, n3 += c == OFX_CHAIN_UNDEFINED, n0 += c == OFX_CHAIN_OK;
        }
        // the chained quad leaves from registers
#include "quad_part_flow_store.h"
        if (mask) store_quad_u8(mask + (size_t)y * (size_t)P.mask_pitch + (size_t)x0, out, npx, P.mask_dwords);
        have = have_next, y = y_next, x0 = x0_next;
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = f_next[k];
    }
    if (!stats) return; // (block-uniform)
    // the block reduction (the rule: quad_stage.h), written out as in consistency_kernel
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n2 += __shfl_xor(n2, o);
        n3 += __shfl_xor(n3, o);
        n0 += __shfl_xor(n0, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = n2, red[threadIdx.x >> 6][1] = n3, red[threadIdx.x >> 6][2] = n0;
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

struct Span {
    uintptr_t lo, hi;
};
inline bool apart(Span a, Span b) { return a.hi <= b.lo || b.hi <= a.lo; }

} // namespace

extern "C" int ofx_displacement_chain(const ofx_chain_desc *items, int n, void *stream)
{
    const char *who = "ofx_displacement_chain";
    OFX_REQUIRE(items != nullptr, "%s: items is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_STREAM_MAX_BATCH, "%s: n = %d is not in 1 .. %d", who, n, OFX_STREAM_MAX_BATCH);
    static thread_local ChainArgs A;
    memset(&A, 0, sizeof A);
    unsigned long long *slots[OFX_STREAM_MAX_BATCH];
    int wmost = 1, hmost = 1;
    unsigned blocks = 0;
    for (int i = 0; i < n; ++i) {
        const ofx_chain_desc &d = items[i];
        OFX_REQUIRE(d.n_links >= 2 && d.n_links <= OFX_CHAIN_MAX_LINKS, "%s: item %d: n_links = %d is not in 2 .. %d", who, i, d.n_links, OFX_CHAIN_MAX_LINKS);
        OFX_REQUIRE(d.d_dst != nullptr, "%s: item %d: d_dst is null", who, i);
        OFX_REQUIRE(d.w >= 1 && d.h >= 1, "%s: item %d: the size %d x %d must be positive", who, i, d.w, d.h);
        OFX_REQUIRE((size_t)d.w * (size_t)d.h < ((size_t)1 << 28), "%s: item %d: w * h = %d x %d is not below 2^28", who, i, d.w, d.h);
        OFX_REQUIRE(((uintptr_t)d.d_dst & 7) == 0, "%s: item %d: d_dst must be 8-byte aligned", who, i);
        OFX_REQUIRE(((uintptr_t)d.d_stats & 7) == 0, "%s: item %d: d_stats must be 8-byte aligned", who, i);
        OFX_REQUIRE(d.d_mask == nullptr || d.mask_pitch >= d.w, "%s: item %d: mask_pitch = %d is below the width %d", who, i, d.mask_pitch, d.w);
        const size_t fb = (size_t)d.w * (size_t)d.h * 8;
        const Span dst = {(uintptr_t)d.d_dst, (uintptr_t)d.d_dst + fb};
        const Span msk = {(uintptr_t)d.d_mask, (uintptr_t)d.d_mask + (size_t)(d.h - 1) * (size_t)d.mask_pitch + (size_t)d.w};
        const Span sts = {(uintptr_t)d.d_stats, (uintptr_t)d.d_stats + 4 * sizeof(int64_t)};
        OFX_REQUIRE(!d.d_mask || apart(msk, dst), "%s: item %d: d_mask and d_dst overlap", who, i);
        OFX_REQUIRE(!d.d_stats || apart(sts, dst), "%s: item %d: d_stats and d_dst overlap", who, i);
        OFX_REQUIRE(!d.d_stats || !d.d_mask || apart(sts, msk), "%s: item %d: d_stats and d_mask overlap", who, i);
        ChainItem &P = A.it[i];
        for (int k = 0; k < d.n_links; ++k) {
            OFX_REQUIRE(d.d_link[k] != nullptr, "%s: item %d: link %d: d_link is null", who, i, k);
            OFX_REQUIRE(((uintptr_t)d.d_link[k] & 7) == 0, "%s: item %d: link %d: d_link must be 8-byte aligned", who, i, k);
            const Span lnk = {(uintptr_t)d.d_link[k], (uintptr_t)d.d_link[k] + fb};
            // (in place: d_dst may be exactly link 0)
            OFX_REQUIRE((k == 0 && d.d_link[0] == d.d_dst) || apart(lnk, dst), "%s: item %d: link %d: d_link and d_dst overlap", who, i, k);
            OFX_REQUIRE(!d.d_mask || apart(lnk, msk), "%s: item %d: link %d: d_link and d_mask overlap", who, i, k);
            P.link[k] = d.d_link[k];
        }
        P.dst = d.d_dst, P.mask = d.d_mask, P.stats = slots[i] = reinterpret_cast<unsigned long long *>(d.d_stats);
        P.w = d.w, P.h = d.h, P.n_links = d.n_links, P.mask_pitch = d.d_mask ? d.mask_pitch : 0;
        P.mask_dwords = (((uintptr_t)d.d_mask | (uintptr_t)P.mask_pitch) & 3) == 0;
        const unsigned b = grid(d.w, d.h, 1).x;
        if (b > blocks) blocks = b, wmost = d.w, hmost = d.h;
    }
    OFX_TRY(zero_stats(slots, n, 4, stream)); // (everything is checked)
    hipLaunchKernelGGL(chain_kernel, grid(wmost, hmost, n), dim3(kThreads), 0, ofx_stream(stream), A);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
