// Coarse-to-fine propagation (ofx_flow_prolong): a level's starting flow from the whole flow of the level above and, fused, the
// next image warped by it.  The definition is the comment block "coarse-to-fine propagation" in include/ofx.h; every float32
// operation below is the definition's, in its order, and the build compiles with -ffp-contract=off, so nothing is fused.
//
// One launch, blockIdx.y = the descriptor; the march is quad_stage.h's.  A thread owns four adjacent fine pixels of one row.  Their
// columns x0 .. x0 + 3 (x0 a multiple of 4) sample the coarse columns x0/2, x0/2 + 1 and x0/2 + 2, each clamped to wc - 1, on the
// coarse rows y0 and y1: six 8-byte loads through a buffer resource of exactly the coarse field's bytes, all issued before the
// first is used, the NEXT quad's six before this quad's warp taps.  (On an even row y1's loads repeat y0's offsets.)  Each tap is
// sanitised as it arrives; the even positions take their tap without arithmetic, the odd ones a + 0.5f * (b - a) -- also where
// the clamp has made a and b the same tap, as the definition does.
//
// The four fine vectors stay in registers: they leave by quad_part_flow_store.h and feed the fused warp, quad_part_warp.h (the
// rules of both are stated there).  The warped quad leaves as one dword where it is whole and aligned.
//
// Traffic: 8 B written and 2 B of coarse field read per fine pixel, 1 B of taps (cache-resident neighbours) and 1 B written: ~12 B.
#include <string.h>

#include "quad_stage.h"

namespace {

using namespace quad;

struct ProlongLevel {
    const float *coarse;
    float *fine;
    const uint8_t *src;
    uint8_t *dst;
    int wc, hc, w, h, src_pitch, dst_pitch, dwords;
    float scale, max_px;
};
struct ProlongArgs {
    ProlongLevel lv[OFX_MAX_LEVELS];
};

// the six coarse taps of a quad: T[2 * (3 * r + c)] / [.. + 1] = (u, v) of coarse column c (of three) on coarse row r (of two)
__device__ __forceinline__ void load_taps(const __amdgpu_buffer_rsrc_t &rs, int wc, int hc, bool in, int y, int x0, float *T)
{
    const int xc = x0 >> 1, cy0 = min(y >> 1, hc - 1), cy1 = (y & 1) ? min(cy0 + 1, hc - 1) : cy0;
    const int c0 = min(xc, wc - 1), c1 = min(xc + 1, wc - 1), c2 = min(xc + 2, wc - 1);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t row = (uint32_t)((r ? cy1 : cy0) * wc);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t o = in ? 8u * (row + (uint32_t)(c == 0 ? c0 : c == 1 ? c1 : c2)) : kNowhere;
            const f32x2 t = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, o, 0, 0));
            T[2 * (3 * r + c)] = t[0], T[2 * (3 * r + c) + 1] = t[1];
        }
    }
}

__global__ __launch_bounds__(kThreads) void prolong_kernel(const ProlongArgs A)
{
    const ProlongLevel &P = A.lv[blockIdx.y];
    const int w = P.w, h = P.h, wc = P.wc, hc = P.hc, wmax = w - 1, hmax = h - 1;
    const uint32_t qrow = quads_per_row(w), n_quads = qrow * (uint32_t)h;
    if ((blockIdx.x * kQuads) * kThreads >= n_quads) return; // (the grid is the largest descriptor's)
    const float scale = P.scale, max_px = P.max_px;
    const bool limit = max_px > 0.0f;
    const int sp = P.src_pitch;
    const bool warp = P.src != nullptr;
    const __amdgpu_buffer_rsrc_t rs_c = rsrc(P.coarse, wc * hc * 8), rs_f = rsrc(P.fine, w * h * 8);
    const __amdgpu_buffer_rsrc_t rs_s = rsrc(P.src, warp ? hmax * sp + w : 0);
    const float wmaxf = (float)wmax, hmaxf = (float)hmax;

    int y, x0, y_next = 0, x0_next = 0;
    float T[12], T_next[12];
    bool have = place(qrow, n_quads, 0, y, x0), have_next = false;
    load_taps(rs_c, wc, hc, have, y, x0, T);
#pragma nounroll
    for (int g = 0; g < kQuads; ++g) {
        if (!have) break;
        // the next quad's coarse taps go out before this quad's warp taps: their latency runs under them
        have_next = g + 1 < kQuads && place(qrow, n_quads, g + 1, y_next, x0_next);
        load_taps(rs_c, wc, hc, have_next, y_next, x0_next, T_next);
        const int npx = w - x0 < 4 ? w - x0 : 4;
        // 1. sanitise the six taps
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const float u = T[2 * t], v = T[2 * t + 1];
            bool bad = !(__builtin_fabsf(u) < __builtin_inff() && __builtin_fabsf(v) < __builtin_inff()); // (a NaN fails)
            if (limit) bad = bad || __builtin_fabsf(scale * u) > max_px || __builtin_fabsf(scale * v) > max_px;
            T[2 * t] = bad ? 0.0f : u, T[2 * t + 1] = bad ? 0.0f : v;
        }
        // 2. horizontally on the two coarse rows, then vertically; 3. times two
        const bool odd_y = (y & 1) != 0;
        float fu[4], fv[4];
#pragma unroll
        for (int comp = 0; comp < 2; ++comp) {
            float hz[2][4];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float a = T[2 * (3 * r) + comp], b = T[2 * (3 * r + 1) + comp], c = T[2 * (3 * r + 2) + comp];
                hz[r][0] = a;
                hz[r][1] = a + 0.5f * (b - a);
                hz[r][2] = b;
                hz[r][3] = b + 0.5f * (c - b);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float mid = hz[0][k] + 0.5f * (hz[1][k] - hz[0][k]);
                const float val = 2.0f * (odd_y ? mid : hz[0][k]);
                if (comp == 0) fu[k] = val;
                else fv[k] = val;
            }
        }
        // the four fine vectors leave from registers
#include "quad_part_flow_store.h"
        if (warp) { // (block-uniform)
            // 4. the warp of the quad by the vectors it holds
#include "quad_part_warp.h"
            store_quad_u8(P.dst + (size_t)y * (size_t)P.dst_pitch + (size_t)x0, out, npx, P.dwords);
        }
        have = have_next, y = y_next, x0 = x0_next;
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = T_next[k];
    }
}

} // namespace

extern "C" int ofx_flow_prolong(const ofx_prolong_desc *levels, int n, void *stream)
{
    const char *who = "ofx_flow_prolong";
    OFX_REQUIRE(levels != nullptr, "%s: levels is null", who);
    OFX_REQUIRE(n >= 1 && n <= OFX_MAX_LEVELS, "%s: n = %d is not in 1 .. %d", who, n, OFX_MAX_LEVELS);
    static thread_local ProlongArgs A;
    memset(&A, 0, sizeof A);
    unsigned blocks = 1;
    for (int i = 0; i < n; ++i) {
        const ofx_prolong_desc &d = levels[i];
        OFX_REQUIRE(d.d_coarse && d.d_fine, "%s: level %d: d_coarse or d_fine is null", who, i);
        OFX_REQUIRE(d.wc > 0 && d.hc > 0, "%s: level %d: the coarse size %d x %d must be positive", who, i, d.wc, d.hc);
        OFX_REQUIRE((size_t)d.wc * (size_t)d.hc < ((size_t)1 << 26), "%s: level %d: the coarse field %d x %d is more than this build takes", who, i, d.wc, d.hc);
        OFX_REQUIRE((d.w == 2 * d.wc || d.w == 2 * d.wc + 1) && (d.h == 2 * d.hc || d.h == 2 * d.hc + 1),
                    "%s: level %d: the fine size %d x %d is not 2 * wc (+ 1) x 2 * hc (+ 1) of the coarse %d x %d", who, i, d.w, d.h, d.wc, d.hc);
        OFX_REQUIRE((size_t)d.w * (size_t)d.h < ((size_t)1 << 28), "%s: level %d: w * h = %d x %d is more than this build takes (2^28 pixels)", who, i, d.w, d.h);
        OFX_REQUIRE(__builtin_isfinite(d.max_px) && d.max_px >= 0.0f, "%s: level %d: max_px must be finite and >= 0", who, i);
        OFX_REQUIRE(__builtin_isfinite(d.scale), "%s: level %d: the scale must be finite", who, i);
        OFX_REQUIRE((((uintptr_t)d.d_coarse | (uintptr_t)d.d_fine) & 7) == 0, "%s: level %d: d_coarse and d_fine must be 8-byte aligned", who, i);
        const uintptr_t c0 = (uintptr_t)d.d_coarse, c1 = c0 + (size_t)d.wc * (size_t)d.hc * 8, f0 = (uintptr_t)d.d_fine, f1 = f0 + (size_t)d.w * (size_t)d.h * 8;
        OFX_REQUIRE(f1 <= c0 || c1 <= f0, "%s: level %d: d_fine overlaps d_coarse", who, i);
        OFX_REQUIRE((d.d_src != nullptr) == (d.d_dst != nullptr), "%s: level %d: d_src and d_dst go together (both, or neither for the flow alone)", who, i);
        ProlongLevel &P = A.lv[i];
        P = ProlongLevel{d.d_coarse, d.d_fine, d.d_src, d.d_dst, d.wc, d.hc, d.w, d.h, 0, 0, 0, d.scale, d.max_px};
        if (d.d_src) {
            OFX_TRY(check_warp_planes(who, "level", i, d.w, d.h, d.d_src, d.src_pitch, d.d_dst, d.dst_pitch, &P.dwords));
            P.src_pitch = d.src_pitch, P.dst_pitch = d.dst_pitch;
        }
        const unsigned b = grid(d.w, d.h, 1).x;
        blocks = b > blocks ? b : blocks;
    }
    hipLaunchKernelGGL(prolong_kernel, dim3(blocks, n), dim3(kThreads), 0, ofx_stream(stream), A);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}
