// The stream pipeline's motion-compensation stage (ofx_session_stream_motion) and the stateless call underneath
// (ofx_motion_compensate): for every pair one call of the pipeline completes, in ONE launch, the next image pulled back onto
// the previous one by the pair's flow, and four integer sums that say how well that worked.  The definition is the comment
// block "motion compensation" in include/ofx.h: mc = ofx_warp_levels(ofx_shift_1ch(next, uv), flow, scale), bit for bit.
//
// The shift is fused: no shifted plane exists.  A thread owns four adjacent pixels of a row.  It forms the tap coordinates in
// SHIFTED space exactly as warp_row_prepare (lk_body_warp.h) does, then sends every tap's row and column through the shift's
// map (int)((float)j + u), in range when > -1 and < w (rows: v, h); a tap whose target is out of range falls back to the
// shift's out-of-image rule: the unshifted byte at the tap's own position while 3 * (y * w + x) < w * h, else 0.
//
// The map is no translation near zero: truncation sends j + u in (-1, 0) and in [0, 1) both to column 0.  So the trick of
// lk_body_warp.h -- one dword AT the left tap's byte holds both taps of a row -- only holds where the two taps' mapped columns
// are consecutive and in range.  A lane proves that for its four pixels (both tap rows in range too, and the dword inside the
// plane) and then takes eight dword loads; any other lane takes sixteen byte loads, each tap mapped on its own.  Every load
// goes through a buffer resource of exactly the plane's (h - 1) * pitch + w bytes, and a tap that the rule sets to 0 is given
// an offset beyond it: the unit returns 0, and no coordinate, however wild, reads outside the plane.
//
// The march is quad_stage.h's.  prev's dword and the unshifted next's (for the sums) go out with a quad's taps.  The sums are
// integers: per-thread v_sad_u8 partial sums, then the block reduction described in quad_stage.h into the pair's slot.  (A lane on the byte
// path waits for its sixteen taps inside that branch, before prev's and next's dwords go out: a wave with a border lane runs both
// branches in turn.  Only waves at the image's borders have one.)
#include <string.h>

#include "quad_stage.h"

namespace {

using namespace quad;

// four bytes at `off` of a plane of `bytes` bytes: one dword where it lies inside, else its first n bytes one by one
__device__ __forceinline__ uint32_t load_quad(const __amdgpu_buffer_rsrc_t &rs, uint32_t off, int bytes, int n)
{
    if (off + 4u <= (uint32_t)bytes) return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) r |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, off + k, 0, 0) << (8 * k);
    return r;
}

__global__ __launch_bounds__(kThreads) void motion_ring_kernel(const ofx_motion_batch A)
{
    __shared__ uint32_t red[kThreads / 64][3];
    const int b = blockIdx.y;
    const int w = A.w, h = A.h, wmax = w - 1, hmax = h - 1;
    const int pp = A.prev_pitch[b], np = A.next_pitch[b];
    const int prev_bytes = hmax * pp + w, next_bytes = hmax * np + w;
    const __amdgpu_buffer_rsrc_t rs_prev = rsrc(A.prev[b], prev_bytes), rs_next = rsrc(A.next[b], next_bytes);
    const float *flow = A.flow[b];
    uint8_t *dst = A.dst[b];
    unsigned long long *stats = A.stats[b];
    float u = 0.0f, v = 0.0f; // (NULL: no shift -- the map is the identity then)
    if (A.uv[b]) u = A.uv[b][0], v = A.uv[b][1];
    const float wf = (float)w, hf = (float)h, wmaxf = (float)wmax, hmaxf = (float)hmax, scale = A.scale;
    const uint32_t third = ((uint32_t)w * (uint32_t)h + 2u) / 3u; // 3 * pos < w * h  <=>  pos < ceil(w * h / 3)
    const uint32_t qrow = quads_per_row(w), n_quads = qrow * (uint32_t)h;

    // the shift's map of one coordinate: in range?  and where to
    auto map_col = [&](int x, int &nx) -> bool {
        const float t = (float)x + u;
        const bool in = t > -1.0f && t < wf;
        nx = in ? (int)t : 0;
        return in;
    };
    auto map_row = [&](int y, int &ny) -> bool {
        const float t = (float)y + v;
        const bool in = t > -1.0f && t < hf;
        ny = in ? (int)t : 0;
        return in;
    };

    // (the ragged end's pixels are computed like the others)
    const __amdgpu_buffer_rsrc_t rs_flow = rsrc(flow, w * h * 8);

    uint32_t sad_raw = 0, sad_mc = 0, unwarped = 0;
    int y, x0, y_next, x0_next;
    float f[8], f_next[8];
    bool have = place(qrow, n_quads, 0, y, x0), have_next = false;
    load_field(rs_flow, w, have, y, x0, f);
#pragma unroll
    for (int g = 0; g < kQuads; ++g) {
        if (!have) break;
        // the next quad's flow goes out before this quad's taps: its latency runs under them
        have_next = g + 1 < kQuads && place(qrow, n_quads, g + 1, y_next, x0_next);
        load_field(rs_flow, w, have_next, y_next, x0_next, f_next);
        const int npx = w - x0 < 4 ? w - x0 : 4;
        float fu[4], fv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) fu[k] = f[2 * k], fv[k] = f[2 * k + 1];
        // the taps in shifted space (warp_row_prepare's operation order); a pixel past the row's end has zero flow and its
        // clamped column: taps inside the plane, bytes nobody looks at
        const float xf0 = (float)x0, yf = (float)y;
        float fx[4], fy[4];
        int xi[4], x1[4], ya[4], yb[4];
        uint32_t bad = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float xr = xf0 + (float)k;
            const float sxr = xr + scale * fu[k], syr = yf + scale * fv[k];
            const bool ok = __builtin_fabsf(sxr) <= 1e9f && __builtin_fabsf(syr) <= 1e9f; // (NaN fails)
            if (k < npx && !ok) ++bad;
            const float sx = __builtin_amdgcn_fmed3f(ok ? sxr : xr, 0.0f, wmaxf);
            const float sy = __builtin_amdgcn_fmed3f(ok ? syr : yf, 0.0f, hmaxf);
            xi[k] = (int)sx;
            ya[k] = (int)sy;
            fx[k] = __builtin_amdgcn_fractf(sx); // == sx - (float)xi: sx >= 0, the difference is exact
            fy[k] = __builtin_amdgcn_fractf(sy);
            x1[k] = min(xi[k] + 1, wmax), yb[k] = min(ya[k] + 1, hmax);
        }
        // through the shift's map.  off[k][r]: where tap (row r, left column) of pixel k is read, when the dword form holds
        uint32_t off[4][2];
        bool dword = true;
        int cx[4][2], ry[4][2];
        bool cin[4][2], rin[4][2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cin[k][0] = map_col(xi[k], cx[k][0]), cin[k][1] = map_col(x1[k], cx[k][1]);
            rin[k][0] = map_row(ya[k], ry[k][0]), rin[k][1] = map_row(yb[k], ry[k][1]);
            // (the right tap of column w - 1 is the pixel itself, its fraction 0: byte 1 of the dword is not looked at)
            const bool cols = cin[k][0] && (x1[k] == xi[k] || (cin[k][1] && cx[k][1] == cx[k][0] + 1));
            off[k][0] = (uint32_t)(ry[k][0] * np + cx[k][0]), off[k][1] = (uint32_t)(ry[k][1] * np + cx[k][0]);
            dword = dword && cols && rin[k][0] && rin[k][1] && max(off[k][0], off[k][1]) + 4u <= (uint32_t)next_bytes;
        }
        uint32_t ra[4], rb[4]; // per pixel (left, right) of rows ya and yb in bytes 0 and 1
        if (dword) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ra[k] = __builtin_amdgcn_raw_buffer_load_b32(rs_next, off[k][0], 0, 0);
                rb[k] = __builtin_amdgcn_raw_buffer_load_b32(rs_next, off[k][1], 0, 0);
            }
        } else {
            uint32_t t[4][2][2];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int ty = r ? yb[k] : ya[k], tx = c ? x1[k] : xi[k];
                        const uint32_t own = (uint32_t)ty * (uint32_t)w + (uint32_t)tx < third ? (uint32_t)(ty * np + tx) : kNowhere;
                        const uint32_t o = rin[k][r] && cin[k][c] ? (uint32_t)(ry[k][r] * np + cx[k][c]) : own;
                        t[k][r][c] = __builtin_amdgcn_raw_buffer_load_b8(rs_next, o, 0, 0);
                    }
#pragma unroll
            for (int k = 0; k < 4; ++k) ra[k] = t[k][0][0] | (t[k][0][1] << 8), rb[k] = t[k][1][0] | (t[k][1][1] << 8);
        }
        uint32_t pv = 0, nv = 0;
        if (stats) {
            pv = load_quad(rs_prev, (uint32_t)(y * pp + x0), prev_bytes, npx);
            nv = load_quad(rs_next, (uint32_t)(y * np + x0), next_bytes, npx);
        }
        // the taps have arrived: the blend of warp_row_finish
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) out |= round_u8(blend_u8(ra[k], rb[k], fx[k], fy[k])) << (8 * k);
        if (dst) store_quad_u8(dst + (size_t)y * (size_t)A.dst_pitch + (size_t)x0, out, npx, A.dst_dwords);
        if (stats) {
            const uint32_t m = npx == 4 ? 0xffffffffu : (1u << (8 * npx)) - 1u;
            sad_raw = __builtin_amdgcn_sad_u8(pv & m, nv & m, sad_raw);
            sad_mc = __builtin_amdgcn_sad_u8(pv & m, out & m, sad_mc);
            unwarped += bad;
        }
        have = have_next, y = y_next, x0 = x0_next;
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = f_next[k];
    }
    if (!stats) return; // (block-uniform)
    // the block reduction (the rule: quad_stage.h), written out: behind a function the kernel's other instructions come out in another order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sad_raw += __shfl_xor(sad_raw, o);
        sad_mc += __shfl_xor(sad_mc, o);
        unwarped += __shfl_xor(unwarped, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = sad_raw, red[threadIdx.x >> 6][1] = sad_mc, red[threadIdx.x >> 6][2] = unwarped;
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

int ofx_motion_batch_launch(const ofx_motion_batch *a, void *stream)
{
    const char *who = "ofx_motion_batch_launch";
    OFX_REQUIRE(a, "%s: bad arguments", who);
    OFX_TRY(check_batch(who, a->n, a->w, a->h, 1, {a->prev_pitch, a->next_pitch}, {a->flow}, a->stats));
    for (int i = 0; i < a->n; ++i) {
        OFX_REQUIRE(a->prev[i] && a->next[i], "%s: pair %d: null pointer", who, i);
        OFX_REQUIRE(a->dst[i] || a->stats[i], "%s: pair %d has neither an image nor a stats slot", who, i);
        OFX_REQUIRE(((uintptr_t)a->uv[i] & 3) == 0, "%s: pair %d: the shift vector must be 4-byte aligned", who, i);
        OFX_REQUIRE(!a->dst[i] || a->dst_pitch >= a->w, "%s: the image's row pitch %d is below the width %d", who, a->dst_pitch, a->w);
        OFX_REQUIRE(!a->dst_dwords || !a->dst[i] || (((uintptr_t)a->dst[i] | (uintptr_t)a->dst_pitch) & 3) == 0,
                    "%s: pair %d: dword stores need a 4-byte aligned image and pitch", who, i);
    }
    OFX_TRY(zero_stats(a->stats, a->n, 4, stream)); // (everything is checked)
    hipLaunchKernelGGL(motion_ring_kernel, grid(a->w, a->h, a->n), dim3(kThreads), 0, ofx_stream(stream), *a);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

extern "C" int ofx_motion_compensate(const uint8_t *d_prev, int prev_pitch, const uint8_t *d_next, int next_pitch, int w, int h,
                                     const float *d_flow, const float *d_uv, float scale, uint8_t *d_dst, int dst_pitch, int64_t *d_stats,
                                     void *stream)
{
    static thread_local ofx_motion_batch mb; // (1 KB)
    memset(&mb, 0, sizeof mb);
    mb.n = 1, mb.w = w, mb.h = h, mb.scale = scale;
    mb.prev[0] = d_prev, mb.prev_pitch[0] = prev_pitch;
    mb.next[0] = d_next, mb.next_pitch[0] = next_pitch;
    mb.flow[0] = d_flow, mb.uv[0] = d_uv;
    mb.dst[0] = d_dst, mb.dst_pitch = d_dst ? dst_pitch : 0;
    mb.dst_dwords = d_dst && (((uintptr_t)d_dst | (uintptr_t)dst_pitch) & 3) == 0;
    mb.stats[0] = reinterpret_cast<unsigned long long *>(d_stats);
    return ofx_motion_batch_launch(&mb, stream); // (checks every argument before it enqueues anything)
}
