// The bilinear warp of lk_iter in the form the accumulating march uses (lk_body_buf.h, ITER >= 2): one
// lane's 4 adjacent pixels of one row, in two stages with the loads of the taps in flight between them.  Included by lk_body.h.
//
// A refinement iteration used to be two launches: warp_u8_kernel (flow -> warped image: a flow load, then the tap loads that
// depend on it, per short wave -- latency-bound at 0.37 of the HBM roofline) and the accumulating level kernel.  The march of
// iteration j now also writes the warped image iteration j + 1 reads: the flow of an output row is in registers right after
// its solve, so the row's warp needs no flow load at all, and its tap loads have a whole step of the march to arrive.  Only the
// first refinement iteration of a pair still needs warp_u8_kernel.
//
// Per pixel the four taps are two (generally unaligned) dwords, one from each of the rows yi and y1, fetched AT byte xi of the row
// through a buffer resource, so that no coordinate, however wild, reads outside the level: eight loads per lane, no selector, no
// permute, no branch.  Byte 0 of such a dword is p(xi) and byte 1 is p(xi + 1) whenever p(xi + 1) is looked at:
// (a) the right tap is only replaced by the pixel itself (replicate border) for xi = w - 1, and there the source column was clamped
// to w - 1, its fraction is 0 and p + 0 * (q - p) is p for every byte q -- whatever byte 1 holds;
// (b) a dword that starts in the last three bytes of the row pitch runs into the next row, but its bytes 0 and 1 are still this
// row's (xi <= w - 1 < pitch, and xi + 1 <= w - 1 when it counts).
// What is left is the dword that starts in the last three bytes of the LAST row of the plane: the resource is declared three bytes
// longer than the rows (lk_body_buf.h), which is why d_warp_src must be followed by three readable bytes (include/ofx.h; every
// plane of a session is followed by 64).
// The arithmetic per pixel is the oracle's (orc_warp_bilinear_u8), in the operation order of warp4_general (stages_body.h):
// the bytes are those of warp_u8_kernel (the iteration tests compare against the warp launch and the oracle).  A pixel whose flow
// is not finite is not warped (stages_body.h): here, a pixel with zero flow -- both fractions are 0 then, and p + 0 * (q - p) is p
// for all bytes p, q.  (The forms with per-pixel selectors and with a branch for the common row: profiles/r04_ablation.txt, batch 4.)
#pragma once

namespace ofx_dev {

struct WarpRowState {      // a row of a lane between the two stages
    float fx[4], fy[4];    // the fractions of the source coordinates
    // Two leftovers of the removed forms, which nothing reads: sel[] is never written either, general is.  Without either of them
    // hipcc allocates the registers of the kernels that warp differently, so they stay until those kernels are measured anyway
    // (DESIGN.md section 9).
    uint32_t sel[4];
    uint32_t ra[4], rb[4]; // per pixel the dwords of rows yi and y1 (loads in flight between the stages)
    int general;
};

__device__ __forceinline__ void warp_row_clear(WarpRowState &M)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) M.fx[k] = M.fy[k] = 0.0f, M.ra[k] = M.rb[k] = 0u;
    M.general = 1;
}

// Stage 1: source coordinates; issues the eight tap loads through `rs` (the rows [row0, row_end) of the warp source,
// `pitch` bytes apart, pitch >= 4: the whole level, or -- ROWWIN -- the row window a shard holds).
// ROWWIN: a tap row outside the window is replaced by the window's nearest row, and `miss` gets bit k set for a wanted pixel k
// (k < npx) with a finite flow whose taps needed such a row: the caller reports it (ofx_session_corner_status, bits 16 + level).
template <bool ROWWIN>
__device__ __forceinline__ void warp_row_prepare(const __amdgpu_buffer_rsrc_t &rs, float scale, int w, int h, int pitch, int row0, int row_end, int x0,
                                                 int y, int npx, const float (&fu)[4], const float (&fv)[4], WarpRowState &M, uint32_t &miss)
{
    const float xf0 = (float)x0, yf = (float)y, wmaxf = (float)(w - 1), hmaxf = (float)(h - 1);
    const int hmax = h - 1;
    int xi[4], ya[4], yb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xr = xf0 + (float)k;
        const float sxr = xr + scale * fu[k], syr = yf + scale * fv[k];
        const bool ok = __builtin_fabsf(sxr) <= 1e9f && __builtin_fabsf(syr) <= 1e9f; // (NaN fails)
        const float sx = __builtin_amdgcn_fmed3f(ok ? sxr : xr, 0.0f, wmaxf);
        const float sy = __builtin_amdgcn_fmed3f(ok ? syr : yf, 0.0f, hmaxf);
        xi[k] = (int)sx;
        const int yi = (int)sy;
        M.fx[k] = __builtin_amdgcn_fractf(sx); // == sx - (float)xi: sx >= 0, the difference is exact
        M.fy[k] = __builtin_amdgcn_fractf(sy);
        ya[k] = yi, yb[k] = min(yi + 1, hmax);
        if constexpr (ROWWIN) {
            if (k < npx && ok && (ya[k] < row0 || yb[k] >= row_end)) miss |= 1u << k;
            ya[k] = min(max(ya[k], row0), row_end - 1) - row0;
            yb[k] = min(max(yb[k], row0), row_end - 1) - row0;
        }
    }
    M.general = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        M.ra[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, (uint32_t)(ya[k] * pitch + xi[k]), 0, 0);
        M.rb[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, (uint32_t)(yb[k] * pitch + xi[k]), 0, 0);
    }
}

// Stage 2: the taps have arrived; the row's four bytes.
__device__ __forceinline__ uint32_t warp_row_finish(const WarpRowState &M)
{
    uint32_t out = 0;
    auto blend = [&](int k, uint32_t pa, uint32_t pb) {
        const float p00 = (float)(pa & 0xffu), p01 = (float)((pa >> 8) & 0xffu); // (v_cvt_f32_ubyte0 / 1)
        const float p10 = (float)(pb & 0xffu), p11 = (float)((pb >> 8) & 0xffu);
        const float a = p00 + M.fx[k] * (p01 - p00);
        const float b = p10 + M.fx[k] * (p11 - p10);
        const float v = a + M.fy[k] * (b - a);
        out |= ((uint32_t)(int)(v + 0.5f) & 0xffu) << (8 * k);
    };
#pragma unroll
    for (int k = 0; k < 4; ++k) blend(k, M.ra[k], M.rb[k]);
    return out;
}

} // namespace ofx_dev
