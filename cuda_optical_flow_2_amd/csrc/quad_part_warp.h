// A TEXTUAL part of the quad march (quad_stage.h): #include it at the place of use, inside the loop over a thread's quads.  It is
// text and not a function because behind any function boundary the compiler schedules the kernels around it otherwise
// (profiles/refactor_quad_parts.txt); so it has no include guard, and its locals are the enclosing block's.
//
// The fused warp of a quad by the four vectors the thread holds (prolong_kernel, median_march): motion_ring.hip's arithmetic
// without the shift, in warp_row_prepare's operation order.  Pixel k samples (x0 + k + scale * fu[k], y + scale * fv[k]); a position
// that is not finite or beyond 1e9 is not warped: the pixel has its own position and zero fractions, its own byte.  The position
// is clamped to the plane BEFORE it becomes an offset, and the taps go through rs_s, a buffer resource of exactly the plane's
// (h - 1) * pitch + w bytes: no vector, however wild, reads outside the plane.  The two taps of a tap row are one 16-bit load
// where the lane has proved xi < w - 1 for its live pixels (`wide`), else two byte loads with the right one AT column x1 -- in the
// last column that is the left tap again, because the byte behind it is the row's padding, the next row, or nothing (the
// lk_body_warp.h / motion_ring.hip / interp.hip rule).  A pixel past the row's ragged end gets kNowhere and loads zeros nobody
// looks at.  All taps are issued before the first is used; the blend and the rounding are quad_stage.h's.
//
// Reads   int x0, y, npx, sp (the plane's pitch), wmax, hmax; float fu[4], fv[4], scale, wmaxf, hmaxf; the resource rs_s
// Defines uint32_t out: byte k = the warped pixel k, for store_quad_u8  (and the locals xf0, yf, fx, fy, o0, o1, dx, wide, r0, r1)
const float xf0 = (float)x0, yf = (float)y;
float fx[4], fy[4];
uint32_t o0[4], o1[4], dx[4];
bool wide = true;
#pragma unroll
for (int k = 0; k < 4; ++k) {
    const float xr = xf0 + (float)k;
    const float sxr = xr + scale * fu[k], syr = yf + scale * fv[k];
    const bool ok = __builtin_fabsf(sxr) <= 1e9f && __builtin_fabsf(syr) <= 1e9f; // (a NaN fails: not warped)
    const float sx = __builtin_amdgcn_fmed3f(ok ? sxr : xr, 0.0f, wmaxf);
    const float sy = __builtin_amdgcn_fmed3f(ok ? syr : yf, 0.0f, hmaxf);
    const int xi = (int)sx, yi = (int)sy;
    fx[k] = __builtin_amdgcn_fractf(sx); // == sx - (float)xi: sx >= 0, the difference is exact
    fy[k] = __builtin_amdgcn_fractf(sy);
    const int y1 = min(yi + 1, hmax);
    const bool live = k < npx; // (a pixel past the row's end has its clamped column: its taps read as 0, nobody looks)
    const uint32_t a0 = (uint32_t)yi * (uint32_t)sp + (uint32_t)xi, a1 = (uint32_t)y1 * (uint32_t)sp + (uint32_t)xi;
    o0[k] = live ? a0 : kNowhere, o1[k] = live ? a1 : kNowhere;
    dx[k] = xi < wmax ? 1u : 0u;
    wide = wide && (!live || dx[k]);
}
uint32_t r0[4], r1[4]; // per pixel (left, right) of the two tap rows in bytes 0 and 1
if (wide) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r0[k] = __builtin_amdgcn_raw_buffer_load_b16(rs_s, o0[k], 0, 0);
        r1[k] = __builtin_amdgcn_raw_buffer_load_b16(rs_s, o1[k], 0, 0);
    }
} else {
    uint32_t l[2][4], r[2][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        l[0][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_s, o0[k], 0, 0);
        r[0][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_s, o0[k] + dx[k], 0, 0);
        l[1][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_s, o1[k], 0, 0);
        r[1][k] = __builtin_amdgcn_raw_buffer_load_b8(rs_s, o1[k] + dx[k], 0, 0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) r0[k] = l[0][k] | (r[0][k] << 8), r1[k] = l[1][k] | (r[1][k] << 8);
}
uint32_t out = 0;
#pragma unroll
for (int k = 0; k < 4; ++k) out |= round_u8(blend_u8(r0[k], r1[k], fx[k], fy[k])) << (8 * k);
