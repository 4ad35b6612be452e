// A TEXTUAL part of the frame interpolation kernels (interp_kernel, interp3_kernel): #include it as the first thing in the kernel.
// It is text and not a function or template because behind either the compiler schedules the kernels otherwise
// (profiles/refactor_quad_parts.txt); so it has no include guard, and what it declares are the kernel's locals.
//
// The planes hold kBpp bytes per pixel, channels interleaved: a row is kBpp * w bytes, a pixel's tap is at y * pitch + kBpp * x.
// Each plane goes through a buffer resource of exactly its (h - 1) * pitch + kBpp * w bytes and each field through one of its
// w * h * 8 bytes.  A sampling position is clamped to the plane, or is the pixel's own where it is not finite or beyond 1e9,
// BEFORE it becomes an offset, and a pixel past the row's ragged end gets kNowhere: no field value, however wild, reads outside a
// plane.  The right tap is the next pixel (dx = 1) only where xi < w - 1: in the last column it is the left pixel again, and no
// load may begin in a row's last pixel and end behind it (the lk_body_warp.h / motion_ring.hip rule).
//
// Reads   the kernel's argument A (an ofx_interp_batch) and the file's constant kBpp, the planes' bytes per pixel
// Defines the LDS counters cnt and wave sums red (for interp_part_reduce.h); b, w, h, wmax, hmax, nt, ap, bp, wmaxf, hmaxf, qrow,
//         n_quads, dst, stats; the resources rs_a, rs_b (planes), rs_ab, rs_ba (fields); the lambdas load_fields and side
__shared__ uint32_t cnt[OFX_INTERP_MAX_TIMES][kThreads];
__shared__ uint32_t red[kThreads / 64][OFX_INTERP_MAX_TIMES][3];
const int b = blockIdx.y;
const int w = A.w, h = A.h, wmax = w - 1, hmax = h - 1, nt = A.n_times;
const int ap = A.a_pitch[b], bp = A.b_pitch[b];
const __amdgpu_buffer_rsrc_t rs_a = rsrc(A.a[b], hmax * ap + kBpp * w), rs_b = rsrc(A.b[b], hmax * bp + kBpp * w);
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
// steps 3 to 5 of one side of one pixel, up to the taps: the byte offsets of the left taps of its two tap rows, whether the right
// taps are the next pixel (xi < w - 1) or the same one, and the fractions.  Returns "usable".
auto side = [&](float px, float py, float xf, float yf, int pitch, bool live, uint32_t &o0, uint32_t &o1, uint32_t &dx, float &fx,
                float &fy) -> bool {
    const bool fin = __builtin_fabsf(px) <= 1e9f && __builtin_fabsf(py) <= 1e9f; // (a NaN fails)
    const bool usable = fin && px >= 0.0f && px <= wmaxf && py >= 0.0f && py <= hmaxf;
    const float sx = fin ? __builtin_amdgcn_fmed3f(px, 0.0f, wmaxf) : xf;
    const float sy = fin ? __builtin_amdgcn_fmed3f(py, 0.0f, hmaxf) : yf;
    const int xi = (int)sx, yi = (int)sy;
    fx = sx - (float)xi, fy = sy - (float)yi;
    const int y1 = min(yi + 1, hmax);
    o0 = live ? (uint32_t)(yi * pitch + kBpp * xi) : kNowhere, o1 = live ? (uint32_t)(y1 * pitch + kBpp * xi) : kNowhere;
    dx = xi < wmax ? 1u : 0u;
    return usable;
};
