/*
 * ofx.h -- C ABI of the MI355X dense pyramidal Lucas-Kanade engine (libofx_hip.so).
 *
 * This is the drop-in boundary for the reference's hot path: plain pointers and
 * sizes, no C++ or torch types.  The reference exposes the same path as C++
 * free functions (OptFlowGpu.cuh:5-35); include/OptFlowGpu.cuh in this repo
 * re-declares that surface and implements it on top of the entry points below
 * (INTEGRATION.md shows the binding).  Every entry point names the reference
 * interface it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, an OFX_E_* code otherwise, and never
 *     throws; ofx_last_error() returns the message of the calling thread's last
 *     failure (the reference returns void and checks nothing).
 *   - "d_" pointers are DEVICE pointers, "h_" pointers are HOST pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Device
 *     entry points only enqueue work; they never synchronise or allocate.
 *   - a device entry point (every stateless call: what takes `stream` and no
 *     session) may be called while its stream is capturing (hipStreamBeginCapture,
 *     any mode).  It then records only kernel nodes on that stream -- the zeroing
 *     of its stats, d_outside, d_counts and tracker counters is a launch of the
 *     library's own, no memset node -- and nothing runs until the graph is
 *     launched.  Host arrays (descriptors, tables, models, parameters, times) are
 *     fixed at capture: they are read before the call returns, as ever; device
 *     buffers are read at every replay, so a replay on other frames, fields,
 *     points or matches at the same addresses is the call on those.  `stream`
 *     must not be NULL when capturing.  A call that is refused (OFX_E_INVALID)
 *     records nothing and leaves the capture open.  What returns data to the
 *     host synchronises and cannot be captured: ofx_session_get_flow_host, the
 *     status reads (ofx_session_corner_status, ofx_session_pair_status) and
 *     ofx_session_timing_read / _read_kind.  The session's own calls: see
 *     "capturing a session's pair" at ofx_session_run_flow.
 *   - "3ch" images are HWC interleaved u8, 3 bytes per pixel, tightly packed
 *     (the reference's layout, main.cu:95-104).  "1ch" planes are u8 with a row
 *     pitch in bytes that is a multiple of 4 and >= w.  A plane pointer is 4-byte
 *     aligned (the kernels load and store dwords); otherwise OFX_E_INVALID.  Pad
 *     bytes (columns [w, pitch) of a row) of an input may hold anything.
 *   - flow is interleaved (u,v) float32, 2*w floats per row, tightly packed
 *     (OptFlowGpu.cu:1844-1845).  A flow pointer handed to ofx_lk_level(s) or
 *     ofx_warp_levels is 8-byte aligned (a (u,v) pair is loaded and stored as one
 *     piece, rows as 16-byte pieces at 8-byte aligned addresses); otherwise
 *     OFX_E_INVALID.  Nothing more is needed: not 16 bytes, not a padded row.
 *   - window sizes are the reference's ww/wh (full size, not radius).
 */
#ifndef OFX_H
#define OFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFX_OK 0
#define OFX_E_INVALID 1     /* bad argument (size, alignment, unsupported window ...) */
#define OFX_E_HIP 2         /* a HIP runtime call failed; message holds hipGetErrorString */
#define OFX_E_UNSUPPORTED 3 /* valid request this build does not implement */
#define OFX_E_STATE 4       /* session used out of order */

/* which reference semantics a flow level follows */
#define OFX_MODE_COMPAT_CPU 0 /* cpu::calc_optical_flow, OptFlowCPU.cpp:312-399: wrapped-u8 derivatives,
                                 Gaussian It, inline solve (c unscaled) */
#define OFX_MODE_LK_FLOAT 1   /* gpu::calc_opt_flow, OptFlowGpu.cu:1909-1979: float derivatives, Dt_3x3,
                                 double solve */

#define OFX_MODE_LK_FLOAT_FAST 2 /* lk_float with the solve in its <= 1 ulp(float) formulation (SURVEY 8c's tolerance for the
                                    solve; identical NaN / Inf positions) instead of the replay of the reference's
                                    operation order: numerators first, reciprocal to 2^-44 -- 11 double operations per
                                    pixel instead of 19.  Everything else (window sums, shift, pyramid) is bit-exact. */

#define OFX_MAX_LEVELS 12
#ifndef OFX_MAX_LK_ITEMS /* (build experiments only: the shipped library and this header must agree) */
#define OFX_MAX_LK_ITEMS 80
#endif /* (level, pair) items one fused LK launch can carry (ofx_lk_levels, ofx_stream_launch) */

const char *ofx_last_error(void);
/* library/ABI version, bumped when a signature changes */
int ofx_abi_version(void);
/* number of visible HIP devices, or a negative OFX_E code */
int ofx_device_count(void);

/* ------------------------------------------------------------------------
 * Geometry of one pyramid level as seen by one rank.  Unsharded use:
 * row0 = 0, rows = h, out_y0 = 0, out_y1 = h.  Row-sharded use:
 * the plane buffers hold global rows [row0, row0+rows) -- the rank's block plus
 * halo -- and the kernels produce global rows [out_y0, out_y1).  Rows outside
 * [0,h) are the image border (taps skipped, as the reference does); rows inside
 * [0,h) that a stencil needs must be present in the buffer or the call fails
 * with OFX_E_INVALID.
 * ---------------------------------------------------------------------- */
typedef struct ofx_geom {
    int w, h;   /* global width / height of this level */
    int pitch;  /* bytes per row of the 1ch planes (multiple of 4, >= w) */
    int row0;   /* global row index held in buffer row 0 */
    int rows;   /* rows present in the buffers */
    int out_y0; /* first global row to produce */
    int out_y1; /* one past the last global row to produce */
} ofx_geom;

/* ---- hot path, device-resident ------------------------------------------ */

/* One level of dense LK, fully fused: 3x3 derivative stencils, the five
 * windowed sums of products and the 2x2 solve in one kernel.
 * Replaces the device work of gpu::calc_opt_flow (OptFlowGpu.cu:1930-1964) /
 * cpu::calc_optical_flow steps 1-3 (OptFlowCPU.cpp:329-384) for one level.
 * d_next must already be shifted (ofx_shift_1ch) when level != top (or use ofx_lk_levels with d_uv).
 * d_flow receives rows [out_y0,out_y1) at row offset (y - flow_row0).
 * window: odd, 3..23 (lk_float) / 3..25 (compat_cpu). */
int ofx_lk_level(const uint8_t *d_prev, const uint8_t *d_next, const ofx_geom *g, int window, int mode,
                 float *d_flow, int flow_row0, void *stream);

/* Several levels in ONE launch (the levels of a pyramid are independent once the shift vectors are known -- see
 * ofx_corner_flows).  Descriptors are processed in the order given; coarse levels first is the useful order. */
typedef struct ofx_lk_desc {
    const uint8_t *d_prev;
    const uint8_t *d_next;
    ofx_geom geom;
    float *d_flow;
    int flow_row0;
    /* NULL: d_next is used as it is (top level, or already shifted with ofx_shift_1ch).  Non-NULL: 2 floats on the
     * device; the kernel reads d_next THROUGH the reference's global shift by that vector (cpu::shift_back_pyramid,
     * OptFlowCPU.cpp:241-282, fused into the row loads) -- same bits as shifting first, without the extra pass. */
    const float *d_uv;
    int accumulate; /* non-zero: d_flow += result (refinement iterations, ofx_warp_levels) instead of d_flow = result */
    /* Extension (the reference divides unguarded, OptFlowGpu.cu:1833-1838 / OptFlowCPU.cpp:369-372, and writes
     * NaN / Inf / huge vectors where a window has no texture or a single edge): > 0 = a pixel whose determinant Sxx*Syy - Sxy^2,
     * rounded to float, is below min_det gets the flow (0, 0).  0 = the reference.  One value per launch: the first
     * descriptor's -- levels[0].min_det, also when levels[0] is empty (out_y1 == out_y0) and launches nothing itself. */
    float min_det;
    /* Extension (lk_iter; csrc/lk_body_warp.h).  d_warp_out non-NULL, with accumulate set: the launch also writes the warped image
     * the NEXT refinement iteration reads as its d_next -- d_warp_out = ofx_warp_levels(d_warp_src, the flow this launch leaves in
     * d_flow, warp_scale), same bytes -- so that only a pair's first refinement iteration needs ofx_warp_levels.  d_warp_src is the
     * warp source (the globally shifted next image), d_warp_out a plane of the level's geometry other than d_next and d_warp_src.
     * d_warp_src MUST BE FOLLOWED BY THREE READABLE BYTES (ABI v10: the launch fetches a tap's dword at the tap's own byte, also in
     * the last three columns of the plane's last row; the bytes beyond the plane are never looked at.  Every plane of an ofx_session
     * is followed by 64.)
     * For all descriptors of a launch or for none.  On a row window (a shard: geom.row0 / rows / out rows are not the whole level)
     * d_warp_out receives the out rows, a tap row outside [row0, row0 + rows) is replaced by the nearest row held, and bit
     * warp_status_bit of *d_warp_status (optional) is set when a pixel with a finite flow needed such a row.
     * Pad bytes of d_warp_out: an out row is stored as whole dwords, so its columns [w, (w + 3) & ~3) are written with unspecified
     * values; the columns from (w + 3) & ~3 on, and every row that is not an out row, are left untouched. */
    const uint8_t *d_warp_src;
    uint8_t *d_warp_out;
    float warp_scale;
    int *d_warp_status;
    int warp_status_bit;
} ofx_lk_desc;
int ofx_lk_levels(const ofx_lk_desc *levels, int n, int window, int mode, void *stream);

/* descriptor of one level's shift (ofx_shift_levels, ofx_stream_launch) */
typedef struct ofx_shift_desc {
    const uint8_t *d_src;
    uint8_t *d_dst;
    ofx_geom geom;
    const float *d_uv;
} ofx_shift_desc;

/* One tick of the frame-stream pipeline in ONE launch: the pyramids of the newest frame(s) | the corner flows of earlier
 * pair(s) | the fused LK of still earlier pair(s), as disjoint block ranges of one grid.  Every stage only reads what
 * earlier launches wrote, so the stages need no synchronisation; a stage is skipped when its count is 0.  A tick may
 * carry up to OFX_STREAM_MAX_BATCH frames / pairs per stage (ofx_params.stream_batch): the LK items of B pairs then
 * share one launch, which multiplies the strip height by B (1/B of the priming rows per output row) and divides the
 * number of launches by B.
 * ofx_session_stream_submit drives this; it is exposed for callers that manage their own buffers. */
#ifndef OFX_STREAM_MAX_BATCH
#define OFX_STREAM_MAX_BATCH 16
#endif
typedef struct ofx_pyramid_stage {
    /* levels 1..levels-1 from d_frame, plus a copy of level 0 into d_levels[0] */
    const uint8_t *d_frame;
    int frame_pitch, w, h, levels;
    uint8_t *d_levels[OFX_MAX_LEVELS];
    int pitches[OFX_MAX_LEVELS];
    /* row windows of the destination planes (row-sharded callers): with windowed != 0, d_levels[k] holds the global rows
     * [row0[k], row0[k] + rows[k]) of level k and only those are written; d_frame is always the whole frame. */
    int windowed;
    int row0[OFX_MAX_LEVELS], rows[OFX_MAX_LEVELS];
    /* a second, small pyramid of the same frame's top-left patch_w x patch_h corner (patch_levels = 0: none).  A
     * pyramid of such a patch equals the top-left part of the frame's pyramid at every level (the stencil 2x-1..2x+1
     * never reaches past column/row 2*w_k-1), which lets a rank that does not hold row 0 compute the corner flows. */
    int patch_w, patch_h, patch_levels;
    uint8_t *d_patch_levels[OFX_MAX_LEVELS];
    int patch_pitches[OFX_MAX_LEVELS];
} ofx_pyramid_stage;
typedef struct ofx_corner_stage {
    /* descriptors as for ofx_corner_flows.  cols[k] > 0: the planes of level k are a patch holding columns [0, cols[k])
     * and rows [0, geom.rows) of the geom.w x geom.h level; d_status (may be NULL): bit k is OR-ed in when level k needed
     * a pixel inside the image but outside its planes (the shift left the patch: that pair's result is not the
     * reference's).  shard_rows[k] = {need0, need1, valid0, valid1} (all zero: unchecked), for a row-sharded caller: the
     * image rows [need0, need1) of level k that the LK stencils of this shard touch and the rows [valid0, valid1) its
     * buffers hold; bit 8 + k is OR-ed in when level k's vertical shift sends those reads to rows that exist in the image
     * but not in the shard (the rows of that pair next to the shard's edge are then not the reference's). */
    ofx_lk_desc level[OFX_MAX_LEVELS];
    int levels;
    float *d_uv;
    int cols[OFX_MAX_LEVELS];
    int *d_status;
    int shard_rows[OFX_MAX_LEVELS][4];
    /* build_patch != 0: the stage first builds the patch pyramids it reads -- levels 1 .. levels-1 of the top-left
     * patch_w x patch_h corner of BOTH frames, from d_patch_src[0] (the pair's previous frame) and d_patch_src[1] (its next
     * frame) into d_patch[0][k] / d_patch[1][k] (pitch patch_pitch[k]) -- and then walks the chain.  level[k] must
     * describe exactly those planes for k >= 1 and the frames themselves for k = 0.  With it a pair's shift vectors need
     * nothing but the two frames, i.e. they can be formed in the tick in which the pair's second frame arrives
     * (ofx_params.stream_two_stage). */
    int build_patch, patch_w, patch_h;
    const uint8_t *d_patch_src[2];
    int patch_src_pitch[2];
    uint8_t *d_patch[2][OFX_MAX_LEVELS];
    int patch_pitch[OFX_MAX_LEVELS];
    /* REPAIR of a shift that leaves the patch (cpu::shift_back_pyramid defines the shift for every input,
     * OptFlowCPU.cpp:255-273: a flat or nearly singular corner sends the next level's shifted corner anywhere in the image).
     * d_patch_reloc[1 .. levels-1] != NULL: a third set of patch planes (same sizes and pitches as d_patch[f]); when level k
     * needs a pixel of the next frame's pyramid that the top-left patch does not hold, the stage's block rebuilds that small
     * pyramid AROUND the shifted corner from the whole next frame and runs the level again on it -- no status bit, no host
     * round trip, the reference's result.  Needs level[0] to describe the WHOLE frames (geom.rows = h, cols[0] = 0 or w) and
     * patch_w / patch_h / patch_pitch to be set (with or without build_patch).  NULL: bit k of the status words is raised
     * instead, as before.
     * d_pair_status (may be NULL): THIS pair's status word is WRITTEN there when the chain ends: the bits raised in
     * *d_status by this pair, plus OFX_STATUS_REPAIRED when a relocated patch was used (the pair is exact all the same). */
    uint8_t *d_patch_reloc[OFX_MAX_LEVELS];
    int *d_pair_status;
} ofx_corner_stage;
#define OFX_STATUS_REPAIRED (1 << 24)
typedef struct ofx_stream_stages {
    ofx_pyramid_stage pyr[OFX_STREAM_MAX_BATCH];
    int n_pyr;
    ofx_corner_stage corner[OFX_STREAM_MAX_BATCH];
    int n_corner;
    ofx_lk_desc lk[OFX_MAX_LK_ITEMS]; /* the LK items of every pair of the tick (levels x pairs <= OFX_MAX_LK_ITEMS) */
    int n_lk;
    int deep_fetch; /* 0 = by size, +1 / -1 = deep / one-step row fetch of the LK stage (see ofx_params.deep_fetch; OFX_LK_DMA overrides) */
} ofx_stream_stages;
int ofx_stream_launch(const ofx_stream_stages *stages, int window, int mode, void *stream);
/* Measurement hook: with a device buffer of 8 * capacity_blocks uint64 set, every wave of every later ofx_stream_launch
 * records its start and end time (100 MHz wall clock) at [2 * (4 * block + wave)]; first (2 * OFX_STREAM_MAX_BATCH + 1 ints, may be NULL) receives
 * the block ranges of the last launch (corner blocks first, then LK up to first[0], then the pyramid stages).
 * d_buf = NULL switches it off.  Process-global, not thread-safe. */
int ofx_debug_stream_trace(unsigned long long *d_buf, int capacity_blocks, int *first);

/* Same level, but stopping before the solve: writes the five window sums
 * (Sxx, Syy, Sxy, Sxt, Syt) as int32 planes of w ints per row.  Test/inspection
 * entry point; equals five gpu::srm_1ch(_float) calls (OptFlowGpu.cu:1944-1960). */
int ofx_lk_level_sums(const uint8_t *d_prev, const uint8_t *d_next, const ofx_geom *g, int window, int mode,
                      int32_t *d_sums5, int flow_row0, void *stream);

/* 2x decimating 3x3 Gaussian on a 1ch plane: dst(x,y) = trunc(sum G[p][q] *
 * src(2x-1+q, 2y-1+p)), taps outside the source skipped.  Replaces one level
 * of gpu::gauss_pyramid (OptFlowGpu.cu:1198-1232) / cpu::downscale_gaussian
 * (OptFlowCPU.cpp:112-148) for grey images.  `dst` describes the destination
 * level; the source level is (2*dst->w) x (2*dst->h) and src_row0/src_rows say
 * which of its rows d_src holds.  Pad bytes of d_dst: the columns [w, (w + 3) & ~3)
 * of the out rows are written as 0, everything else is left untouched. */
int ofx_downsample_1ch(const uint8_t *d_src, int src_pitch, int src_row0, int src_rows,
                       uint8_t *d_dst, const ofx_geom *dst, void *stream);

/* All levels of a grey pyramid from level 0 in ONE launch (same arithmetic as ofx_downsample_1ch level by level;
 * whole, unsharded levels only).  d_levels[k] / pitches[k] for k = 1..levels-1 (index 0 unused).  Only the pixels are
 * stored: the pad bytes of the planes (columns >= w >> k) are left untouched. */
int ofx_pyramid_1ch(const uint8_t *d_level0, int pitch0, int w, int h, uint8_t *const *d_levels, const int *pitches,
                    int levels, void *stream);

/* Translation the reference applies to `next` below the top level:
 * (u,v) = sum_{k=top..level+1} 2^(k-level) * flow_k[pixel 0]  in float, coarsest
 * first (OptFlowCPU.cpp:255-266, where `i * (1 >> offset)` is always 0).
 * d_flow_levels[k] = device pointer to level k's flow (only k > level are read).
 * Writes 2 floats to d_uv. */
int ofx_shift_vector(const float *const *d_flow_levels, int level, int max_level, float *d_uv, void *stream);

/* The shift of level k only needs PIXEL 0 of every coarser flow level (OptFlowCPU.cpp:260-262), and pixel 0's flow
 * only needs the (radius+2)^2 top-left corner of its level.  This entry point walks the pyramid coarse to fine in
 * one tiny launch: for each level it forms the shift vector from the corner flows found so far, evaluates pixel 0's
 * window sums on the shifted corner, solves, and stores d_uv[2k..2k+1] (and flow level k's pixel 0 when the
 * descriptor's flow_row0 is 0).  After it every level's shift and LK launch is independent of the others.
 * Descriptors: index k = pyramid level k, d_next = the UNSHIFTED next plane, geom.row0 must be 0. */
int ofx_corner_flows(const ofx_lk_desc *levels, int n_levels, int window, int mode, float *d_uv, void *stream);

/* Several ofx_shift_1ch calls in one launch (ofx_shift_desc is declared above).  Pad bytes of d_dst: the out rows are
 * stored over their whole pitch, columns [w, pitch) as 0; rows that are not out rows are left untouched. */
int ofx_shift_levels(const ofx_shift_desc *levels, int n, void *stream);

/* dst(x,y) = src((int)(x+u), (int)(y+v)) when that lands inside the image,
 * else src(x,y) if 3*(y*w+x) < w*h else 0 -- cpu::shift_back_pyramid
 * (OptFlowCPU.cpp:241-282) on channel 0 with the destination zero-initialised.
 * (u,v) is read from d_uv on the device.  Source rows needed but absent from
 * the buffer make the affected pixels undefined; the caller sizes halos. */
int ofx_shift_1ch(const uint8_t *d_src, uint8_t *d_dst, const ofx_geom *g, const float *d_uv, void *stream);

/* Extension (the reference has no iterations): d_dst(x,y) = round_u8(bilinear(d_src, x + scale*u, y + scale*v))
 * with (u,v) = d_flow at (x,y), replicate border, non-finite flow = no warp.  The planes may hold a row window of the level
 * (geom.row0 / rows; rows [out_y0, out_y1) are produced): a source row the warp needs that lies inside the image but outside
 * the window is replaced by the nearest row held and, when d_status is not NULL, bit status_bit is OR-ed into *d_status (a
 * row-sharded caller's flow reached beyond its halo).  One refinement
 * iteration of a level = this warp of the (shifted) next image by the flow so far, then ofx_lk_levels with
 * accumulate = 1.  scale = OFX_ITER_SCALE turns the reference's flow units into pixels (Sobel gain 8 / Dt_3x3 gain 15).
 * Pad bytes of d_dst: the out rows are stored over their whole pitch, columns [w, pitch) as 0; rows that are not out rows
 * are left untouched.  No tap reads outside the rows * pitch bytes of d_src, whatever the flow holds. */
#define OFX_ITER_SCALE 0.533333361148834228515625f
typedef struct ofx_warp_desc {
    const uint8_t *d_src;
    uint8_t *d_dst;
    ofx_geom geom;
    const float *d_flow;
    int flow_row0;
    float scale;
    int *d_status;  /* may be NULL */
    int status_bit;
} ofx_warp_desc;
int ofx_warp_levels(const ofx_warp_desc *levels, int n, void *stream);

/* ---- motion compensation -------------------------------------------------
 * The next image of a pair pulled back onto the previous one by the pair's flow -- "the image the next refinement iteration
 * would have read" -- and four sums that say how good the flow was.  THE definition (everything else quotes it), for one
 * level of w x h pixels:
 *   inputs  prev, next: u8 planes, each with its own row pitch; flow: interleaved (u, v) float32, w x h, tightly packed;
 *           uv: two floats on the device, the level's global shift (NULL = (0, 0)); scale.
 *   sh    = what ofx_shift_1ch(next, ., uv) writes, its out-of-image rule included: next((int)(x+u), (int)(y+v)) when that
 *           lands inside the image, else next(x, y) if 3*(y*w+x) < w*h, else 0.  (uv = (0, 0) is the identity.)
 *   mc    = what ofx_warp_levels writes for {src = sh, flow, scale}: orc_warp_bilinear_u8's operation order, replicate
 *           border, and a pixel with |x + scale*u| > 1e9, |y + scale*v| > 1e9 or a NaN there is NOT WARPED: mc = sh.
 *   stats = four int64:  [0] w*h   [1] sum |prev - next| (the unshifted next: no motion model at all)
 *                        [2] sum |prev - mc|             [3] the number of pixels that were not warped.
 * mc equals that two-launch chain bit for bit, and the sums are integers: they depend on no order, tile or batch.
 * stats[2] is the photometric error the solve was minimising; stats[2] / stats[1] says what the flow bought, and a scene
 * cut or a failed pair shows as a ratio near (or above) 1.
 *
 * ofx_motion_compensate: one level, stateless, one launch with the shift fused (no shifted plane is written).  Pitches >= w;
 * d_flow and d_stats 8-byte aligned; otherwise OFX_E_INVALID.  d_dst (rows dst_pitch apart; bytes beyond column w - 1 are
 * left untouched) or d_stats (4 values, overwritten) may be NULL on its own.  No tap reads outside the h x pitch bytes of
 * d_prev / d_next, whatever the flow holds.  d_stats needs no initialisation (the call zeroes it on the stream first) and carries
 * nothing from one call to the next. */
int ofx_motion_compensate(const uint8_t *d_prev, int prev_pitch, const uint8_t *d_next, int next_pitch, int w, int h,
                          const float *d_flow, const float *d_uv /* NULL = no shift */, float scale,
                          uint8_t *d_dst /* may be NULL */, int dst_pitch, int64_t *d_stats /* may be NULL; 4 values, overwritten */,
                          void *stream);

/* main.cu:138-147: dense flow at `level` = sum_k 2^(k-level) flow_k(y>>s, x>>s). */
int ofx_compose_flow(const float *const *d_flow_levels, int w, int h, int levels, int level, float *d_dst,
                     void *stream);

/* The composed field sampled instead of composed everywhere.  C(y, x) below is ofx_compose_flow's value at pixel (y, x) of `level`
 * (w x h), bit for bit; w and h must be multiples of 2^(levels - 1 - level) (every level but the coarsest even), otherwise
 * OFX_E_INVALID.
 *
 * ofx_sample_arrows: the arrow field of main.cu:123-169.  offset = w / arrow_res (integer division; 0 is OFX_E_INVALID -- the
 * reference would loop forever); grid points i = 0, offset, .. < h and j = 0, offset, .. < w, ny = ceil(h / offset) by
 * nx = ceil(w / offset) of them.  At each: (u, v) = C(i, j), each clamped to [-offset, +offset] by float comparisons a NaN passes
 * unclamped; x1 = (int)(u + (float)j), y1 = (int)(v + (float)i), one float add each, truncated toward zero.  The arrow is not
 * drawn when x1 < 0 || y1 < 0 or a sum is NaN.  d_dst (16-byte aligned) receives [ny][nx] records of four int32
 * (x0 = j, y0 = i, x1, y1), x1 = y1 = -1 for an undrawn arrow, in pixels of `level`.
 *
 * ofx_advect_points: n_points float32 (x, y) in pixels of `level` (d_points, 8-byte aligned) with an int32 status each (0 = alive)
 * moved through one pair's flow.  A point with status != 0 is left alone; one outside [0, w) x [0, h) (NaN included) gets
 * status = pair and keeps its position; otherwise (u, v) = C((int)y, (int)x) and (x + u, y + v), one float add each, is stored --
 * unless a sum is not finite: status = pair, position kept.  pair >= 1. */
int ofx_sample_arrows(const float *const *d_flow_levels, int w, int h, int levels, int level, int arrow_res, int32_t *d_dst, void *stream);
int ofx_advect_points(const float *const *d_flow_levels, int w, int h, int levels, int level, int pair, float *d_points, int32_t *d_status,
                      int n_points, void *stream);

/* ---- forward-backward consistency -------------------------------------------
 * Which pixels of a dense field can be trusted: follow the forward vector into the next frame, read the backward field
 * there, and see whether the two cancel.  THE definition (everything else quotes it), for one pair at one level of w x h
 * pixels:
 *   inputs  fwd: the field of frame a -> frame b; bwd: the field of frame b -> frame a (the same clip through the same
 *           pipeline in reverse order).  Both interleaved (u, v) float32, w x h, tightly packed, 8-byte aligned -- in practice
 *           two ofx_compose_flow fields.  scale: field units -> pixels (OFX_ITER_SCALE for this library's flows, 1 for fields
 *           in pixels).  alpha >= 0, beta >= 0, both finite; beta is in squared FIELD units.
 * Every float32 operation is rounded once, nothing is fused, denormals are kept.  For pixel (x, y) with (u, v) = fwd(y, x):
 *   1. px = (float)x + scale*u, py = (float)y + scale*v: the product rounded, then the sum (ofx_warp_levels' order).
 *   2. unless |px| <= 1e9 && |py| <= 1e9 (a NaN fails): class 3, UNDEFINED.
 *   3. else if px < 0 || px > (float)(w-1) || py < 0 || py > (float)(h-1): class 2, LEAVES -- the vector points out of the
 *      frame.  Nothing is clamped and bwd is not read.
 *   4. else x0 = (int)px, y0 = (int)py, fx = px - (float)x0, fy = py - (float)y0, x1 = min(x0+1, w-1), y1 = min(y0+1, h-1).
 *   5. for each component c of bwd, with b00 = bwd(y0,x0), b01 = bwd(y0,x1), b10 = bwd(y1,x0), b11 = bwd(y1,x1):
 *        a = b00 + fx*(b01 - b00);  c' = b10 + fx*(b11 - b10);  r_c = a + fy*(c' - a)
 *      (the blend of orc_warp_bilinear_u8, on floats).  In the last column x1 == x0, so b01 IS b00 (and b11 is b10) whatever
 *      lies behind the pixel in memory; likewise in the last row.
 *   6. du = u + r_u, dv = v + r_v, e = du*du + dv*dv, m = (u*u + v*v) + (r_u*r_u + r_v*r_v), thr = alpha*m + beta.
 *   7. unless |e| <= FLT_MAX: class 3.  Else class 0, CONSISTENT, when e <= thr, else class 1, INCONSISTENT.
 *   outputs, each may be absent but not all of them:
 *     mask  = u8, rows mask_pitch >= w apart, the class; bytes beyond column w - 1 are left untouched.
 *     err   = float32, w per row, tightly packed: e for classes 0 and 1, +Inf (0x7f800000) for classes 2 and 3; never a NaN.
 *     stats = four int64:  [0] w*h   [1] pixels of class 1   [2] of class 2   [3] of class 3.
 * The counts are integers: they depend on no order, tile or batch.  The check is one-sided: the other direction (occlusion
 * as seen from frame b) is the same call with the fields swapped.  e is the squared round-trip error in field units; alpha
 * scales the tolerance with the squared magnitudes of the two vectors, beta is its floor (0.01 and 0.5 px^2 are the usual
 * choice: beta = 0.5 / scale^2).
 *
 * ofx_flow_consistency: one pair, one launch.  ofx_flow_consistency_batch: 1 <= n <= OFX_STREAM_MAX_BATCH pairs of one size in
 * ONE launch; an output array may be NULL (that output is then off for all pairs), the entries of a non-NULL array must be
 * non-NULL, at least one output array is required; the host arrays are read before the call returns.  w*h < 2^28; fwd and bwd
 * 8-byte, err 4-byte, stats 8-byte aligned; mask_pitch >= w; scale, alpha and beta as above; otherwise OFX_E_INVALID, before
 * anything is enqueued.  No tap reads outside the w*h*8 bytes of a field, whatever the fields hold.  A stats slot needs no
 * initialisation (the call zeroes it on the stream first) and carries nothing from one call to the next. */
#define OFX_FB_CONSISTENT 0
#define OFX_FB_INCONSISTENT 1
#define OFX_FB_LEAVES 2
#define OFX_FB_UNDEFINED 3
int ofx_flow_consistency(const float *d_fwd, const float *d_bwd, int w, int h, float scale, float alpha, float beta,
                         uint8_t *d_mask /* may be NULL */, int mask_pitch, float *d_err /* may be NULL */,
                         int64_t *d_stats /* may be NULL; 4 values, overwritten */, void *stream);
int ofx_flow_consistency_batch(const float *const *d_fwd, const float *const *d_bwd, int n, int w, int h, float scale,
                               float alpha, float beta, uint8_t *const *d_mask, int mask_pitch, float *const *d_err,
                               int64_t *const *d_stats, void *stream);

/* ---- pixel displacement ------------------------------------------------------
 * ofx_compose_flow above is the reference's DISPLAY quantity (main.cu:138-147: sum_k 2^k flow_k in raw Sobel / Dt units); it is
 * not what the pipeline applies to the next image, and scaled by OFX_ITER_SCALE it is not a displacement either.  What the
 * pipeline applies at a level is the level's global shift uv (integer steps, per pair) and then the level's own flow times
 * OFX_ITER_SCALE.  That sum, in pixels, is the "pixel displacement".  THE definition (everything else quotes it), for one level
 * of w x h pixels:
 *   inputs  flow: interleaved (u, v) float32, w x h, tightly packed; uv: two floats on the device, the level's shift (NULL =
 *           none, as at the coarsest level); scale.
 *   D(y,x) = (floorf(uv[0]) + scale*u, floorf(uv[1]) + scale*v): the product rounded, then the sum.  With uv == NULL the first
 *           term is 0.0f and the add is still performed.  Every float32 operation is rounded once, nothing is fused, denormals
 *           are kept.  Nothing is tested or clamped: a NaN or Inf in uv or flow goes through.
 * Why floor: ofx_shift_1ch reads next((int)(x + u)) at integer x; away from the borders that is a translation by floor(u), and
 * a translation commutes with the bilinear warp that follows.  So away from the image borders the motion-compensated image is
 * mc(x) = bilinear(next, x + D(x)).
 *
 * ofx_flow_displacement: one level, stateless, one launch.  d_flow and d_dst 8-byte aligned, w*h < 2^28, scale finite;
 * otherwise OFX_E_INVALID, before anything is enqueued. */
int ofx_flow_displacement(const float *d_flow, int w, int h, const float *d_uv /* NULL = none */, float scale,
                          float *d_dst, void *stream);

/* ---- frame interpolation -----------------------------------------------------
 * In-between frames of a pair from its two displacement fields.  THE definition (everything else quotes it), for one pair of
 * u8 planes a and b of w x h pixels, each with its own row pitch:
 *   inputs  Dab (a -> b) and Dba (b -> a): displacement fields IN PIXELS, both on the pixel grid, interleaved float32, w x h,
 *           tightly packed; a time t, float32, finite, 0 < t < 1.
 *   host    in float32: omt = 1.0f - t; c00 = -(omt*t); c01 = t*t; c10 = omt*omt.  (The usual gather approximation of the
 *           intermediate flows, F(t->a) = -(1-t)t Dab + t^2 Dba and F(t->b) = (1-t)^2 Dab - t(1-t) Dba: exact for a translation.)
 * Every float32 operation is rounded once, nothing is fused, denormals are kept.  For pixel (x, y):
 *   1. Ta = c00*Dab(y,x) + c01*Dba(y,x) and Tb = c10*Dab(y,x) + c00*Dba(y,x), per component: both products rounded, then the sum.
 *   2. pa = ((float)x + Ta.x, (float)y + Ta.y), one add each; pb the same from Tb.
 *   3. a side is FINITE when |p.x| <= 1e9 && |p.y| <= 1e9 (a NaN fails), and USABLE when it is finite and
 *      0 <= p.x <= (float)(w-1) && 0 <= p.y <= (float)(h-1).
 *   4. its sampling position (sx, sy): finite -- p with each coordinate clamped to [0, w-1] / [0, h-1] (replicate border); not
 *      finite -- ((float)x, (float)y).
 *   5. x0 = (int)sx, y0 = (int)sy, fx = sx - (float)x0, fy = sy - (float)y0, x1 = min(x0+1, w-1), y1 = min(y0+1, h-1), and
 *      ofx_warp_levels' blend on floats: r0 = p00 + fx*(p01 - p00); r1 = p10 + fx*(p11 - p10); V = r0 + fy*(r1 - r0).  V is NOT
 *      rounded here.  This gives A from plane a and B from plane b.
 *   6. class 0: both sides usable; 1: only a; 2: only b; 3: neither.  v = A + t*(B - A) for classes 0 and 3, A for class 1, B
 *      for class 2; out = (uint8_t)(int)(v + 0.5f).
 *   7. stats = four int64 per (pair, time):  [0] w*h   [1] pixels of class 1   [2] of class 2   [3] of class 3.  Integers: they
 *      depend on no order, tile or batch.
 * The rule is geometric on purpose: a pixel whose source in one frame lies outside that frame is taken from the other frame,
 * which is what happens at the borders of a pan.  No tap reads outside the (h-1)*pitch + w bytes of a plane or the w*h*8 bytes
 * of a field, whatever the fields hold.
 *
 * ofx_interpolate_frames: n_times in-between frames of one pair in ONE launch; frame k at d_dst + k*time_stride_bytes (rows
 * dst_pitch apart, bytes beyond column w-1 untouched), its stats at d_stats + 4*k (d_stats may be NULL).
 * ofx_interpolate_frames_batch: the same for 1 <= n <= OFX_STREAM_MAX_BATCH pairs of one size and one set of times, ONE launch.
 * Null inputs, w, h <= 0 or w*h >= 2^28, a pitch below w, fields or stats not 8-byte aligned, n_times outside
 * 1 .. OFX_INTERP_MAX_TIMES, a time that is not finite or not in (0, 1), time_stride_bytes < h*dst_pitch when n_times > 1, a
 * NULL entry in a non-NULL array, n outside 1 .. OFX_STREAM_MAX_BATCH: OFX_E_INVALID, before anything is enqueued.  The host
 * arrays are read before the call returns.  The stats slots need no initialisation (the call zeroes them on the stream first) and
 * carry nothing from one call to the next. */
#define OFX_INTERP_MAX_TIMES 8
int ofx_interpolate_frames(const uint8_t *d_a, int a_pitch, const uint8_t *d_b, int b_pitch, int w, int h,
                           const float *d_disp_ab, const float *d_disp_ba, const float *h_times, int n_times,
                           uint8_t *d_dst, int dst_pitch, size_t time_stride_bytes, int64_t *d_stats /* may be NULL */, void *stream);
int ofx_interpolate_frames_batch(const uint8_t *const *d_a, const int *a_pitches, const uint8_t *const *d_b,
                                 const int *b_pitches, int n, int w, int h, const float *const *d_disp_ab,
                                 const float *const *d_disp_ba, const float *h_times, int n_times,
                                 uint8_t *const *d_dst, int dst_pitch, size_t time_stride_bytes,
                                 int64_t *const *d_stats /* may be NULL */, void *stream);

/* ---- colour frame interpolation ------------------------------------------------
 * "frame interpolation" above, for interleaved 3-channel u8 planes a and b of w x h pixels, each with its own row pitch in bytes
 * >= 3*w; no alignment is required of a plane, its pitch or the destination, and the channel order does not matter.  Dab, Dba,
 * the times and the host step for c00 / c01 / c10 are exactly as there.  Steps 1 to 4 and the class are computed ONCE per pixel;
 * step 5's blend and step 6's value and rounding are applied to each channel with the same fx, fy and class.  Hence the byte at
 * channel c of a pixel is, bit for bit, what "frame interpolation" gives for the planes a[..., c] and b[..., c].  stats are its
 * four words per (pair, time), counted once per pixel, not per channel.  The motion of a picture is one geometry: three grey calls
 * would read both fields three times.  No tap reads outside the (h-1)*pitch + 3*w bytes of a plane or the w*h*8 bytes of a field,
 * whatever the fields hold; bytes of a destination row beyond column 3*w - 1 are left untouched.
 *
 * ofx_interpolate_frames_3ch / ofx_interpolate_frames_3ch_batch: as ofx_interpolate_frames / ofx_interpolate_frames_batch, frame k
 * at d_dst3 + k*time_stride_bytes, rows dst_pitch >= 3*w apart.  The refusals are theirs, every pitch compared against 3*w, and a
 * plane of 2^31 bytes or more: OFX_E_INVALID, before anything is enqueued.  The host arrays are read before the call returns; the
 * stats slots need no initialisation and carry nothing from one call to the next, as there. */
int ofx_interpolate_frames_3ch(const uint8_t *d_a3, int a_pitch, const uint8_t *d_b3, int b_pitch, int w, int h,
                               const float *d_disp_ab, const float *d_disp_ba, const float *h_times, int n_times,
                               uint8_t *d_dst3, int dst_pitch, size_t time_stride_bytes, int64_t *d_stats /* may be NULL */, void *stream);
int ofx_interpolate_frames_3ch_batch(const uint8_t *const *d_a3, const int *a_pitches, const uint8_t *const *d_b3, const int *b_pitches,
                               int n, int w, int h, const float *const *d_disp_ab, const float *const *d_disp_ba, const float *h_times,
                               int n_times, uint8_t *const *d_dst3, int dst_pitch, size_t time_stride_bytes,
                               int64_t *const *d_stats /* may be NULL */, void *stream);

/* ---- coarse-to-fine propagation ------------------------------------------------
 * The reference hands a level ONE vector of the level above -- pixel 0's, as a global translation (ofx_shift_vector) -- and every
 * consumer of a displacement inherits that: beyond about 2 px per frame, or with two motions in one scene, the local estimate is
 * noise.  Here a level starts from the whole flow of the level above.  THE definition (everything else quotes it).
 *
 * PROLONGATION of a coarse field c (wc x hc, interleaved (u, v) float32, tightly packed) to a fine size w in {2*wc, 2*wc + 1},
 * h in {2*hc, 2*hc + 1}, with a `scale` (field units -> pixels) and a `max_px` >= 0.  Every float32 operation is rounded once,
 * nothing is fused, denormals are kept.
 *   1. Sanitise.  A coarse vector is replaced by (+0, +0) when either component is not finite and, with max_px > 0, when
 *      |scale*u| > max_px or |scale*v| > max_px (the product rounded once to float; `>` is false for a NaN, and the finiteness
 *      test has caught those).  max_px == 0: only the finiteness test.
 *   2. Sample at (x/2, y/2): pixel xc of pyramid level k + 1 sits at position 2*xc of level k, because ofx_downsample_1ch centres
 *      its stencil there.  x0 = min(x >> 1, wc - 1), x1 = min(x0 + 1, wc - 1), a = c(., x0), b = c(., x1), per component:
 *        even x: a itself, no arithmetic (a + 0*(b - a) would turn -0 into +0);
 *        odd x:  a + 0.5f*(b - a): the difference, the product, the sum.
 *      Horizontally first, on the coarse rows y0 = min(y >> 1, hc - 1) and y1 = min(y0 + 1, hc - 1); then the same rule
 *      vertically on the two results (even y: row y0's result itself).
 *   3. fine(x, y) = 2.0f * that (exact, unless it overflows to Inf).
 *   4. warped = what ofx_warp_levels writes for {src, fine, scale}, byte for byte: orc_warp_bilinear_u8's operation order,
 *      replicate border, and a pixel with |x + scale*u| > 1e9, |y + scale*v| > 1e9 or a NaN there is NOT WARPED.
 *
 * A PAIR'S DENSE FLOW, for L levels and iters >= 1 launches per level, lk_float:
 *   level L-1:  what ofx_session_run_flow computes for that level: iteration 1 is the reference's level (it is not shifted), then
 *               iters - 1 refinement iterations.
 *   level k < L-1, no global shift:  flow_k = prolong(flow_{k+1}; scale = OFX_ITER_SCALE, max_px);  W = warped(next_k, flow_k);
 *               then iters times:  flow_k += LK(prev_k, W), a float32 add, the solve under the min_det guard;  and
 *               W = ofx_warp_levels(next_k, flow_k, OFX_ITER_SCALE) for all but the last.
 *   The level's displacement in pixels is OFX_ITER_SCALE * flow_k: ofx_flow_displacement with d_uv = NULL.
 *
 * ofx_flow_prolong: 1 <= n <= OFX_MAX_LEVELS prolongations in ONE launch.  d_src / d_dst (both or neither): the launch also
 * writes step 4's image, from the fine vectors it holds in registers; d_src is the next image of the fine level (row pitch
 * src_pitch >= w), d_dst a plane that does not overlap it (row pitch dst_pitch >= w; the bytes beyond column w - 1 of a row are
 * left untouched).  d_coarse and d_fine 8-byte aligned and not overlapping; w * h < 2^28 and a plane below 2^31 bytes; scale
 * finite; max_px finite and >= 0; otherwise OFX_E_INVALID, before anything is enqueued.  No tap reads outside the
 * (h - 1) * pitch + w bytes of d_src or the wc * hc * 8 bytes of d_coarse, whatever the field holds. */
typedef struct ofx_prolong_desc {
    const float *d_coarse;
    int wc, hc;
    float *d_fine; /* 8-byte aligned, tightly packed */
    int w, h;
    float scale, max_px;
    const uint8_t *d_src; /* warp source (the next image of the fine level); NULL = flow only */
    int src_pitch;
    uint8_t *d_dst; /* warped image; bytes beyond column w-1 untouched */
    int dst_pitch;
} ofx_prolong_desc;
int ofx_flow_prolong(const ofx_prolong_desc *levels, int n, void *stream);

/* ---- flow median ---------------------------------------------------------------
 * Lucas-Kanade on weak texture leaves isolated wrong vectors, prolongation spreads each of them over four fine pixels and their
 * neighbours, and max_px only removes the wildest.  The standard remedy is a median filter on the intermediate flow fields after
 * every warping step (Sun, Roth, Black, "Secrets of optical flow estimation and their principles").  A median is a pure selection:
 * it needs no rounding.  THE definition (everything else quotes it), for a field f (w x h, interleaved (u, v) float32, tightly
 * packed) and a radius r in {1, 2}, i.e. a 3x3 or 5x5 window:
 *   1. Sanitise.  A vector with a component that is not finite is read as (+0, +0): prolongation's finiteness rule, without max_px.
 *   2. Select.  The window is the (2r+1)^2 vectors at (clamp(x + i, 0, w - 1), clamp(y + j, 0, h - 1)), |i|, |j| <= r: the border
 *      is replicated, so the count is always odd, also when w or h is smaller than the window.  Per component on its own, the
 *      result is the middle one of the (2r+1)^2 sanitised values ordered by value.  A selection: no arithmetic, no averaging.
 *   3. Zeros.  -0 and +0 compare equal, so a result equal to zero is stored as +0 (m + 0.0f, one add); every other result has the
 *      selected value's bits, denormals kept.
 *   4. warped (optional) = what ofx_warp_levels writes for {src, the filtered field, scale}, byte for byte; the "not warped" rule
 *      of prolongation's step 4 applies.
 *
 * A PAIR'S DENSE FLOW WITH MEDIAN, for L levels, iters >= 1 and a radius r: the pair's dense flow above with one median after
 * every step that leaves a flow --
 *   level L-1:  as above, then flow_{L-1} = median(flow_{L-1}; r).
 *   level k < L-1:  flow_k = prolong(flow_{k+1}; OFX_ITER_SCALE, max_px);  W = warped(next_k, flow_k);  then iters times:
 *               flow_k += LK(prev_k, W);  flow_k = median(flow_k; r);  and W = ofx_warp_levels(next_k, flow_k, OFX_ITER_SCALE) for
 *               all but the last.
 *
 * ofx_flow_median: 1 <= n <= OFX_STREAM_MAX_BATCH items in ONE launch; they may differ in size and radius.  d_src / d_dst (both or
 * neither): the launch also writes step 4's image, from the filtered vectors it holds in registers; d_src has row pitch src_pitch
 * >= w, d_dst is a plane that does not overlap it (row pitch dst_pitch >= w; the bytes beyond column w - 1 of a row are left
 * untouched).  d_src_flow and d_dst_flow 8-byte aligned and not overlapping (a median is out of place); w, h > 0, w * h < 2^28 and
 * a plane below 2^31 bytes; radius 1 or 2; scale finite; otherwise OFX_E_INVALID, before anything is enqueued.  No tap reads
 * outside the w * h * 8 bytes of d_src_flow or the (h - 1) * pitch + w bytes of d_src, whatever the field holds. */
typedef struct ofx_median_desc {
    const float *d_src_flow;
    float *d_dst_flow; /* 8-byte aligned, tightly packed, not overlapping d_src_flow */
    int w, h, radius;
    float scale;          /* for the warp only */
    const uint8_t *d_src; /* warp source; NULL = flow only */
    int src_pitch;
    uint8_t *d_dst; /* warped image; bytes beyond column w-1 untouched */
    int dst_pitch;
} ofx_median_desc;
int ofx_flow_median(const ofx_median_desc *items, int n, void *stream);

/* ---- texture strength and feature selection -------------------------------------
 * The trackers (ofx_session_stream_tracks, ofx_advect_points) take caller-owned points.  Where Lucas-Kanade can measure motion at all
 * is decided by the smaller eigenvalue of the window's structure tensor (Shi, Tomasi, "Good features to track"): on a flat window
 * and on a single edge the 2x2 system is singular and the flow is NaN or noise.  THE definition (everything else quotes it):
 *
 * TEXTURE STRENGTH of a u8 plane p of w x h pixels (rows `pitch` apart), for an odd window 3 .. 23:
 *   1. Sxx, Syy, Sxy are planes 0, 1, 2 of what ofx_lk_level_sums(p, p, the whole level's geometry, window, OFX_MODE_LK_FLOAT, ..)
 *      writes: Ix, Iy the 3x3 Sobel correlations of p with the taps outside the image skipped, and the sums of Ix^2, Iy^2, Ix Iy over
 *      the window clipped at the image.  |Ix|, |Iy| <= 1020, so the sums are exact integers below 2^31 that depend on p only.
 *   2. In float64, every operation rounded once, nothing fused:
 *        tr = Sxx + Syy;  d = Sxx - Syy  (both exact);  q = d * d;  p2 = Sxy * Sxy;  p4 = 4 * p2 (exact);  r = q + p4;
 *        s = sqrt(r), correctly rounded (IEEE);  m = tr - s;  lambda = 0.5 * m (exact).
 *   3. strength = lambda rounded once to float32 when lambda > 0, else +0: never a NaN, never negative, never -0.
 *
 * FEATURE SELECTION on a strength plane R (float32, w x h) for a cell size c in 4 .. 256, a border b >= 0 and a min_strength that
 * is finite and >= 0:
 *   1. A pixel is a CANDIDATE when  b <= x < w - b  and  b <= y < h - b;  R(x, y) > min_strength (strict: with 0 a flat or singular
 *      pixel is never a candidate);  and, among its up to eight neighbours inside the image, R(x, y) > R(n) for every neighbour
 *      that comes before it in raster order and R(x, y) >= R(n) for every one after it (of a plateau the first pixel remains).
 *   2. The cell of a pixel is (x / c, y / c) on a grid of ncx x ncy = ceil(w / c) x ceil(h / c).  A cell's FEATURE is its candidate
 *      with the largest R; among equal ones the one with the smallest y * w + x.
 *   3. Per item:  cells = int32 [ncy][ncx][2] = (x, y), or (-1, -1);  cell_strength = float32 [ncy][ncx] = R of the feature, or +0;
 *      stats = four int64: [0] cells, [1] cells with a feature, [2] candidates, [3] pixels inside the border with
 *      R <= min_strength.  The counts are integers: they depend on no order, tile or batch.
 *
 * COMPACTION: the points are ((float)x, (float)y) of the occupied cells in cell raster order; only the first max_points of them
 * are written, *d_count = min(occupied, max_points), and the entries beyond *d_count are left untouched.
 *
 * ofx_texture_features: 1 <= n <= OFX_STREAM_MAX_BATCH items of any sizes; ONE launch writes every item's strength (the plane is read
 * once, through a buffer resource of exactly (h - 1) * pitch + w bytes: nothing is read outside it), a second one selects for the
 * items that have d_cells.  Refused with OFX_E_INVALID and a message naming the item, before anything is enqueued: null pointers,
 * n outside 1 .. OFX_STREAM_MAX_BATCH, an even window or one outside 3 .. 23, w or h <= 0, w * h >= 2^28, a pitch below w or no
 * multiple of 4 or a plane of 2^31 bytes, a pointer that is not 4-byte (d_stats: 8-byte) aligned, strength_pitch < w, a cell
 * outside 4 .. 256, a negative border, a min_strength that is negative or not finite, only one of d_cells and d_cell_strength, or
 * d_stats without cells.  The points for ofx_session_stream_tracks at `level`: these two calls on ofx_session_plane(s, 0, level).
 * d_stats needs no initialisation (the call zeroes it on the stream first); every output is written in full for the item's own extent
 * and nothing is carried from one call to the next. */
typedef struct ofx_texture_desc {
    const uint8_t *d_plane;
    int pitch, w, h;         /* pitch a multiple of 4, plane 4-byte aligned: what ofx_geom asks */
    float *d_strength;
    int strength_pitch;      /* in floats, >= w; the pad floats of a row are left untouched */
    int32_t *d_cells;        /* [ncy][ncx][2]; NULL = strength only */
    float *d_cell_strength;  /* [ncy][ncx]; with d_cells or not at all */
    int64_t *d_stats;        /* four int64, 8-byte aligned; may be NULL */
    int cell, border;
    float min_strength;
} ofx_texture_desc;
int ofx_texture_features(const ofx_texture_desc *items, int n, int window, void *stream);
int ofx_compact_features(const int32_t *d_cells, int n_cells, int max_points, float *d_points, int32_t *d_count, void *stream);

/* ---- sparse Lucas-Kanade tracking --------------------------------------------------
 * ofx_advect_points adds the composed field of main.cu:138-147 at a point's pixel; that field is not a displacement.  This block
 * tracks chosen points IN PIXELS: per point an iterative, coarse-to-fine Lucas-Kanade (Lucas, Kanade 1981; Bouguet's pyramidal
 * form) on a lattice of 1/32 px.  Everything up to the 2x2 solve is exact integer arithmetic, so no order of summation has to be
 * fixed, and the solve is float64 with one rounding per operation.  THE definition (tests/klt_ref.py restates it in NumPy):
 *
 * INPUTS: two grey pyramids A (frame p - 1) and B (frame p) of `levels` u8 planes, 1 <= levels <= 8; level k is (w >> k) x (h >> k)
 * and the coarsest level has w, h >= 1 (how the planes were made is the caller's business: ofx_pyramid_1ch makes them); w, h <=
 * 2^19, so that every lattice position is exact in float32; an odd window 3 .. 23, R = window / 2; max_iters in 1 .. 32; eps_q >= 0;
 * min_lambda >= 0 and finite; max_sad >= 0 (0 = off).
 *
 * LATTICE: a position q = 32 ix + a with a in 0 .. 31; ix = q >> 5 and a = q & 31 on the two's-complement value (floor division).
 * SAMPLE S(P, qx, qy), with (ix, a) of qx and (iy, b) of qy:
 *   s = (32-a)(32-b) P(ix, iy) + a(32-b) P(ix+1, iy) + (32-a)b P(ix, iy+1) + ab P(ix+1, iy+1), every tap's column and row clamped
 *   to the plane (replicate);  S = (s + 16) >> 5, in 0 .. 8160 (1/32 grey level).
 *
 * A point (x, y) float32 with status 0, per pair:
 *   START  x, y must be finite and inside [0, w-1] x [0, h-1] of level 0, else the point is lost with reason START.
 *          d = (0, 0), int32, in 1/32 px of the current level.
 *   LEVEL  k = levels-1 .. 0:  below the coarsest level d is doubled first.
 *          c = (lrintf(ldexpf(x, 5 - k)), lrintf(ldexpf(y, 5 - k))), ties to even.
 *          For i, j in -R .. R:  I(i,j) = S(A_k, cx + 32 i, cy + 32 j);  gx(i,j) = S(A_k, cx + 32 (i+1), cy + 32 j) - S(A_k, cx +
 *          32 (i-1), cy + 32 j);  gy likewise in j.  Gxx = sum gx^2, Gyy = sum gy^2, Gxy = sum gx gy: exact integers below 2^36.
 *          In float64:  D = Gxx * Gyy - Gxy * Gxy (two products, one difference);  lambda = step 2 of TEXTURE STRENGTH on (Gxx,
 *          Gyy, Gxy).  The level is SINGULAR when !(D > 0) or !(lambda > min_lambda): at k > 0 it is skipped and d is kept, at
 *          k = 0 the point is lost with reason SINGULAR.  Otherwise up to max_iters times:
 *            e(i,j) = S(B_k, cx + dx + 32 i, cy + dy + 32 j) - I(i,j);  bx = sum gx e, by = sum gy e (exact integers);
 *            sx = -64 * ((Gyy * bx - Gxy * by) / D),  sy = -64 * ((Gxx * by - Gxy * bx) / D)  in float64: two products, one
 *            difference, one IEEE division, one (exact) scaling -- g is twice the derivative and the step is wanted in 1/32 px;
 *            t = rint(s) clamped to [-2048, 2048], ties to even;  d += t;  stop after an update with |tx| <= eps_q and |ty| <= eps_q.
 *   END    q = c + d at level 0.  Outside [0, 32 (w-1)] x [0, 32 (h-1)]: lost with reason OUT.  sad = sum |S(B_0, q + 32 (i,j)) -
 *          I(i,j)| (at most 529 * 8160);  max_sad > 0 and sad > max_sad: lost with reason RESIDUAL.  Otherwise the point moves to
 *          ((float)qx / 32, (float)qy / 32), which is exact: the next pair starts from the same lattice point.
 * A lost point keeps its position and its status becomes (pair << 8) | reason, reasons OFX_TRACK_START .. OFX_TRACK_RESIDUAL; a
 * point whose status is not 0 on entry is not touched.
 *
 * CHAIN: a launch carries n_frames = 2 .. 17 frames, n_frames - 1 <= OFX_STREAM_MAX_BATCH pairs, numbered pair0, pair0 + 1, ..; a
 * point walks them in order, the template of a pair taken in its first frame at the point's current position: the result does not
 * depend on how a clip is cut into launches.
 *
 * OUTPUTS per pair b (each may be NULL):  d_history [pairs][n][2] float32, the positions after the pair, frozen ones included;
 * d_sad [pairs][n] int32, -1 for a point not tracked in that pair;  d_stats [pairs][7] int64: [0] points alive after the pair,
 * [1 .. 4] points lost in it by reasons 1 .. 4, [5] iterations summed over points and levels, [6] the sum of sad over the points
 * tracked.  Integer counts: any order of atomics gives them; the call zeroes them on the stream first.
 *
 * ofx_track_points: ONE launch.  clip->planes is a HOST table of n_frames x levels device planes (frame-major), clip->pitches one
 * pitch per level; any pitch >= w >> k and any alignment, the taps are bytes, and every tap is clamped before it becomes an
 * address.  Refused with OFX_E_INVALID and a message naming the argument, before anything is enqueued: null pointers (a plane
 * among them), levels outside 1 .. 8 or a coarsest level of width or height 0, w or h above 2^19, n_frames outside 2 .. 17, an
 * even window or one outside 3 .. 23, max_iters outside 1 .. 32, eps_q < 0, min_lambda negative or not finite, max_sad < 0,
 * pair0 < 1 or pair0 + pairs >= 2^23, n_points < 1, a pitch below the level's width or a plane of 2^31 bytes or more, d_points or
 * d_history not 8-byte aligned, d_status or d_sad not 4-byte aligned, d_stats not 8-byte aligned.  d_history, d_sad and d_stats need
 * no initialisation and carry nothing from one call to the next: d_points and d_status alone hold the chain's state. */
#define OFX_TRACK_START 1
#define OFX_TRACK_SINGULAR 2
#define OFX_TRACK_OUT 3
#define OFX_TRACK_RESIDUAL 4
#define OFX_TRACK_MAX_LEVELS 8
typedef struct ofx_track_clip {
    int w, h, levels, n_frames;
    const uint8_t *const *planes; /* host table: planes[f * levels + k] = level k of frame f, on the device */
    const int *pitches;           /* host table: [levels], in bytes */
} ofx_track_clip;
typedef struct ofx_track_params {
    int window, max_iters, eps_q, max_sad;
    float min_lambda;
} ofx_track_params;
int ofx_track_points(const ofx_track_clip *clip, const ofx_track_params *prm, int pair0, float *d_points, int32_t *d_status, int n_points,
                     float *d_history, int32_t *d_sad, int64_t *d_stats, void *stream);

/* ---- camera motion from point matches ---------------------------------------------
 * The trackers hand back per-point displacements, some of them wrong or on moving objects.  This block answers what they were
 * gathered for: how did the camera move between two frames?  A robust translation / similarity / affine model per pair: RANSAC
 * (Fischler, Bolles 1981) over a counter-based sampler, integer inlier counts, and a least-squares refit whose sums are exact
 * integers up to a small float64 solve.  THE definition (tests/fit_motion_ref.py restates it in NumPy):
 *
 * INPUTS per item (a pair): n matches, 1 <= n <= 2^20; p[i] and q[i] float32 (x, y), p the position in the first frame, q in the
 * second; optionally status[i] and a pair number `pair`; the frame size w, h, each in 1 .. 2^16.
 * PARAMETERS per call: model OFX_MOTION_TRANSLATION (K = 1 sampled match), OFX_MOTION_SIMILARITY (K = 2) or OFX_MOTION_AFFINE
 * (K = 3); hypotheses H in 1 .. 4096; thr_q in 0 .. 2^15, the inlier radius in 1/32 px; refits in 0 .. 3; seed, a uint32.
 *
 * LATTICE  P = (lrintf(ldexpf(px, 5)), lrintf(ldexpf(py, 5))), the tracker's lattice (tracked points sit on it exactly), Q likewise;
 *          u = P - o, v = Q - o with o = (16 (w - 1), 16 (h - 1)): relative to the frame's centre, so that the refit stays well
 *          conditioned.  |u| <= 2^20: products are at most 2^40 and sums over 2^20 matches at most 2^60, exact in int64 in any order.
 * USABLE   match i is usable when all four floats are finite, p and q lie inside [0, w-1] x [0, h-1] and, with a status array,
 *          status[i] == 0 || (status[i] >> 8) > pair: alive through this pair in ofx_track_points' encoding, so that a chain's
 *          d_history rows and its single status array can be passed as they are.
 * SAMPLER  mix(seed, j, k, a) in uint32 arithmetic:
 *            h = seed ^ j*0x9E3779B1 ^ k*0x85EBCA77 ^ a*0xC2B2AE3D;  h ^= h>>16;  h *= 0x7FEB352D;  h ^= h>>15;  h *= 0x846CA68B;  h ^= h>>16
 *          and the index i = (uint64(h) * n) >> 32.  Sample k = 0 .. K-1 of hypothesis j: attempts a = 0 .. 7 in order, the first i
 *          that is usable and differs from the hypothesis's earlier indices; if all eight fail the hypothesis is INVALID.
 * MODEL of a hypothesis: six float64 (a, b, tx, c, d, ty) that map u to v; every floating operation is float64 and rounded once,
 *          nothing fused; integer expressions are exact int64 and converted once.
 *            translation  (1, 0, v0x - u0x, 0, 1, v0y - u0y)
 *            similarity   dp = u1 - u0, dq = v1 - v0;  den = dpx^2 + dpy^2, INVALID when 0;  sa = (dpx dqx + dpy dqy) / den;
 *                         sb = (dpx dqy - dpy dqx) / den;  (a, b, c, d) = (sa, -sb, sb, sa)
 *            affine       d1 = u1 - u0, d2 = u2 - u0, e1 = v1 - v0, e2 = v2 - v0;  det = d1x d2y - d1y d2x, INVALID when 0;
 *                         a = (e1x d2y - e2x d1y) / det;  b = (e2x d1x - e1x d2x) / det;  c = (e1y d2y - e2y d1y) / det;
 *                         d = (e2y d1x - e1y d2x) / det
 *          and for the last two  tx = v0x - (a u0x + b u0y),  ty = v0y - (c u0x + d u0y): two products, one sum, one difference.
 * SCORE    rx = (a ux + b uy) + (tx - vx), ry likewise;  e2 = rx rx + ry ry;  an INLIER is a usable match with e2 <= (double)thr_q *
 *          thr_q.  count_j = the inliers, an integer.  The best hypothesis is the valid j with the largest count, among equal
 *          counts the smallest j: an integer comparison, so any order of reduction gives it.
 * REFIT    `refits` times: over the inliers of the current model the int64 sums m, Sx = sum ux, Sy, Sxx = sum ux^2, Sxy, Syy, Vx = sum
 *          vx, Vy, Sxvx = sum ux vx, Syvx, Sxvy, Syvy, each converted to float64 (to nearest even); n = (double)m;
 *            Cxx = n Sxx - Sx Sx;  Cyy = n Syy - Sy Sy;  Cxy = n Sxy - Sx Sy;  Cxvx = n Sxvx - Sx Vx;  Cyvx, Cxvy, Cyvy likewise;
 *            translation  t = ((Vx - Sx) / n, (Vy - Sy) / n);  skipped when m == 0
 *            similarity   den = Cxx + Cyy, skipped when !(den > 0);  sa = (Cxvx + Cyvy) / den;  sb = (Cxvy - Cyvx) / den
 *            affine       D = Cxx Cyy - Cxy Cxy, skipped when !(D > 0);  a = (Cyy Cxvx - Cxy Cyvx) / D;  b = (Cxx Cyvx - Cxy Cxvx) / D;
 *                         c, d the same on Cxvy, Cyvy
 *          and for the last two  tx = (Vx - (a Sx + b Sy)) / n,  ty = (Vy - (c Sx + d Sy)) / n.  A skipped refit keeps the model.
 * OUTPUTS per item:  d_model float64 [6] in pixels about the image origin: the linear part unchanged, tx_px = ((tx + ox) - (a ox +
 *          b oy)) / 32, ty_px likewise.  d_info int32 [8]: [0] OFX_FIT_OK, OFX_FIT_FEW (fewer than K usable matches) or
 *          OFX_FIT_DEGENERATE (no valid hypothesis); [1] usable matches; [2] valid hypotheses; [3] the best j, or -1; [4] its count;
 *          [5] inliers of the final model; [6] refits that were not skipped; [7] 0.  d_inlier (may be NULL) uint8 [n]: 1 or 0 under
 *          the final model.  On a status other than OK the model is (1, 0, 0, 0, 1, 0), [3] = -1, [4 .. 6] = 0 and the mask zeros.
 *
 * ofx_fit_motion: 1 <= n_items <= OFX_STREAM_MAX_BATCH items that may differ in n, w and h, 5 + refits launches on the stream (the
 * hypotheses' models into d_work, the H x n scores, the choice, a pass over the matches per refit and one for the mask, the
 * outputs), nothing returns to the host between them.  d_work: ofx_fit_motion_work_bytes(prm) bytes
 * per item (host arithmetic; 0 for parameters that would be refused), 8-byte aligned, the caller's, its contents undefined
 * afterwards; items must not share it.  Refused with OFX_E_INVALID and a message naming the item and the argument, before anything
 * is enqueued: null pointers (d_status and d_inlier may be NULL), any range above, d_p, d_q, d_model or d_work not 8-byte aligned,
 * d_info or d_status not 4-byte aligned.  d_work needs no initialisation (the first launch resets every word a later one adds to)
 * and carries nothing from one call to the next: calls with other parameters may follow each other in the same buffer.
 *
 * Host only, in the manner of ofx_generate_gaussian_kernel, on float64 [6] models (a, b, tx, c, d, ty); out may be an input:
 *   ofx_motion_compose  out = m2 after m1:  a = a2 a1 + b2 c1;  b = a2 b1 + b2 d1;  tx = (a2 tx1 + b2 ty1) + tx2;  c, d, ty likewise
 *                       with (c2, d2, ty2): products, then sums left to right.
 *   ofx_motion_invert   det = a d - b c, OFX_E_INVALID when it is 0 or not finite;  ia = d / det;  ib = -b / det;  ic = -c / det;
 *                       id = a / det;  itx = -(ia tx + ib ty);  ity = -(ic tx + id ty). */
#define OFX_MOTION_TRANSLATION 0
#define OFX_MOTION_SIMILARITY 1
#define OFX_MOTION_AFFINE 2
#define OFX_FIT_OK 0
#define OFX_FIT_FEW 1
#define OFX_FIT_DEGENERATE 2
typedef struct ofx_fit_desc {
    const float *d_p, *d_q;  /* [n][2], 8-byte aligned */
    const int32_t *d_status; /* [n]; NULL = every match alive */
    int n, pair, w, h;
    double *d_model;         /* [6] */
    int32_t *d_info;         /* [8] */
    uint8_t *d_inlier;       /* [n]; may be NULL */
    void *d_work;            /* ofx_fit_motion_work_bytes(prm) bytes, 8-byte aligned */
} ofx_fit_desc;
typedef struct ofx_fit_params {
    int model, hypotheses, thr_q, refits;
    uint32_t seed;
} ofx_fit_params;
size_t ofx_fit_motion_work_bytes(const ofx_fit_params *prm);
int ofx_fit_motion(const ofx_fit_desc *items, int n_items, const ofx_fit_params *prm, void *stream);
int ofx_motion_compose(const double *m2, const double *m1, double *out);
int ofx_motion_invert(const double *m, double *out);

/* ---- planar homography from point matches -----------------------------------------
 * The block above stops at six parameters, exact only for a camera that does not rotate out of the image plane.  A camera that
 * pans or tilts in front of a plane or a distant scene moves the image by a planar homography: the fourth model, fitted the same
 * way -- RANSAC over the same sampler, integer inlier counts, a least-squares refit on exact integer sums -- with an 8 x 8 solve, a
 * division-free rational residual and 128-bit sums.  THE definition (tests/homography_ref.py restates it in NumPy and Python ints):
 *
 * INPUTS, PARAMETERS, LATTICE, USABLE, SAMPLER: those of "camera motion from point matches", with model = OFX_MOTION_HOMOGRAPHY and
 *          K = 4 samples per hypothesis.  Every floating operation below is float64 and rounded once, nothing fused; every integer
 *          expression is exact.
 * SCALE    e = the smallest integer >= 0 with 2^e >= max(16 (w - 1), 16 (h - 1), 1).  A lattice value u becomes the normalised
 *          x = ldexp((double)u, -e): exact, |x| <= 1.  Below (x, y) is the normalised u of a match and (X, Y) its normalised v.
 * SOLVE    of an 8 x 9 augmented system M (8 equations, the right-hand side in column 8), Gaussian elimination with partial pivoting:
 *          for c = 0 .. 7:  the pivot row p starts as c, and each r = c + 1 .. 7 in order replaces it when |M[r][c]| > |M[p][c]|
 *          (the largest magnitude, the smallest row among equals);  INVALID when M[p][c] is 0 or not finite;  rows p and c are
 *          swapped;  for each r = c + 1 .. 7:  f = M[r][c] / M[c][c], then for k = c + 1 .. 8:  M[r][k] = M[r][k] - f M[c][k].
 *          Back substitution for c = 7 .. 0:  s = M[c][8], then for k = c + 1 .. 7 in order  s = s - M[c][k] h[k];  h[c] = s / M[c][c].
 *          INVALID when any h[c] is not finite.
 * MODEL of a hypothesis: (h0 .. h7, 1), row-major 3 x 3, maps normalised u to normalised v.  From its four samples in order, k = 0 .. 3:
 *            row 2k     = [x  y  1  0  0  0  -(x X)  -(y X) | X]
 *            row 2k + 1 = [0  0  0  x  y  1  -(x Y)  -(y Y) | Y]
 *          then SOLVE.  The hypothesis is INVALID when the sampler or the solve says so, or when (h6 x + h7 y) + 1 is not > 0 at any
 *          of its four samples.
 * SCORE    W = (h6 x + h7 y) + 1;  rx = ((h0 x + h1 y) + h2) - X W;  ry = ((h3 x + h4 y) + h5) - Y W;  t = ldexp((double)thr_q, -e).
 *          An INLIER is a usable match with W > 0 and rx rx + ry ry <= (t W) (t W): the transfer error against the radius, without
 *          a division.  count_j = the inliers, an integer; the best hypothesis is the valid j with the largest count, among equal
 *          counts the smallest j.
 * REFIT    `refits` times, over the inliers of the current model: the normal equations of min sum (h0 x + h1 y + h2 - X (h6 x + h7 y
 *          + 1))^2 + (h3 x + h4 y + h5 - Y (h6 x + h7 y + 1))^2.  In the lattice integers (ux, uy) -> (x, y), (vx, vy) -> (X, Y), with
 *          R = X X + Y Y, the 23 exact sums
 *            degree 0  m (the count)                      degree 1  Sx, Sy, SX, SY
 *            degree 2  Sxx, Sxy, Syy, SxX, SyX, SxY, SyY    degree 3  SxxX, SxyX, SyyX, SxxY, SxyY, SyyY, SxR, SyR
 *            degree 4  SxxR, SxyR, SyyR
 *          (SxyX = sum ux uy vx, SxR = sum ux (vx vx + vy vy), ...).  Those of degree 3 and 4 reach 2^101 in magnitude: 128-bit
 *          two's-complement integers, exact in any order.  Each sum of degree d is converted to float64 ONCE, to nearest even,
 *          then scaled by ldexp(., -d e) (exact).  The system, in the scaled sums (a minus sign is exact):
 *            row 0 = [ Sxx    Sxy    Sx    0      0      0     -SxxX  -SxyX |  SxX ]
 *            row 1 = [ Sxy    Syy    Sy    0      0      0     -SxyX  -SyyX |  SyX ]
 *            row 2 = [ Sx     Sy     m     0      0      0     -SxX   -SyX  |  SX  ]
 *            row 3 = [ 0      0      0     Sxx    Sxy    Sx    -SxxY  -SxyY |  SxY ]
 *            row 4 = [ 0      0      0     Sxy    Syy    Sy    -SxyY  -SyyY |  SyY ]
 *            row 5 = [ 0      0      0     Sx     Sy     m     -SxY   -SyY  |  SY  ]
 *            row 6 = [-SxxX  -SxyX  -SxX  -SxxY  -SxyY  -SxY    SxxR   SxyR | -SxR ]
 *            row 7 = [-SxyX  -SyyX  -SyX  -SxyY  -SyyY  -SyY    SxyR   SyyR | -SyR ]
 *          then SOLVE.  The refit is skipped, and the model kept, when m < 4 or the solve is INVALID.
 * OUTPUTS  d_model float64 [9], row-major, in pixels about the image origin (q ~ ((g0 px + g1 py + g2) / W, (g3 px + g4 py + g5) / W),
 *          W = g6 px + g7 py + 1): the final (h0 .. h7, h8 = 1) conjugated with the map pixels -> normalised, x = s px - cx.  With
 *          s = ldexp(1.0, 5 - e), cx = ldexp((double)(16 (w - 1)), -e), cy = ldexp((double)(16 (h - 1)), -e), for each row i = 0, 1, 2:
 *            A[i][0] = h[3i] s;  A[i][1] = h[3i+1] s;  A[i][2] = h[3i+2] - (h[3i] cx + h[3i+1] cy)
 *          and for each column j:  B[0][j] = A[0][j] + cx A[2][j];  B[1][j] = A[1][j] + cy A[2][j];  B[2][j] = s A[2][j];
 *          g[3i+j] = B[i][j] / B[2][2].  When B[2][2] is 0 or not finite the item ends OFX_FIT_DEGENERATE.
 *          d_info and d_inlier as in "camera motion from point matches" (OFX_FIT_FEW: fewer than 4 usable matches); on a status
 *          other than OK the model is the identity (1, 0, 0, 0, 1, 0, 0, 0, 1), [3] = -1, [4 .. 6] = 0 and the mask zeros.
 *
 * ofx_fit_homography: ofx_fit_motion's descriptors (d_model float64 [9] here), parameters (model must be OFX_MOTION_HOMOGRAPHY),
 * ranges, alignments and refusals; 1 <= n_items <= OFX_STREAM_MAX_BATCH items that may differ in n, w and h; 5 + 2 refits launches
 * on the stream (hypotheses, scores, the choice, per refit the sums and a one-block solve, the mask, the outputs), nothing returns
 * to the host between them.  d_work: ofx_fit_homography_work_bytes(prm) bytes per item (0 for parameters that would be refused),
 * 8-byte aligned, the caller's, undefined afterwards; items must not share it.  It needs no initialisation and carries nothing from
 * one call to the next, as there. */
#define OFX_MOTION_HOMOGRAPHY 3
size_t ofx_fit_homography_work_bytes(const ofx_fit_params *prm);
int ofx_fit_homography(const ofx_fit_desc *items, int n_items, const ofx_fit_params *prm, void *stream);

/* ---- affine frame warp ------------------------------------------------------------
 * Every other warp of this library takes a dense 8 B/px field.  This one applies a parametric motion -- a model of the block above,
 * or any float64 [6] -- to a u8 frame of 1 or 3 interleaved channels: fixed point, on the tracker's 1/32 px lattice, the same bits
 * everywhere.  THE definition (tests/warp_affine_ref.py restates it in NumPy):
 *
 * INPUTS: a destination of w x h pixels and a source of sw x sh pixels, both u8, `channels` C in {1, 3} interleaved; m = (a, b, tx,
 * c, d, ty) float64, the INVERSE map: output pixel (x, y) shows the source at (a x + b y + tx, c x + d y + ty), in pixels.
 * QUANTISATION, on the host:  A = llrint(a * 2^21), likewise B, C, D, Tx, Ty; ties to even.  Refused: an entry that is not finite,
 *   |a|, |b|, |c|, |d| > 16, |tx|, |ty| > 2^20;  w, h, sw, sh in 1 .. 2^16.
 * POSITION  qx = (A x + B y + Tx + 2^15) >> 16,  qy = (C x + D y + Ty + 2^15) >> 16: int64, arithmetic shift; the source position
 *   in 1/32 px.  It is IN RANGE when 0 <= qx <= 32 (sw - 1) and 0 <= qy <= 32 (sh - 1).
 * BORDER    OFX_BORDER_REPLICATE: qx and qy are clamped to the range.  OFX_BORDER_CONSTANT: a pixel out of range gets `fill`
 *   (0 .. 255) in every channel.
 * VALUE     (ix, fa) = (qx >> 5, qx & 31), (iy, fb) = (qy >> 5, qy & 31), the tracker's LATTICE; per channel s = (32-fa)(32-fb)
 *   P(ix, iy) + fa(32-fb) P(ix+1, iy) + (32-fa)fb P(ix, iy+1) + fa fb P(ix+1, iy+1), the tracker's bilinear sum, the taps clamped to
 *   the plane;  out = (s + 512) >> 10.
 * d_outside (may be NULL; 8-byte aligned): one int64 per item, the output pixels out of range, under either border mode; the call
 *   zeroes it on the stream first.
 * The identity copies the source; a whole-pixel translation gives a shifted copy exactly.
 *
 * ofx_warp_affine: 1 <= n <= OFX_STREAM_MAX_BATCH items of any sizes, channels, borders and models in ONE launch.  Any pitch of at
 * least C w (C sw) and any alignment; d_src and d_dst must not overlap; the bytes of a destination row beyond column C w - 1 stay
 * untouched; no tap reads outside the (sh - 1) src_pitch + C sw bytes of the source, whatever the model.  Refused with
 * OFX_E_INVALID and a message naming the item and the argument, before anything is enqueued: null pointers, n, channels, border,
 * fill, a size or a model entry outside its range, a pitch below its row, planes that overlap, d_outside not 8-byte aligned. */
#define OFX_BORDER_CONSTANT 0
#define OFX_BORDER_REPLICATE 1
typedef struct ofx_warp_affine_desc {
    const uint8_t *d_src;
    int src_pitch, sw, sh;
    uint8_t *d_dst;
    int dst_pitch, w, h;
    int channels, border, fill;
    double model[6];
    int64_t *d_outside;
} ofx_warp_affine_desc;
int ofx_warp_affine(const ofx_warp_affine_desc *items, int n, void *stream);

/* ---- perspective frame warp -------------------------------------------------------
 * A camera that pans or tilts in front of a plane or a distant scene moves the image by a planar homography, which no six
 * parameters hold.  This block applies one: ofx_warp_affine with a float64 [9] model and a division per pixel.  THE definition
 * (tests/warp_persp_ref.py restates it in NumPy):
 *
 * INPUTS: those of "affine frame warp", with m = (m0 .. m8) float64, the INVERSE map, row-major 3 x 3: output pixel (x, y) shows the
 *   source at ((m0 x + m1 y + m2) / (m6 x + m7 y + m8), (m3 x + m4 y + m5) / (m6 x + m7 y + m8)), in pixels.  The model is used
 *   as it is, not quantised.  Refused: an entry that is not finite, |m0|, |m1|, |m3|, |m4| > 16, |m2|, |m5| > 2^20, |m6|, |m7| > 1,
 *   |m8| > 16;  w, h, sw, sh in 1 .. 2^16.
 * POSITION for integer output (x, y), every operation float64 and rounded once, nothing fused, x and y converted exactly:
 *   X = (m0 x + m1 y) + m2;  Y = (m3 x + m4 y) + m5;  W = (m6 x + m7 y) + m8;  r = 1.0 / W;  fx = ldexp(X r, 5);  fy = ldexp(Y r, 5).
 *   Every pixel from its own x and y: nothing is accumulated along a row.
 * UNDEFINED when W is not > 0 (behind the horizon, on it, or NaN), or fx or fy is not finite or exceeds 2^40 in magnitude.  An
 *   undefined pixel gets `fill` in every channel under EITHER border mode and counts in d_outside.
 * Otherwise qx = llrint(fx), qy = llrint(fy), ties to even: the source position in 1/32 px, and the pixel follows IN RANGE, BORDER
 *   and VALUE of "affine frame warp" from there on; d_outside counts the pixels undefined or out of range.
 * The identity (1, 0, 0, 0, 1, 0, 0, 0, 1) copies the source; a whole-pixel translation gives a shifted copy exactly; a model
 * whose bottom row is (0, 0, 1) and whose other entries are multiples of 1/32 gives ofx_warp_affine's bytes for (m0 .. m5), because
 * nothing rounds in either.
 *
 * ofx_warp_perspective: 1 <= n <= OFX_STREAM_MAX_BATCH items of any sizes, channels, borders and models in ONE launch.  Pitches,
 * alignment, the no-overlap rule, the untouched tail of a destination row, "no tap reads outside the source", d_outside and the
 * refusals are ofx_warp_affine's.
 *
 * Host only, on float64 [9] row-major models; out may be an input:
 *   ofx_homography_compose      out = m2 after m1, the 3 x 3 product:  out[3i+j] = (m2[3i] m1[j] + m2[3i+1] m1[3+j]) + m2[3i+2] m1[6+j]:
 *                               products, then sums left to right; NOT renormalised.
 *   ofx_homography_invert       c0 = m4 m8 - m5 m7;  c1 = m5 m6 - m3 m8;  c2 = m3 m7 - m4 m6;  det = (m0 c0 + m1 c1) + m2 c2,
 *                               OFX_E_INVALID when it is 0 or not finite;  out = the adjugate (c0, m2 m7 - m1 m8, m1 m5 - m2 m4;
 *                               c1, m0 m8 - m2 m6, m2 m3 - m0 m5;  c2, m1 m6 - m0 m7, m0 m4 - m1 m3), each entry divided by det.
 *   ofx_homography_normalize    out[k] = m[k] / m[8];  OFX_E_INVALID when m[8] is 0 or not finite.
 *   ofx_homography_from_affine  (a, b, tx, c, d, ty) -> (a, b, tx, c, d, ty, 0, 0, 1). */
typedef struct ofx_warp_persp_desc {
    const uint8_t *d_src;
    int src_pitch, sw, sh;
    uint8_t *d_dst;
    int dst_pitch, w, h;
    int channels, border, fill;
    double model[9];
    int64_t *d_outside;
} ofx_warp_persp_desc;
int ofx_warp_perspective(const ofx_warp_persp_desc *items, int n, void *stream);
int ofx_homography_compose(const double *m2, const double *m1, double *out);
int ofx_homography_invert(const double *m, double *out);
int ofx_homography_normalize(const double *m, double *out);
int ofx_homography_from_affine(const double *m6, double *out);

/* ---- frame mosaic -------------------------------------------------------------------
 * A stabilised frame warped alone shows `fill`, or smeared edge pixels, wherever the smoothed camera looks past the edge of the
 * shaky frame; the neighbouring frames, placed in the same plane by their own maps, saw what it missed.  This block looks through
 * several sources per output pixel, in priority order, and shows the first that holds the pixel; panoramas and background plates
 * are the same launch.  THE definition (tests/mosaic_ref.py restates it in NumPy), on top of "perspective frame warp":
 *
 * INPUTS: a destination of w x h pixels, u8, `channels` C in {1, 3} interleaved; n_sources S in 1 .. OFX_MOSAIC_MAX_SOURCES sources;
 *   source k a u8 plane of sw_k x sh_k pixels with the same C, a pitch of its own and a float64 [9] INVERSE map m_k as in
 *   "perspective frame warp": used as it is, with the same ranges and refusals per entry.  Sources may differ in size, may be the
 *   same plane and may overlap each other; none may overlap the destination or the d_which plane.
 * PER SOURCE k and output pixel (x, y): POSITION and UNDEFINED are those of "perspective frame warp" with m_k, from the pixel's own
 *   x and y; IN RANGE is that of "affine frame warp" with (sw_k, sh_k).  Source k COVERS the pixel when its position is defined and
 *   in range; its value there is VALUE of "affine frame warp".
 * CHOICE    k* = the smallest k that covers the pixel: the output is source k*'s value and which = k*.  When no source covers the
 *   pixel, which = 255 and the output is: under OFX_BORDER_CONSTANT `fill` in every channel; under OFX_BORDER_REPLICATE exactly
 *   what ofx_warp_perspective gives for source 0 under replicate -- the value at its clamped position, or `fill` where source 0 is
 *   undefined there.
 * OUTPUTS   d_dst.  d_which (may be NULL): a u8 plane of w x h with a pitch of its own >= w, at any alignment, holding k* or 255;
 *   the bytes of a row beyond column w - 1 stay untouched, as in d_dst.  d_counts (may be NULL; 8-byte aligned): int64
 *   [OFX_MOSAIC_MAX_SOURCES + 1]; entry k < S the pixels with k* = k, entries S .. 8 zero, entry 9 the pixels no source covers; the
 *   entries sum to w h; the call zeroes all ten on the stream first.
 * With S = 1 the destination is ofx_warp_perspective's, byte for byte under either border, and entry 9 equals its d_outside.
 * Appending a source never changes a pixel that an earlier source covers.  A seam between two sources is not blended.
 *
 * ofx_warp_mosaic: 1 <= n <= OFX_STREAM_MAX_BATCH items of any sizes, channels, borders and source counts in ONE launch (plus the
 * memsets of the counts).  Pitches, alignment and the untouched tail of a row are ofx_warp_affine's; no tap reads outside a source,
 * whether it covers the pixel or not.  The descriptors embed everything: no host pointer has to stay alive.  Sources k >= S are not
 * looked at.  Refused with OFX_E_INVALID and a message naming the call, the item and, for a source, the source, before anything is
 * enqueued: null items, n, n_sources outside 1 .. 9, a null d_src among the first S or a null d_dst, channels, border, fill, a size
 * or a model entry outside its range, a pitch below its row (which_pitch included, when d_which is given), a source that overlaps
 * d_dst or d_which, d_which overlapping d_dst, d_counts not 8-byte aligned. */
#define OFX_MOSAIC_MAX_SOURCES 9
typedef struct ofx_mosaic_source {
    const uint8_t *d_src;
    int src_pitch, sw, sh;
    double model[9];
} ofx_mosaic_source;
typedef struct ofx_mosaic_desc {
    ofx_mosaic_source source[OFX_MOSAIC_MAX_SOURCES];
    int n_sources;
    uint8_t *d_dst;
    int dst_pitch, w, h;
    int channels, border, fill;
    uint8_t *d_which; /* may be NULL */
    int which_pitch;
    int64_t *d_counts; /* may be NULL */
} ofx_mosaic_desc;
int ofx_warp_mosaic(const ofx_mosaic_desc *items, int n, void *stream);

/* ---- temporal noise filter -----------------------------------------------------------
 * Every other consumer of a displacement field makes new frames from it or judges the motion.  This one improves the frames the
 * motion was measured on: a pixel is averaged with the pixels that show the same scene point in its neighbouring frames, each
 * neighbour weighted per pixel by how well its 3 x 3 surroundings agree with the centre's (the patch test), because an average
 * along a wrong vector is worse than no filter.  THE definition (tests/temporal_ref.py restates it in NumPy); after one float32
 * product and one rounding per component it is all integers:
 *
 * INPUTS: a centre plane c of w x h pixels, u8, `channels` C in {1, 3} interleaved, pitch >= C w, any alignment; n_neighbours S in
 *   1 .. OFX_TEMPORAL_MAX_NEIGHBOURS neighbours, neighbour k a plane n_k of the same w, h and C with a pitch of its own and a field
 *   D_k: interleaved float32 (u, v), w x h, tightly packed, 8-byte aligned, IN PIXELS, on c's grid -- neighbour k at x + D_k(x) shows
 *   what c shows at x: "pixel displacement" of the pair c -> n_k.  weights: uint16 [256] on the host, every entry <= 256, copied
 *   into the launch; centre_weight wc in 1 .. 256.  A neighbour plane may be c itself or the plane of another neighbour; nothing
 *   may overlap the destination.
 * POSITION of neighbour k for pixel (x, y), with (u, v) = D_k(y, x): DEFINED when u and v are finite and |u|, |v| <= 1048576.0f (a
 *   NaN fails).  qx = 32 x + (int64) rintf(32.0f * u), ties to even; qy likewise.  The product is an exact scaling, and a denormal
 *   rounds to 0 whether it is kept or flushed: the definition does not depend on the denormal mode.  USABLE when defined and
 *   0 <= qx <= 32 (w - 1) and 0 <= qy <= 32 (h - 1).
 * PATCH     for (i, j) in {-1, 0, 1}^2 the neighbour's patch value N_k(i, j, ch) is VALUE of "affine frame warp" at the position
 *   (clamp(qx + 32 i, 0, 32 (w - 1)), clamp(qy + 32 j, 0, 32 (h - 1))); where nothing clamps, the fraction is the same for all nine,
 *   so they need 4 x 4 taps.  The centre's patch is c(clamp(x + i, 0, w - 1), clamp(y + j, 0, h - 1), ch).  SAD_k = sum |N_k - c|
 *   over the 9 C values;  m_k = min(255, (SAD_k + 4) / 9) for C = 1 and min(255, (SAD_k + 13) / 27) for C = 3, integer division:
 *   the rounded mean absolute difference.  w_k = weights[m_k] when the neighbour is usable at this pixel, else 0.
 * VALUE     per channel  num = wc c + sum_k w_k N_k(0, 0, ch);  den = wc + sum_k w_k;  out = (2 num + den) / (2 den), integer
 *   division, exact; den <= 1280, so it all fits 32 bits.  The geometry, the SADs and the weights are formed once per pixel and
 *   applied to every channel.
 * STATS     d_stats (may be NULL; 8-byte aligned): int64 [8], zeroed by the call on the stream first.  [0] w h;  [1 + k] pixels
 *   where neighbour k is not usable (0 for k >= S);  [5] pixels with sum_k w_k = 0 (the output is c);  [6] sum |out - c| over pixels
 *   and channels;  [7] sum over pixels of sum_k w_k.  Integers: they depend on no order, tile or batch.
 * Consequences: all-zero weights give a copy of c, byte for byte; zero fields with n_k = c give c; a whole-pixel field makes
 * N_k(0, 0) a shifted copy of n_k exactly; appending a neighbour whose weight is 0 everywhere changes nothing but [1 + k]; no tap
 * reads outside the (h - 1) pitch + C w bytes of a plane or the w h 8 bytes of a field, whatever the fields hold; the bytes of a
 * destination row beyond column C w - 1 stay untouched.
 * Not here: a reach above one frame per field -- a neighbour two frames away takes a composed field, which "displacement chain"
 * below makes (engine.denoise_rings(reach=2) feeds all four slots that way); a recursive filter; planar colour.
 *
 * ofx_temporal_filter: 1 <= n <= OFX_STREAM_MAX_BATCH items of any sizes, channel counts and neighbour counts in ONE launch, behind
 * the launches of the library's own kernel that zero the stats on the same stream: one per item that gave d_stats, no memset
 * (Conventions: a call records kernel nodes only).  The descriptors embed everything: no host pointer has to stay alive.
 * Neighbours k >= S are not looked at.  Refused with OFX_E_INVALID and a message naming the call, the item and, for a neighbour,
 * the neighbour, before anything is enqueued: null items or prm; n out of range, n_neighbours outside 1 .. 4; a null plane or field
 * among the first S, a null d_centre or d_dst; channels not 1 or 3; w or h outside 1 .. 2^16, w h >= 2^28, a plane of 2^31 bytes or
 * more; a pitch below its row; a field or d_stats not 8-byte aligned; a weight above 256, centre_weight outside 1 .. 256, a
 * non-zero reserved word; d_dst overlapping any input plane, field or d_stats. */
#define OFX_TEMPORAL_MAX_NEIGHBOURS 4
typedef struct ofx_temporal_neighbour {
    const uint8_t *d_plane;
    int pitch, pad;
    const float *d_field;
} ofx_temporal_neighbour;
typedef struct ofx_temporal_desc {
    ofx_temporal_neighbour neighbour[OFX_TEMPORAL_MAX_NEIGHBOURS];
    int n_neighbours;
    int w, h, channels;
    const uint8_t *d_centre;
    int centre_pitch, dst_pitch;
    uint8_t *d_dst;
    int64_t *d_stats; /* may be NULL */
} ofx_temporal_desc;
typedef struct ofx_temporal_params {
    uint16_t weights[256];
    int centre_weight;
    int reserved; /* 0 */
} ofx_temporal_params;
int ofx_temporal_filter(const ofx_temporal_desc *items, int n, const ofx_temporal_params *prm, void *stream);

/* ---- displacement chain -----------------------------------------------------------------
 * Every producer of a displacement field here gives the field of two CONSECUTIVE frames, and every consumer takes "a field in
 * pixels on the first frame's grid".  This is the operator between them for frames that are further apart: the concatenation of
 * two fields, D_ac(x) = D_ab(x) + D_bc(x + D_ab(x)) -- follow the first vector, read the second field bilinearly there, add --
 * folded over up to OFX_CHAIN_MAX_LINKS fields.  It has the gather of "forward-backward consistency", but it writes a field
 * instead of judging one.  THE definition (tests/chain_ref.py restates it in NumPy):
 *
 * INPUTS: n_links L in 2 .. OFX_CHAIN_MAX_LINKS fields D_0 .. D_{L-1}, each interleaved (u, v) float32, w x h, tightly packed,
 *   8-byte aligned, IN PIXELS: D_j is the displacement of frame j -> frame j + 1 on frame j's grid ("pixel displacement").  All
 *   fields of an item have the same size.
 * Every float32 operation is rounded once, nothing is fused, denormals are kept.
 * STEP   for pixel (x, y): A_0 = D_0(y, x).  For j = 1 .. L - 1, with (u, v) = A_{j-1}:
 *   1. px = (float)x + u, py = (float)y + v.
 *   2. unless |px| <= 1e9 && |py| <= 1e9 (a NaN fails): class 3, UNDEFINED.  Stop.
 *   3. else if px < 0 || px > (float)(w-1) || py < 0 || py > (float)(h-1): class 2, LEAVES -- the path leaves the frame.  Nothing
 *      is clamped and D_j is not read.  Stop.
 *   4. else x0, y0, fx, fy, x1 = min(x0+1, w-1), y1 = min(y0+1, h-1) exactly as in steps 4 and 5 of "forward-backward
 *      consistency": in the last column the right tap IS the pixel itself, whatever lies behind it in memory; likewise in the
 *      last row.  Per component of D_j, with b00 = D_j(y0,x0), b01 = D_j(y0,x1), b10 = D_j(y1,x0), b11 = D_j(y1,x1):
 *        a = b00 + fx*(b01 - b00);  c = b10 + fx*(b11 - b10);  r = a + fy*(c - a)
 *   5. A_j = (u + r_u, v + r_v).  Unless both components satisfy |.| <= FLT_MAX: class 3.  Stop.
 *   A pixel that gets through every link has class 0, OK.
 * OUTPUTS
 *   dst    a float32 field like the inputs: A_{L-1} for class 0.  For classes 2 and 3 BOTH components are the bit pattern
 *          0x7fc00000; the output never holds an Inf or any other NaN.  "temporal noise filter" and "frame interpolation" treat
 *          such a vector as not defined.
 *   mask   (may be absent) u8, rows mask_pitch >= w apart: the class.  Bytes beyond column w - 1 are left untouched.
 *   stats  (may be absent; 8-byte aligned) int64 [4] = [w h, pixels of class 2, of class 3, of class 0], zeroed by the call on the
 *          stream first: a slot needs no initialisation and carries nothing from one call to the next.  Integers: they depend on
 *          no order, tile or batch.
 * Consequences: a chain of L links equals L - 1 two-link calls folded from the left, chain(chain(D_0, D_1), D_2) .., bit for bit,
 * the dead pixels included (a 0x7fc00000 vector fails step 2 and stays what it is); whole-pixel constant fields add exactly
 * wherever the path stays inside; no tap reads outside the w h 8 bytes of a field, whatever the fields hold; an OK vector is finite.
 * In place: d_dst may be exactly d_link[0] -- D_0 is read only at the pixel itself, by the thread that writes it, before the write.
 * Not here: the inverse of a field, and chains of more than OFX_CHAIN_MAX_LINKS links in one call (fold them).
 *
 * ofx_displacement_chain: 1 <= n <= OFX_STREAM_MAX_BATCH items of any sizes and link counts in ONE launch, behind the launches of
 * the library's own kernel that zero the stats on the same stream: one per run of d_stats slots that follow one another in memory
 * in the items' order, no memset (Conventions: a call records kernel nodes only); the slot of an item that gave none is not
 * touched, wherever it lies.  The descriptors embed everything: no host pointer has to stay alive.  Links k >= n_links are not
 * looked at.  Refused with OFX_E_INVALID and a message naming the call, the item and, for a link, the link, before anything is
 * enqueued: null items; n out of range; n_links outside 2 .. 4; a null link among the first L, a null d_dst; w or h < 1, w h >=
 * 2^28; a link, d_dst or d_stats not 8-byte aligned; mask_pitch < w when d_mask is given; within an item, d_dst overlapping a link
 * (other than being exactly link 0), d_mask overlapping a link, and d_dst, d_mask and d_stats overlapping each other. */
#define OFX_CHAIN_MAX_LINKS 4
#define OFX_CHAIN_OK 0
#define OFX_CHAIN_LEAVES 2
#define OFX_CHAIN_UNDEFINED 3
typedef struct ofx_chain_desc {
    const float *d_link[OFX_CHAIN_MAX_LINKS];
    int n_links, w, h, mask_pitch;
    float *d_dst;
    uint8_t *d_mask;  /* may be NULL */
    int64_t *d_stats; /* may be NULL; 4 values, overwritten */
} ofx_chain_desc;
int ofx_displacement_chain(const ofx_chain_desc *items, int n, void *stream);

/* ---- layout helpers ------------------------------------------------------ */
int ofx_extract_ch0(const uint8_t *d_src3, uint8_t *d_dst1, int w, int h, int dst_pitch, void *stream);
int ofx_replicate_3ch(const uint8_t *d_src1, int src_pitch, uint8_t *d_dst3, int w, int h, void *stream);

/* ---- API-compat primitives, device-resident -------------------------------
 * Generic (any mask / window size) counterparts of the reference kernels that
 * the flow path does not use in fused form. */
/* gpu::grayscale_avg, OptFlowGpu.cu:47-60 */
int ofx_grayscale_avg_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int w, int h, void *stream);
/* gpu::conv_3ch_2d / _constant, OptFlowGpu.cu:108-147 (int accumulators, per-tap truncation) */
int ofx_conv_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int w, int h, const float *h_mask, int mw, int mh,
                 int float_acc, void *stream);
/* gpu::conv_3ch_1ch_constant / _tiled, OptFlowGpu.cu:380-425 */
int ofx_conv_3ch_1ch_u8(const uint8_t *d_src3, int w, int h, uint8_t *d_dst, const float *h_mask, int mw, int mh,
                        void *stream);
/* gpu::conv_3ch_1ch_tiled_uchar_float, OptFlowGpu.cu:1040-1090 */
int ofx_conv_3ch_1ch_f32(const uint8_t *d_src3, int w, int h, float *d_dst, const float *h_mask, int mw, int mh,
                         void *stream);
/* gpu::gauss_pyramid one level on 3ch images, OptFlowGpu.cu:1198-1232 (mask fixed to GAUS_KERNEL_3x3) */
int ofx_downsample_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int dw, int dh, void *stream);
/* gpu::srm_1ch, OptFlowGpu.cu:1463-1502 */
int ofx_srm_u8(const uint8_t *d_a, const uint8_t *d_b, int w, int h, int ww, int wh, int32_t *d_dst, void *stream);
/* gpu::srm_1ch_float, OptFlowGpu.cu:1549-1588 (row-major float accumulation) */
int ofx_srm_f32(const float *d_a, const float *d_b, int w, int h, int ww, int wh, float *d_dst, void *stream);
/* gpu::inverse_matrix, OptFlowGpu.cu:1727-1755 */
int ofx_solve_i32(const int32_t *d_sxx, const int32_t *d_syy, const int32_t *d_sxy, const int32_t *d_sxt,
                  const int32_t *d_syt, float *d_flow, int w, int h, int variant, void *stream);
/* gpu::inverse_matrix_float, OptFlowGpu.cu:1819-1846 */
int ofx_solve_f32(const float *d_sxx, const float *d_syy, const float *d_sxy, const float *d_sxt,
                  const float *d_syt, float *d_flow, int w, int h, void *stream);
/* solve variants for ofx_solve_i32 */
#define OFX_SOLVE_F64 0        /* OptFlowGpu.cu:1737-1754, double, correct */
#define OFX_SOLVE_INLINE_CPU 1 /* OptFlowCPU.cpp:369-382, double, c unscaled */
#define OFX_SOLVE_F32 2        /* OptFlowCPU.cpp:293-304, float */
/* utils::generate_gaussian_kernel, OptFlowUtils.cpp:68-114 (host arithmetic, double; dst holds ks*ks values,
 * (ks+1)^2 when ks is even, 2*pi*sigma rounded when ks == -1) */
void ofx_generate_gaussian_kernel(double sigma_s, int kernel_size, double *h_dst);
/* gpu::bilinear_filter (a bilateral filter), OptFlowGpu.cu:1984-2048 */
int ofx_bilateral_3ch(const uint8_t *d_src3, const uint8_t *d_gray3, uint8_t *d_dst3, int w, int h, int ww, int wh,
                      double sigma_s, double sigma_b, void *stream);

/* The same filter within SURVEY 8c's tolerance for this stage (+-1 LSB of the reference's byte), several times faster: float
 * accumulators, the range weight evaluated (v_exp_f32) instead of looked up, the quotient formed around the centre value for
 * grey images.  Odd ww <= 13, odd wh <= ww.  Opt-in: ofx_bilateral_3ch stays the bit-exact kernel. */
int ofx_bilateral_3ch_fast(const uint8_t *d_src3, const uint8_t *d_gray3, uint8_t *d_dst3, int w, int h, int ww, int wh,
                           double sigma_s, double sigma_b, void *stream);
/* gpu::bilinear_filter / cpu::bilinear_filter_3ch have the reference's signatures and carry no mode: this process-wide switch
 * makes them run ofx_bilateral_3ch_fast (on != 0) or the bit-exact kernel (on == 0, the default; environment
 * OFX_BILATERAL_FAST=1 starts with it on).  on < 0 only queries.  Returns the previous setting. */
int ofx_bilateral_wrappers_fast(int on);
/* The stream pipeline's colour front end as a batched call: main.cu:222-240 -- grayscale_avg, then the bilateral pre-filter with
 * the grey image as its own source (square odd window 3 .. 13: ofx_bilateral_3ch(g, g, ...) of the grey image) -- for n <=
 * OFX_STREAM_MAX_BATCH colour frames in ONE launch, each written as a one-channel plane.  Frame i: d_src3[i] interleaved 3-channel
 * u8 (channel order does not matter), 4-byte aligned, row pitch src_pitches[i] >= 3 * w bytes (tightly packed odd widths
 * included); d_dst[i] one-channel u8, row pitch dst_pitches[i] >= w, of which columns [0, w) of every row are written (either
 * pitch array may be NULL when every frame's pitch is src_pitch0 / dst_pitch0).  Per frame (modes[i], or mode0 for all when
 * modes is NULL):
 *   OFX_FRONTEND_GREY            (c0 + c1 + c2) / 3 in integers (ofx_grayscale_avg_3ch's value)
 *   OFX_FRONTEND_BILATERAL       then the bit-exact filter (= ofx_bilateral_3ch of that grey image as its own source, channel 0)
 *   OFX_FRONTEND_BILATERAL_FAST  then the +-1 LSB filter (ofx_bilateral_3ch_fast's float arithmetic; the exact one where that
 *                                does not apply: sigma_b > 2e4)
 * window / sigma_s / sigma_b are ignored when every frame is GREY; an unsupported window is OFX_E_UNSUPPORTED.  A call that mixes
 * BILATERAL and BILATERAL_FAST frames launches twice.  The tables are built on the host when (window, sigma_s, sigma_b) changes. */
#define OFX_FRONTEND_OFF 0
#define OFX_FRONTEND_GREY 1
#define OFX_FRONTEND_BILATERAL 2
#define OFX_FRONTEND_BILATERAL_FAST 3
int ofx_frontend_1ch(const uint8_t *const *d_src3, const int *src_pitches, int src_pitch0, uint8_t *const *d_dst, const int *dst_pitches,
                     int dst_pitch0, int n, int w, int h, const int *modes, int mode0, int window, double sigma_s, double sigma_b,
                     void *stream);

/* the remaining functions of namespace cpu (OptFlowCpu.hpp:3-184), device-resident, so that the cpu:: call surface of
 * include/OptFlowCpu.hpp runs on the MI355X as well */
/* cpu::sub_arr, OptFlowCPU.cpp:11-17 (bytes, wrapping) */
int ofx_sub_u8(const uint8_t *d_a, const uint8_t *d_b, size_t n, uint8_t *d_dst, void *stream);
/* cpu::srm_3ch, OptFlowCPU.cpp:202-238 (bounds test `>` as there; taps past the end of the buffer contribute nothing) */
int ofx_srm_3ch_u8(const uint8_t *d_a3, const uint8_t *d_b3, int w, int h, int ww, int wh, int32_t *d_dst3, void *stream);
/* cpu::downscale_gaussian, OptFlowCPU.cpp:112-148: one pyramid level on 3ch images with the CALLER's mask (<= 81 taps) */
int ofx_downscale_mask_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int dw, int dh, const float *h_mask, int mw, int mh, void *stream);
/* cpu::shift_back_pyramid on the 3ch image, OptFlowCPU.cpp:241-282: d_dst3 keeps its contents except for its first w*h bytes
 * (copied from d_src3) and the pixels whose shifted target lies inside the image */
int ofx_shift_3ch(const uint8_t *d_src3, uint8_t *d_dst3, int w, int h, const float *d_uv, void *stream);

/* ---- session: device-resident pyramids for a stream of frames -------------
 * Mirrors main.cu:192-272: the previous frame's pyramid is kept, each new
 * frame gets its pyramid built and every level is solved coarse to fine. */
typedef struct ofx_session ofx_session;

typedef struct ofx_params {
    int width, height; /* level-0 size; (width>>k, height>>k) must be even for k < levels-1 */
    int levels;        /* 1..OFX_MAX_LEVELS (main.cu:192 uses 4) */
    int window;        /* reference: 9 (CPU, OptFlowCPU.cpp:344) / 19 (GPU, OptFlowGpu.cu:1944) */
    int mode;          /* OFX_MODE_* */
    int device;        /* HIP device ordinal */
    /* Row sharding.  sharded == 0: this session holds whole levels.  sharded != 0: for level k this
     * rank OWNS global rows [own_y0[k], own_y1[k]) -- it computes the pyramid and the flow for them -- and its
     * plane buffers HOLD rows [buf_y0[k], buf_y1[k]) (own rows plus halo; the halo rows are filled by the
     * caller's exchange between ofx_session_downsample_level and ofx_session_run_levels, or recomputed: comp_y*). */
    int sharded;
    int own_y0[OFX_MAX_LEVELS], own_y1[OFX_MAX_LEVELS];
    int buf_y0[OFX_MAX_LEVELS], buf_y1[OFX_MAX_LEVELS];
    /* rows of level k (k >= 1) this rank produces itself when it builds the pyramid, own <= comp <= buf.
     * comp == own: halos come from the neighbours (exchange); comp == buf: halos are recomputed locally from a
     * wider halo one level below (no exchange).  Ignored (treated as own) when comp_y1[k] == 0. */
    int comp_y0[OFX_MAX_LEVELS], comp_y1[OFX_MAX_LEVELS];
    /* refinement iterations per level (extension, lk_float only): 0 or 1 = the reference (no refinement).  Unsharded
     * sessions run them pair at a time (ofx_session_run_flow) or through the stream pipeline (one warp + one accumulating LK
     * launch per iteration for all pairs of a tick); sharded sessions through the stream pipeline only (local_corner), with
     * buf_y* holding own rows +- ((window/2 + 1) * iters + slack for the shift and the warp): parallel.ShardPlan(iters=...). */
    int iters;
    /* Sharded sessions: compute the corner flows (the reference's shift vectors, formed from pixel 0 of every coarser
     * flow level) LOCALLY from a small top-left patch of every frame instead of receiving them from the rank that owns
     * row 0.  Every frame handed to the session is the whole frame, so the patch is always at hand; with it a rank
     * needs nothing from any other rank and can run the one-launch-per-frame stream pipeline
     * (ofx_session_stream_*).  patch_size: level-0 side of the square patch, 0 = automatic
     * (2^(levels-1) * (window/2 + 2 + 8), at least 256, clipped to the frame).  With borrow_frames the shift is exact for
     * every input (a shifted corner that leaves the patch is read through a relocated one, ofx_corner_stage.d_patch_reloc);
     * with copied frames it is exact while it stays inside the patch and ofx_session_corner_status reports when it did not. */
    int local_corner;
    int patch_size;
    /* frames per tick of the stream pipeline: 0 or 1 = one launch per frame, 2 .. 16 = one launch per that many frames
     * (see ofx_session_stream_submit); stream_batch * levels <= OFX_MAX_LK_ITEMS. */
    int stream_batch;
    /* Stream pipeline without its own copy of level 0: the LK and corner stages read level 0 straight from the frame
     * buffers handed to ofx_session_stream_submit, and the pyramid stage only writes levels 1 and up.
     * LIFETIME RULE (the one statement of it; INTEGRATION.md, DESIGN.md and engine.py quote it): the buffer of frame f
     * (frames counted from 0, B = stream_batch) is last read by the launch that the submit of frame f + dB enqueues, at the
     * latest, where d = 3, or 2 with stream_two_stage (below).  It may be rewritten (a) by work enqueued on the SAME stream after that submit call, or (b) from the host or
     * another stream once that launch has COMPLETED -- the submit call returning is not enough.  A producer that writes
     * frame g into its buffer on the stream, right before submitting it, therefore needs a ring of at least dB + 1
     * buffers; one that writes asynchronously needs as many more as it has launches in flight.
     * Saves 2 bytes per level-0 pixel of HBM traffic per frame and a third of the pipeline's cache working set
     * (DESIGN.md section 4.3).  0 = copy (any buffer lifetime).
     * Pair-at-a-time path (ofx_session_set_frame_device + build_pyramid + run_flow + swap): the flag makes
     * ofx_session_set_frame_device remember the buffer instead of copying it (no copy launch; the pyramid, corner and LK
     * launches read it in place).  There the buffer of a frame is read until the run_flow of the pair in which it is the
     * PREVIOUS frame has run, and its pitch must be the session's level-0 pitch (the width rounded up to 64 bytes,
     * ofx_session_plane reports it) at a 4-byte aligned address; host frames (ofx_session_set_frame_host*) and the staged
     * path still copy.  A single-level session with refinement iterations (levels == 1, iters > 1) copies its frames whatever
     * this flag says (pair at a time: the stream pipeline needs two levels): its level 0 would be the fused warp's source, which must be followed by three
     * readable bytes (ofx_lk_desc.d_warp_src). */
    int borrow_frames;
    /* determinant guard of the solve, see ofx_lk_desc.min_det (0 = the reference: flat regions are NaN) */
    float min_det;
    /* Stream pipeline in TWO stages instead of three: a tick runs pyramid(its frames) | corner(the pairs its frames complete)
     * | LK(the pairs of the tick before), the corner stage building the two small patch pyramids it needs itself
     * (ofx_corner_stage.build_patch) instead of waiting a tick for the pyramid stage.  A pair's flow is complete one tick
     * earlier, the pipeline holds 2B + 2 image sets instead of 3B + 2 and a borrowed frame f is read until the launch
     * enqueued by the submit of frame f + 2B (ring of >= 2B + 1 buffers) -- which is what lets eight 4K frames per launch
     * stay inside the Infinity Cache.  Needs borrow_frames.  The shift vectors are exact for EVERY input: a shifted corner that
     * leaves the patch (256 level-0 pixels or patch_size) is read through a patch pyramid the corner block rebuilds around it
     * (ofx_corner_stage.d_patch_reloc; ofx_session_pair_status says for which pairs that happened). */
    int stream_two_stage;
    /* The frame buffers handed to this (sharded, local_corner) session are PARTIAL: only the level-0 rows the plan holds
     * (buf_y0[0] .. buf_y1[0]) and the frame's top-left patch were ever written; every other byte is undefined (the ranks of
     * parallel.ShardedFlow's "stream_exchange" mode only ever receive those).  The corner chain then reads level 0 through the
     * patch's extent only and the repair of a shift that leaves the patch is OFF (it would rebuild from rows that are not
     * there): such a pair raises bit k of the status word, as with copied frames, and is an error.  Not with stream_two_stage. */
    int frames_partial;
    /* Where the stream tick's LK stage expects its image rows to come from (ABI v10).  0 = decide by the size of the largest level
     * (levels of 16 Mpx and more: deep fetch); +1 = the frames handed over are COLD -- they were last touched more than an
     * Infinity Cache (256 MiB) of traffic ago, e.g. a long pool of decoded surfaces that is consumed much later than it is
     * written: fetch rows two steps ahead straight into LDS (ofx_stream_stages.deep_fetch; measured on MI355X with a ring of 44
     * 4K frames: 272.8 vs 287.2 us per tick of eight pairs, 1080p 137.8 vs 142.8); -1 = they are warm (just written by a producer, or a
     * short ring): fetch one step ahead (2 % faster then).  A hint about speed only: every choice gives the same bits. */
    int deep_fetch;
} ofx_params;

int ofx_session_create(const ofx_params *p, ofx_session **out);
/* Sharded sessions: *h_status receives (and the session clears) the OR over all pairs so far of bit k = "level k's shift left
 * the top-left patch" (local_corner), bit 8 + k = "level k's vertical shift reached image rows beyond this shard's halo" (the
 * margin rows of the plan) and bit 16 + k = "a refinement iteration's warp at level k reached beyond the halo" (iters > 1);
 * 0 = every pair so far is exactly the unsharded result.  Synchronises `stream`. */
int ofx_session_corner_status(ofx_session *s, int *h_status, void *stream);
/* The same word for ONE pair of the stream pipeline (frames counted from 0, pair p = frame p-1 -> frame p), while it is one of
 * the newest 2 * stream_batch pairs whose corner stage has run: the bits that pair raised, plus OFX_STATUS_REPAIRED when its
 * shifted corner left the top-left patch and was read through a relocated one (informational: the flow is the reference's).
 * With the repair in place (stream_two_stage, or local_corner with borrow_frames and whole frames: not frames_partial) bit k can
 * no longer occur; bits 8 + k and
 * 16 + k (a shard's halo) stay errors.  Synchronises `stream`; does not clear anything. */
int ofx_session_pair_status(ofx_session *s, int pair, int *h_status, void *stream);
int ofx_session_destroy(ofx_session *s);
/* Load the NEXT frame's level 0 (1ch, tightly packed w bytes per row, full frame) from host / device memory. */
int ofx_session_set_frame_host(ofx_session *s, const uint8_t *h_gray1, void *stream);
int ofx_session_set_frame_host_3ch(ofx_session *s, const uint8_t *h_img3, void *stream);
int ofx_session_set_frame_device(ofx_session *s, const uint8_t *d_gray1, int pitch, void *stream);
/* Build the next frame's pyramid (gpu::gauss_pyramid, main.cu:250): ofx_session_downsample_level for k = 1..levels-1. */
int ofx_session_build_pyramid(ofx_session *s, void *stream);
/* Level k of the next frame's pyramid from level k-1, own rows only. */
int ofx_session_downsample_level(ofx_session *s, int level, void *stream);
/* All levels against the previous frame's pyramid (main.cu:256-262) in three launches: ofx_session_corner_flows,
 * then ofx_session_run_levels (one multi-level shift launch, one multi-level LK launch).
 * Capturing a session's pair: on the plain single-stream path (no shard, no borrowed frames, timing not armed) the sequence
 * set_frame_device, build_pyramid, swap, set_frame_device, build_pyramid, run_flow may be recorded into one graph on `stream`,
 * with refinement iterations as well, AFTER one such pair has run live: a session makes the packed plan of a launch shape with
 * an allocation and a blocking copy the first time it meets the shape, which a capture does not allow.  The host state (which
 * image set is `prev`, what has been loaded) is consulted and changed when the calls are made, not at a replay: the graph holds
 * the addresses of the capture, reads the two frame buffers anew at every replay and leaves the flow where ofx_session_flow
 * pointed when it was recorded.  Not covered, and not to be captured: the staged path with its aux stream
 * (ofx_session_stage_frame .. solve_staged), the stream pipeline (ofx_session_stream_*), and whatever returns data to the host
 * (Conventions). */
int ofx_session_run_flow(ofx_session *s, void *stream);
int ofx_session_corner_flows(ofx_session *s, void *stream);
int ofx_session_run_levels(ofx_session *s, void *stream);
/* The pair's DENSE flow of "coarse-to-fine propagation" above, in ofx_session_run_flow's place in the call sequence (set frame,
 * build pyramid, THIS, swap); results through ofx_session_flow(s, k), iters = ofx_params.iters (0 counts as 1), min_det =
 * ofx_params.min_det.  max_px: the definition's, in pixels of the COARSE level (0 = off; the window size is the usual choice: a
 * vector the level above could not have measured starts the level below from nothing instead).  The top level runs as in
 * ofx_session_run_flow; then per level, coarse to fine, one ofx_flow_prolong (timing kind OFX_TIME_WARP) and iters single-level
 * accumulating ofx_lk_levels launches, all but the last of which also write the next warped image.  The warped images alternate
 * between the level's two shifted-scratch planes, which nothing shifts here; the levels depend on each other, so a pair takes
 * (levels - 1) * (iters + 1) launches below its top level.  Never allocates, never synchronises.
 * Unsharded lk_float / lk_float_fast sessions that copy their frames: OFX_E_UNSUPPORTED for a sharded session, compat_cpu and
 * borrow_frames (level 0 of the next frame would be the warp source, and a caller's buffer need not be followed by the three
 * readable bytes of ofx_lk_desc.d_warp_src).  OFX_E_STATE without a previous and a next frame; max_px negative or not finite:
 * OFX_E_INVALID. */
int ofx_session_run_flow_dense(ofx_session *s, float max_px, void *stream);
/* "A pair's dense flow with median" of the block "flow median" above, in ofx_session_run_flow_dense's place: the same calls, and one
 * ofx_flow_median (radius 1 or 2; timing kind OFX_TIME_WARP) after the top level and after every accumulating launch below it.  A
 * median is out of place, so a level's flow alternates between the session's flow plane and d_scratch: a second flow pyramid that
 * the CALLER owns, like the output rings (level k at the sum of the sizes of the levels below it, w_k * h_k * 8 bytes each;
 * ofx_session_dense_median_scratch_bytes tells the total; 8-byte aligned).  Below the top level the accumulating launches write no
 * warped image: all but the last median of a level write it, from the filtered vectors, into the level's other shifted-scratch
 * plane.  Afterwards ofx_session_flow(s, k) holds the filtered flow of every level, whatever iters is (a level starts in the buffer
 * that makes its last median end in the session's plane; the top level's one median is copied back).  Never allocates, never
 * synchronises; the scratch holds nothing the next call needs.  Refusals: ofx_session_run_flow_dense's, and OFX_E_INVALID for a
 * radius other than 1 or 2 and a scratch that is null, not 8-byte aligned or smaller than the total. */
int ofx_session_run_flow_dense_median(ofx_session *s, float max_px, int radius, void *d_scratch, size_t scratch_bytes, void *stream);
int ofx_session_dense_median_scratch_bytes(ofx_session *s, size_t *bytes);
/* The same result the reference's way: per level ofx_session_compute_uv then ofx_session_run_level, coarse to fine. */
int ofx_session_run_flow_sequential(ofx_session *s, void *stream);
/* Shift vector of `level` from the coarser flows' pixel 0 into the session's uv slot (meaningful on the rank that
 * owns row 0; a sharded driver broadcasts the slot before ofx_session_run_level). */
int ofx_session_compute_uv(ofx_session *s, int level, void *stream);
/* Shift (below the top level) + fused LK of one level, own rows, using the uv slot as it stands. */
int ofx_session_run_level(ofx_session *s, int level, void *stream);
/* Pipelined pair (throughput path): the staging half of a pair -- frame load, pyramid, corner flows, shifts -- runs on
 * a session-owned auxiliary stream underneath the previous pair's LK launch; the solve half runs on `stream`.
 * ofx_session_submit_device does a whole pair and leaves the new frame as the previous one; results are bit-identical
 * to set_frame_device + build_pyramid + run_flow + swap.  d_gray1 must be complete in HBM at the call.
 * A sharded driver issues the halves itself: stage_frame; corner_flows (rank holding row 0) and the broadcast of the
 * shift vectors on the aux stream (ofx_session_aux_stream); stage_shift; solve_staged. */
int ofx_session_submit_device(ofx_session *s, const uint8_t *d_gray1, int pitch, void *stream);
int ofx_session_stage_frame(ofx_session *s, const uint8_t *d_gray1, int pitch, void *aux_stream);
int ofx_session_stage_shift(ofx_session *s, void *aux_stream);
int ofx_session_solve_staged(ofx_session *s, void *stream);
int ofx_session_aux_stream(ofx_session *s, void **stream);
/* Stream pipeline (highest throughput): ONE launch (ofx_stream_launch) per tick of B = ofx_params.stream_batch frames
 * (1 .. 16), in which the pyramids of those frames, the corner flows of the B pairs before and the fused LK (shift
 * included) of the B pairs before that run side by side.  With B = 1 every call launches and the flow of pair p (frame
 * p-1 -> frame p, frames counted from 0) is written by the launch of frame p+2.  (ofx_params.stream_two_stage: the corner
 * flows of the pairs the tick's own frames complete, the LK of the B pairs before -- everything one tick earlier.)  With B > 1 only every B-th call launches,
 * for the B frames received since the last launch (the others are remembered: their buffers must stay unmodified until
 * that launching call has returned); pairs complete B at a time, one tick later.  *completed_pair receives the HIGHEST
 * pair complete after the call in `stream` order (all lower ones are complete too; -1 when the call completed none); the
 * flows of the newest B pairs are at ofx_session_flow_of.  After the last frame call ofx_session_stream_drain until it
 * reports -2.  Results are bit-identical to the pair-at-a-time paths.  A frame buffer must stay valid until the launch
 * that received it has finished. */
int ofx_session_stream_begin(ofx_session *s);
int ofx_session_stream_submit(ofx_session *s, const uint8_t *d_gray1, int pitch, void *stream, int *completed_pair);
int ofx_session_stream_drain(ofx_session *s, void *stream, int *completed_pair);
/* The same for n consecutive frames in one call (n >= 1; pitches may be NULL when every frame's pitch is `pitch0`): exactly
 * what n calls of ofx_session_stream_submit do, for callers whose frames arrive in groups or whose call overhead counts
 * (an FFI call per frame is ~1.5 us; a rank of an 8-way sharded 4K pair spends ~5 us of GPU time per frame). */
int ofx_session_stream_submit_frames(ofx_session *s, const uint8_t *const *d_gray1, const int *pitches, int pitch0, int n, void *stream,
                                     int *completed_pair);
/* Flow of `pair` at `level` while it is one of the newest stream_batch completed pairs of the stream pipeline (pair p
 * lives in flow set p mod stream_batch).  Same outputs as ofx_session_flow. */
int ofx_session_flow_of(ofx_session *s, int pair, int level, float **d_ptr, int *row0, int *rows);
/* Composed dense flow (main.cu:138-147, = ofx_compose_flow at `level`, bit for bit) of every pair the stream pipeline
 * completes, written by the pipeline into a caller-owned ring: pair p (frames counted from 0, pair p = frame p-1 -> frame p)
 * goes to slot (p - 1) mod n_slots at d_ring + slot * slot_stride_bytes, rows x (width >> level) x 2 floats, tightly packed
 * (rows = the level's own rows, as ofx_session_flow_of reports them; a sharded session composes its own rows, and is refused
 * with OFX_E_UNSUPPORTED when they would read coarse rows it does not own).  Every call of ofx_session_stream_submit /
 * _submit_frames / _drain that completes pairs enqueues ONE more launch on its `stream`, after the call's last launch, that
 * writes the slots of all those pairs (timing kind OFX_TIME_COMPOSE).
 * Lifetime: the slot of pair p is written by the launch that the call reporting p complete enqueues on its `stream`, and
 * overwritten by the launch of pair p + n_slots; reading it on another stream or from the host needs that launch to have
 * completed.  The ring must stay allocated while the pipeline may write it.
 * d_ring 16-byte aligned, slot_stride_bytes a multiple of 16 and at least the slot's size, 0 <= level < levels,
 * n_slots >= stream_batch (the pairs one call completes); otherwise OFX_E_INVALID.  d_ring == NULL turns it off (the default:
 * no launch, no allocation).  Only before the first frame of a stream (before or right after ofx_session_stream_begin);
 * OFX_E_STATE once a stream has frames.  Stays in effect for later streams. */
int ofx_session_stream_compose(ofx_session *s, int level, float *d_ring, size_t slot_stride_bytes, int n_slots);
/* Slot of `pair` while it is one of the newest n_slots pairs composed into the ring; row0 / rows as ofx_session_flow_of.
 * OFX_E_STATE without a ring, OFX_E_INVALID for a pair not (or no longer) in it. */
int ofx_session_composed_of(ofx_session *s, int pair, float **d_ptr, int *row0, int *rows);
/* The stream pipeline's sampled output stage: what ofx_sample_arrows / ofx_advect_points compute, for every pair the pipeline
 * completes, read straight from the pairs' flow pyramids -- no composed ring needed (the ring may be on as well).  Every call of
 * ofx_session_stream_submit / _submit_frames / _drain that completes pairs enqueues ONE more launch on its `stream`, after the
 * call's last launch, for arrows and tracks together (no timing kind records it); with neither set nothing is launched.
 *   arrows: pair p's field (ofx_sample_arrows at `level` with `arrow_res`, main.cu:267 uses 30) goes to slot (p - 1) mod n_slots at
 *     d_ring + slot * slot_stride_bytes, [ny][nx][4] int32 tightly packed.  d_ring 16-byte aligned, slot_stride_bytes a multiple
 *     of 16 and at least ny * nx * 16, n_slots >= stream_batch, arrow_res between 1 and the level's width; otherwise OFX_E_INVALID.
 *     Lifetime of a slot: as the compose ring's.
 *   tracks: the caller's points (d_points, n_points x (x, y) float32 in pixels of `level`, 8-byte aligned) and statuses (d_status,
 *     int32, 0 = alive) are advected through the completed pairs in increasing order (ofx_advect_points with pair = p: a lost point's
 *     status is the pair that lost it); after the launch that completes pair p they hold the positions in frame p.  The result does
 *     not depend on stream_batch.  The caller owns and initialises both buffers; ofx_session_stream_begin does not touch them.
 *     d_history (may be NULL): slot (p - 1) mod n_slots at d_history + slot * slot_stride_bytes receives all n_points positions
 *     after pair p, frozen ones included; 16-byte aligned, stride a multiple of 16 and at least n_points * 8, n_slots >= stream_batch.
 * d_ring == NULL / d_points == NULL turns that output off (the default).  Only before the first frame of a stream (OFX_E_STATE once
 * a stream has frames); stays in effect for later streams, whose pairs count from 1 again.  Sharded sessions: OFX_E_UNSUPPORTED
 * (points cross shard boundaries). */
int ofx_session_stream_arrows(ofx_session *s, int level, int arrow_res, int32_t *d_ring, size_t slot_stride_bytes, int n_slots);
/* Slot of `pair` while it is one of the newest n_slots pairs sampled into the arrow ring, and the grid's size.  OFX_E_STATE
 * without a ring, OFX_E_INVALID for a pair not (or no longer) in it. */
int ofx_session_arrows_of(ofx_session *s, int pair, int32_t **d_ptr, int *ny, int *nx);
int ofx_session_stream_tracks(ofx_session *s, int level, float *d_points, int32_t *d_status, int n_points, float *d_history,
                              size_t slot_stride_bytes, int n_slots);
/* The stream pipeline's motion-compensation stage: mc and stats of "motion compensation" above, at `level` with `scale`
 * (OFX_ITER_SCALE for the session's own flows), for every pair the pipeline completes.  Pair p's image goes to slot
 * (p - 1) mod n_slots at d_ring + slot * slot_stride_bytes, rows x row_pitch bytes (the bytes of a row beyond the level's
 * width are left untouched), its four int64 to d_stats_ring + 4 * slot.  Every call of ofx_session_stream_submit /
 * _submit_frames / _drain that completes pairs enqueues ONE more kernel launch on its `stream` for all those pairs, after the
 * compose ring's and the sampled stage's (preceded by the memset that zeroes the pairs' stats slots; no timing kind records
 * it).
 *   row_pitch a multiple of 4 and >= the level's width, d_ring 16-byte aligned, slot_stride_bytes a multiple of 16 and at
 *   least rows * row_pitch, n_slots >= stream_batch, d_stats_ring 8-byte aligned, 0 <= level < levels; otherwise OFX_E_INVALID.
 *   d_ring or d_stats_ring may be NULL on its own: image only, or stats only (which moves one byte per pixel less).  Both
 *   NULL turns the stage off (the default: nothing is launched or allocated).
 * Only before the first frame of a stream (OFX_E_STATE once a stream has frames); stays in effect for later streams, whose
 * pairs count from 1 again.  Sharded sessions and frames_partial: OFX_E_UNSUPPORTED (a warp crosses shard rows).
 * Sources: the launch reads, for pair p, level `level` of frames p - 1 and p as the LK stage saw them (each with the pitch it was
 * submitted with: the borrowed level-0 frames of ONE stream must share a pitch, a later stream may bring another), the pair's shift vector of that level (none at the coarsest) and the flow
 * ofx_session_flow_of points to.  All of them are intact in the call that completes the pair: that call's own LK stage reads
 * both image sets and the pair's shift-vector slot, a set is rewritten 3B + 2 (two stages: 2B + 2) frames later and a slot
 * by the corner stage of a later tick, and the last launch of a tick always leaves the final flow in the set flow_of reports.
 * LIFETIME of borrowed frames: unchanged.  Frames p - 1 and p are read by the LK launch of the very call that enqueues this
 * one, so frame f is still last read by a launch of the submit of frame f + dB (ofx_params.borrow_frames).
 * Lifetime of a slot: as the compose ring's. */
int ofx_session_stream_motion(ofx_session *s, int level, float scale, uint8_t *d_ring, int row_pitch, size_t slot_stride_bytes,
                              int n_slots, int64_t *d_stats_ring /* n_slots x 4, may be NULL */);
/* Slot of `pair` while it is one of the newest n_slots pairs of the motion stage: its image (NULL without an image ring) and
 * row pitch, and its four sums (NULL without a stats ring).  OFX_E_STATE without the stage, OFX_E_INVALID for a pair not (or no
 * longer) in the ring. */
int ofx_session_motion_of(ofx_session *s, int pair, uint8_t **d_ptr, int *row_pitch, int64_t **d_stats);
/* The stream pipeline's displacement stage: D of "pixel displacement" above, at `level` with `scale` (OFX_ITER_SCALE for the
 * session's own flows), for every pair the pipeline completes.  Pair p's field (rows x w x 2 floats, tightly packed) goes to slot
 * (p - 1) mod n_slots at d_ring + slot * slot_stride_bytes.  Every call that completes pairs enqueues ONE more kernel launch
 * on its `stream` for all those pairs, after the motion stage's (no timing kind records it).
 *   d_ring 16-byte aligned, slot_stride_bytes a multiple of 16 and at least rows * w * 8, n_slots >= stream_batch,
 *   0 <= level < levels; otherwise OFX_E_INVALID.  d_ring == NULL turns the stage off (the default: nothing is launched or
 *   allocated).
 * Only before the first frame of a stream (OFX_E_STATE once a stream has frames); stays in effect for later streams, whose
 * pairs count from 1 again.  Sharded sessions and frames_partial: OFX_E_UNSUPPORTED.
 * Sources: the pair's shift vector of that level (none at the coarsest) and the flow ofx_session_flow_of points to.  As written
 * at ofx_session_stream_motion: "All of them are intact in the call that completes the pair: that call's own LK stage reads both
 * image sets and the pair's shift-vector slot, a set is rewritten 3B + 2 (two stages: 2B + 2) frames later and a slot by the
 * corner stage of a later tick, and the last launch of a tick always leaves the final flow in the set flow_of reports."  The
 * stage reads no frame: the lifetime of borrowed frames is unchanged.  Lifetime of a slot: as the compose ring's. */
int ofx_session_stream_displacement(ofx_session *s, int level, float scale, float *d_ring, size_t slot_stride_bytes, int n_slots);
/* Slot of `pair` while it is one of the newest n_slots pairs of the displacement stage.  OFX_E_STATE without the stage,
 * OFX_E_INVALID for a pair not (or no longer) in the ring. */
int ofx_session_displacement_of(ofx_session *s, int pair, float **d_ptr);
/* Colour frames into the stream pipeline (main.cu:222-272 as one device-resident pipeline): with the front end set, every call
 * that launches a tick first enqueues ONE launch of the front end (ofx_frontend_1ch) for that tick's colour frames on its `stream`,
 * writing the filtered one-channel planes the tick then reads as its frames:
 *   mode: OFX_FRONTEND_OFF (the default: nothing allocated or launched), OFX_FRONTEND_GREY (average only) or
 *         OFX_FRONTEND_BILATERAL (average, then the bilateral filter with window / sigma_s / sigma_b; square odd windows 3 .. 13,
 *         others OFX_E_UNSUPPORTED; main.cu:240 uses 9, 2.0, 10.0);
 *   flags: OFX_FRONTEND_FLAG_FAST = the +-1 LSB arithmetic of the filter; OFX_FRONTEND_FLAG_FIRST_GREY = frame 0 of every stream is
 *         averaged only (main.cu:198-209: the first frame primes the previous pyramid unfiltered).
 * The planes: with borrow_frames = 0 the front end writes level 0 of the frame's image set and the pyramid stage does not copy
 * it; with borrow_frames = 1 the session owns one plane per image set at its level-0 pitch (allocated here, only then), and
 * those planes are what the later stages borrow.  Refinement iterations, the corner repair and the compose ring work unchanged.
 * Only before the first frame of a stream (OFX_E_STATE once a stream has frames); stays in effect for later streams.  Sharded
 * sessions: OFX_E_UNSUPPORTED. */
#define OFX_FRONTEND_FLAG_FAST 1
#define OFX_FRONTEND_FLAG_FIRST_GREY 2
int ofx_session_stream_frontend(ofx_session *s, int mode, int window, double sigma_s, double sigma_b, int flags);
/* ofx_session_stream_submit / _submit_frames for colour frames: interleaved 3-channel u8, 4-byte aligned, row pitch >= 3 * width
 * (OFX_E_INVALID otherwise).  The same contracts as the grey calls, completed pairs included.  A stream takes grey frames or colour
 * frames, not both (OFX_E_STATE), and colour frames need the front end set (OFX_E_STATE).  LIFETIME: a colour frame is read by
 * the front-end launch of the call that launches its tick, and by nothing after it -- it must stay valid and unmodified until
 * that launch has finished (the rule of a non-borrowed grey frame), whatever borrow_frames says. */
int ofx_session_stream_submit_3ch(ofx_session *s, const uint8_t *d_img3, int pitch, void *stream, int *completed_pair);
int ofx_session_stream_submit_frames_3ch(ofx_session *s, const uint8_t *const *d_img3, const int *pitches, int pitch0, int n, void *stream,
                                         int *completed_pair);
/* prev <- next (main.cu:270-272). */
int ofx_session_swap(ofx_session *s);
/* Device pointers / geometry of the session's buffers. which: 0 = prev, 1 = next, 2 = shifted scratch. */
int ofx_session_plane(ofx_session *s, int which, int level, uint8_t **d_ptr, ofx_geom *geom);
int ofx_session_flow(ofx_session *s, int level, float **d_ptr, int *row0, int *rows);
/* Shift vector slot of `level` for the pair IN PROGRESS (2 floats; levels are contiguous, 2 floats apart).  The session
 * alternates between two slots per pair, so query it again after every ofx_session_swap / solve_staged. */
int ofx_session_shift_uv(ofx_session *s, int level, float **d_uv);
/* Copy one level's flow (the rows this session owns, tightly packed) to host, synchronising `stream`. */
int ofx_session_get_flow_host(ofx_session *s, int level, float *h_dst, void *stream);

/* Time the fused LK launch (all levels in ofx_session_run_levels, level 0 in ofx_session_run_level) with HIP events recorded on the launch stream: arm for up to max_launches
 * launches (0 disarms); read returns the average/minimum duration in microseconds and re-arms. */
int ofx_session_timing(ofx_session *s, int max_launches);
int ofx_session_timing_read(ofx_session *s, double *avg_us, double *min_us, int *launches);
/* While armed, EVERY launch the session issues is bracketed and tagged with its kind; ofx_session_timing_read averages the
 * dominant ones (LK, LK_ACC, STREAM) and re-arms, ofx_session_timing_read_kind reads one kind and leaves the records in place
 * (call it before ofx_session_timing_read). */
#define OFX_TIME_LK 0      /* fused LK launch that writes the flow (all levels, or level 0 of run_level) */
#define OFX_TIME_LK_ACC 1  /* fused LK launch of a refinement iteration (flow += result) */
#define OFX_TIME_WARP 2    /* bilinear warp of a refinement iteration, all levels */
#define OFX_TIME_STREAM 3  /* one tick of the stream pipeline */
#define OFX_TIME_SHIFT 4   /* stand-alone global shift of all levels (refinement iterations only) */
#define OFX_TIME_CORNER 5  /* corner kernel */
#define OFX_TIME_PYRAMID 6 /* fused pyramid launch */
#define OFX_TIME_LK_ACC_WARP 7 /* the same launch when it also writes the next iteration's warped image (lk_body_warp.h) */
#define OFX_TIME_COMPOSE 8 /* the stream pipeline's output stage (ofx_session_stream_compose): one per call that completes pairs */
#define OFX_TIME_KINDS 9
int ofx_session_timing_read_kind(ofx_session *s, int kind, double *avg_us, double *min_us, int *launches);

/* ---- host-pointer convenience used by the gpu:: compat surface ------------ */
/* gpu::calc_opt_flow (OptFlowGpu.cuh:33): host 3ch images in, host flow pyramid in/out. */
int ofx_calc_opt_flow_host(const uint8_t *h_prev3, const uint8_t *h_next3, int w, int h, float **h_flow_pyr,
                           int level, int max_level, int window, int mode);

/* The host-pointer entry points (this one, ofx_compose_flow_host and the gpu:: / cpu:: wrappers) move transfers of 3 MB and
 * more in 2 MB chunks through pinned bounce buffers, on several threads at once: the caller and a small pool the library keeps
 * (environment OFX_STAGE_THREADS = pool size, default 3; -1 = plain hipMemcpy).  Returns the number of threads that share a
 * transfer.  The calls stay synchronous and retain nothing of the caller's. */
int ofx_stage_threads(void);

/* main.cu:138-147 (the dense field visualizeFlowField samples) with host pointers: h_flow_pyr[k] for k >= level are the
 * host flow levels gpu::calc_opt_flow filled, (w, h) is the size of `level`; h_dst receives 2*w*h floats. */
int ofx_compose_flow_host(float *const *h_flow_pyr, int w, int h, int levels, int level, float *h_dst);

#ifdef __cplusplus
}
#endif
#endif /* OFX_H */
