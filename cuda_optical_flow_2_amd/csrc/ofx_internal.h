// Internal helpers shared by the HIP translation units of libofx_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ofx.h"

// thread-local last-error message behind ofx_last_error()
void ofx_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define OFX_HIP(call)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            ofx_set_error("%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);           \
            return OFX_E_HIP;                                                                            \
        }                                                                                                \
    } while (0)

#define OFX_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            ofx_set_error(__VA_ARGS__); \
            return OFX_E_INVALID;       \
        }                               \
    } while (0)

#define OFX_TRY(expr)               \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != OFX_OK) return rc_; \
    } while (0)

static inline hipStream_t ofx_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

static inline int ofx_div_up(int a, int b) { return (a + b - 1) / b; }

// zeroes `words` 64-bit words at d_words (8-byte aligned) by a launch on the stream (zero_words.hip: why it is no memset)
int ofx_zero_words(void *d_words, size_t words, hipStream_t st);

// roctx range around a stage of the session (ofx_core.cpp; active with OFX_ROCTX=1, see there)
void ofx_range_push(const char *name);
void ofx_range_pop(void);
struct OfxRange {
    explicit OfxRange(const char *name) { ofx_range_push(name); }
    ~OfxRange() { ofx_range_pop(); }
    OfxRange(const OfxRange &) = delete;
    OfxRange &operator=(const OfxRange &) = delete;
};

// validates the parts of an ofx_geom every kernel relies on
int ofx_check_geom(const ofx_geom *g, const char *who);

// rows of the level that a stencil of vertical radius `halo` around [out_y0,out_y1) touches, clipped to the image,
// must be present in the buffer
int ofx_check_halo(const ofx_geom *g, int halo, const char *who);

// argument builders shared between the stand-alone stage launches and the stream (pipelined) launch; the structs live
// in stages_body.h / corner_body.h
namespace ofx_dev {
struct PyrArgs;
struct PyrMarchArgs;
struct ShiftTable;
struct CornerHead;
struct CornerLevel;
} // namespace ofx_dev
// row0/rows (NULL: whole levels): the global rows each destination plane (index 0 = the level-0 copy) holds
int ofx_pyramid_args(const uint8_t *d_level0, int pitch0, int w, int h, uint8_t *const *d_levels, const int *pitches, int levels,
                     uint8_t *d_level0_copy, int copy_pitch, const int *row0, const int *rows, ofx_dev::PyrArgs *out,
                     size_t *lds_bytes, int *blocks_x, int *blocks_y);
// the stream kernel's pyramid stage (pyr_march.h); *items = waves needed
int ofx_pyramid_march_args(const uint8_t *d_level0, int pitch0, int w, int h, uint8_t *const *d_levels, const int *pitches, int levels,
                           uint8_t *d_level0_copy, int copy_pitch, const int *row0, const int *rows, int target_waves,
                           ofx_dev::PyrMarchArgs *out, int *items);
int ofx_shift_table(const ofx_shift_desc *levels, int n, ofx_dev::ShiftTable *out, int *blocks_out);
// cols (NULL: full width): columns [0, cols[k]) each level's planes hold; d_status (NULL: none): see CornerHead::status;
// shard_rows (NULL: unchecked): 4 ints per level, CornerLevel::need0 .. valid1
int ofx_corner_args(const ofx_lk_desc *levels, int n_levels, int window, int mode, float *d_uv, const int *cols, int *d_status,
                    const int *shard_rows, ofx_dev::CornerHead *out, ofx_dev::CornerLevel *lv_out);
// sharded sessions whose shift vectors come from another rank: raise status bit 8 + k when level k's vertical shift sends the
// shard's reads (rows [need0, need1) before the shift) to image rows outside [valid0, valid1); shard_rows = 4 ints per level
int ofx_shard_margin_check(const float *d_uv, int levels, const int *heights, const int *shard_rows, int *d_status, void *stream);

// two refinement iterations in one launch (lk_level.hip, lk_body_pair.h): windows up to 9x9, lk_float solves, whole levels;
// d_flow_in[i]: the flow so far (read), levels[i].d_flow: the flow after both (written; another buffer)
// opts (NULL: one strip per wave): how the launch is planned.  pack: waves of equal steps, each marching up to two segments
// (pair_plan.h); the plans live on the device in *cache, which the first packed launch creates and its owner frees with
// ofx_pair_cache_free -- one plan per launch shape, made and uploaded when the shape is first seen, nothing after that.  waves > 0:
// the wave count of the packed plan instead of the device's (tests: small levels then straddle waves as large ones do).
struct ofx_pair_cache;
struct ofx_pair_opts {
    int pack, waves;
    ofx_pair_cache **cache;
};
void ofx_pair_cache_free(ofx_pair_cache *c);
int ofx_lk_levels_pair(const ofx_lk_desc *levels, const float *const *d_flow_in, int n, int window, int mode, const ofx_pair_opts *opts, void *stream);

// the stream pipeline's output stage (compose_ring.hip): the dense field (main.cu:138-147, = ofx_compose_flow at `level`) of
// n <= OFX_STREAM_MAX_BATCH pairs in one launch.  Pair i reads lv[i][k] (k = level .. levels-1; each points at global row own0[k]
// of its level, rows tightly packed, w >> (k - level) wide) and writes its rows x w x 2 floats tightly packed at dst[i]
// (16-byte aligned).  Own row y of the output reads row ((own0[level] + y) >> (k - level)) - own0[k] of level k: the caller
// sees that every such row is one the pair's level k holds.
struct ofx_compose_batch {
    const float *lv[OFX_STREAM_MAX_BATCH][OFX_MAX_LEVELS];
    float *dst[OFX_STREAM_MAX_BATCH];
    int own0[OFX_MAX_LEVELS];
    int n, w, rows, levels, level;
    unsigned n_px; // w * rows
};
int ofx_compose_batch_launch(const ofx_compose_batch *a, void *stream);

// the stream pipeline's sampled output stage (sample_ring.hip): the composed field (compose_px.h) of n <= OFX_STREAM_MAX_BATCH pairs
// read at a few positions instead of composed everywhere, in ONE launch.  Pair i reads lv[i][k] as in ofx_compose_batch.
//   arrows (arrows[0] != NULL): the arrow field of main.cu:123-169 of pair i at a_level (a_w x a_h, grid step a_offset = a_w / arrow_res,
//     a_ny x a_nx arrows), a_ny * a_nx records of four int32 (x0, y0, x1, y1; an undrawn arrow has x1 = y1 = -1) at arrows[i] (16-byte aligned);
//   tracks (points != NULL): n_points float2 (x, y) in pixels of t_level (t_w x t_h) and their int32 status (0 = alive), advected
//     through the n pairs in order; a point that leaves the level or meets a non-finite flow at pair i is frozen with status
//     pair0 + i.  hist[i] (NULL: none; 8-byte aligned) receives every point's position after pair i.
struct ofx_sample_batch {
    const float *lv[OFX_STREAM_MAX_BATCH][OFX_MAX_LEVELS];
    int32_t *arrows[OFX_STREAM_MAX_BATCH];
    float *hist[OFX_STREAM_MAX_BATCH];
    float *points;
    int32_t *status;
    int own0[OFX_MAX_LEVELS];
    int n, levels;
    int a_level, a_w, a_h, a_offset, a_ny, a_nx;
    int t_level, t_w, t_h, n_points, pair0;
};
int ofx_sample_batch_launch(const ofx_sample_batch *a, void *stream);
// offset / ny / nx of the arrow grid of a w x h level (main.cu:125-131); OFX_E_INVALID when w / arrow_res would be 0
int ofx_arrow_grid(int w, int h, int arrow_res, int *offset, int *ny, int *nx, const char *who);
// every level of a w x h pyramid that a coarser one is read under must have even dimensions (the session's rule): then pixel
// (y >> s, x >> s) of level k exists for every pixel of level `level`
int ofx_check_sample_pyramid(int w, int h, int levels, int level, const char *who);

// the stream pipeline's motion-compensation stage (motion_ring.hip; the definition: "motion compensation" in include/ofx.h) for
// n <= OFX_STREAM_MAX_BATCH pairs of one w x h level in ONE launch.  Pair i reads prev[i] / next[i] (u8 planes, each with its own
// pitch >= w), flow[i] (w x h interleaved float32, 8-byte aligned) and uv[i] (two floats on the device; NULL = no shift), and
// writes the image at dst[i] (rows dst_pitch apart, bytes beyond column w - 1 untouched; NULL = none) and ADDS its four sums to
// stats[i] (8-byte aligned; NULL = none), which the launch function zeroes on the stream first, consecutive slots by one launch.  dst_dwords: every dst and
// dst_pitch is 4-byte aligned, whole quads are stored as one dword.  Every argument is checked before anything is enqueued.
struct ofx_motion_batch {
    const uint8_t *prev[OFX_STREAM_MAX_BATCH], *next[OFX_STREAM_MAX_BATCH];
    const float *flow[OFX_STREAM_MAX_BATCH], *uv[OFX_STREAM_MAX_BATCH];
    uint8_t *dst[OFX_STREAM_MAX_BATCH];
    unsigned long long *stats[OFX_STREAM_MAX_BATCH];
    int prev_pitch[OFX_STREAM_MAX_BATCH], next_pitch[OFX_STREAM_MAX_BATCH];
    int n, w, h, dst_pitch, dst_dwords;
    float scale;
};
int ofx_motion_batch_launch(const ofx_motion_batch *a, void *stream);

// the forward-backward check (consistency.hip; the definition: "forward-backward consistency" in include/ofx.h) for
// n <= OFX_STREAM_MAX_BATCH pairs of one w x h level in ONE launch.  Pair i reads fwd[i] and bwd[i] (w x h interleaved float32,
// 8-byte aligned) and writes the classes at mask[i] (rows mask_pitch apart, bytes beyond column w - 1 untouched; NULL = none), e at
// err[i] (w floats per row, 4-byte aligned; NULL = none) and ADDS its four counts to stats[i] (8-byte aligned; NULL = none), which
// the launch function zeroes on the stream first, consecutive slots by one launch.  A pair needs one output at least.  The launch
// function works out by itself whether whole quads go out as one dword (every mask and mask_pitch 4-byte aligned) and as four
// floats (every err 16-byte aligned, w a multiple of 4).  Every argument is checked before anything is enqueued.
struct ofx_consistency_batch {
    const float *fwd[OFX_STREAM_MAX_BATCH], *bwd[OFX_STREAM_MAX_BATCH];
    uint8_t *mask[OFX_STREAM_MAX_BATCH];
    float *err[OFX_STREAM_MAX_BATCH];
    unsigned long long *stats[OFX_STREAM_MAX_BATCH];
    int n, w, h, mask_pitch;
    float scale, alpha, beta;
};
int ofx_consistency_batch_launch(const ofx_consistency_batch *a, void *stream);

// the pixel displacement (interp.hip; the definition: "pixel displacement" in include/ofx.h) of n <= OFX_STREAM_MAX_BATCH pairs of
// one w x h level in ONE launch.  Pair i reads flow[i] (w x h interleaved float32, 8-byte aligned) and uv[i] (two floats on the
// device; NULL = none) and writes w x h x 2 floats tightly packed at dst[i] (8-byte aligned).  Every argument is checked before
// anything is enqueued.
struct ofx_displacement_batch {
    const float *flow[OFX_STREAM_MAX_BATCH], *uv[OFX_STREAM_MAX_BATCH];
    float *dst[OFX_STREAM_MAX_BATCH];
    int n, w, h;
    float scale;
};
int ofx_displacement_batch_launch(const ofx_displacement_batch *a, void *stream);

// frame interpolation (interp.hip; the definition: "frame interpolation" in include/ofx.h) of n <= OFX_STREAM_MAX_BATCH pairs of one
// w x h size at n_times <= OFX_INTERP_MAX_TIMES times in ONE launch.  Pair i reads a[i] / b[i] (u8 planes, each with its own pitch
// >= w) and dab[i] / dba[i] (w x h interleaved float32, 8-byte aligned), writes frame k at dst[i] + k * time_stride (rows dst_pitch
// apart, bytes beyond column w - 1 untouched) and ADDS its counts to stats[i] + 4 * k (8-byte aligned; NULL = none), which the
// launch function zeroes on the stream first.  c00 / c01 / c10 / t: the definition's host step per time.  The launch function works
// out by itself whether whole quads go out as one dword.  Every argument is checked before anything is enqueued.
struct ofx_interp_batch {
    const uint8_t *a[OFX_STREAM_MAX_BATCH], *b[OFX_STREAM_MAX_BATCH];
    const float *dab[OFX_STREAM_MAX_BATCH], *dba[OFX_STREAM_MAX_BATCH];
    uint8_t *dst[OFX_STREAM_MAX_BATCH];
    unsigned long long *stats[OFX_STREAM_MAX_BATCH];
    int a_pitch[OFX_STREAM_MAX_BATCH], b_pitch[OFX_STREAM_MAX_BATCH];
    float t[OFX_INTERP_MAX_TIMES], c00[OFX_INTERP_MAX_TIMES], c01[OFX_INTERP_MAX_TIMES], c10[OFX_INTERP_MAX_TIMES];
    int n, w, h, n_times, dst_pitch;
    size_t time_stride;
};
int ofx_interp_batch_launch(const ofx_interp_batch *a, void *stream);

// colour frame interpolation (interp3.hip; the definition: "colour frame interpolation" in include/ofx.h): ofx_interp_batch's
// fields with a[i] / b[i] and dst[i] interleaved 3-channel planes, every pitch in bytes and >= 3 * w, the geometry and the counts
// once per pixel.  Whole quads go out as three dwords where every dst, dst_pitch and time_stride are 4-byte aligned.
struct ofx_interp3_batch : ofx_interp_batch {};
int ofx_interp3_batch_launch(const ofx_interp3_batch *a, void *stream);

// the stream pipeline's colour front end (frontend.hip): the filter's tables for one (window, sigma_s, sigma_b), built once on the
// host (window 0: grey frames only; an unsupported window is OFX_E_UNSUPPORTED), and one launch over n <= OFX_STREAM_MAX_BATCH
// frames (modes[i]: OFX_FRONTEND_GREY / _BILATERAL / _BILATERAL_FAST; a call that mixes the two bilateral forms launches twice)
struct ofx_frontend_tables;
int ofx_frontend_tables_make(int window, double sigma_s, double sigma_b, ofx_frontend_tables **out);
void ofx_frontend_tables_free(ofx_frontend_tables *t);
int ofx_frontend_run(const ofx_frontend_tables *t, const uint8_t *const *src3, const int *src_pitch, uint8_t *const *dst, const int *dst_pitch,
                     const int *modes, int n, int w, int h, hipStream_t st);
