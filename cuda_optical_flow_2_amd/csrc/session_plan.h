// What a session is and where its buffers lie: everything ofx_session_create decides before it touches the device -- the checks of
// ofx_params, the paths the session takes (iterations fused, two per launch; the corner's repair), the geometry of its levels and
// the byte offset, from the base of its one hipMalloc arena, of every pointer it holds.  Plain host code without HIP in it, like
// iter_plan.h and pair_plan.h: tools/session_plan_main.cpp prints the plans, tests/test_session_plan.py checks them against a
// transcription of the function that used to hold this arithmetic (tests/session_layout_ref.py).  ofx_session_create (session.cpp)
// allocates plan.total bytes and walks the offsets.
#pragma once

#include <stdio.h>
#include <string.h>

#include "ofx.h"

#ifndef OFX_ITER_PAIRS_DEFAULT
#define OFX_ITER_PAIRS_DEFAULT 1 // the stream pipeline's iterations two per launch (lk_body_pair.h); OFX_ITER_PAIRS=0 / 1 overrides
#endif

namespace ofx_plan {

// The stream pipeline with B frames per tick uses 3B + 2 image sets and 2B shift-vector slots (see stream_tick); the
// pair-at-a-time paths rotate 3 sets and alternate 2 slots.
constexpr int kMaxBatch = OFX_STREAM_MAX_BATCH;
constexpr int kSets = 3 * kMaxBatch + 2;
constexpr int kUvSlots = 2 * kMaxBatch;
constexpr size_t kAlign = 256; // of every plane and table in the arenas
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// frames per tick of the stream pipeline (a session created without a stream_batch may still stream one frame per tick), and the
// image sets it cycles through: (D + 1) B + 2 with D stages (stream_tick); the pair-at-a-time paths rotate the first three
inline int stream_batch_of(const ofx_params &p) { return p.stream_batch >= 2 ? p.stream_batch : 1; }
inline int stream_sets(const ofx_params &p) { return (p.stream_two_stage ? 2 : 3) * stream_batch_of(p) + 2; }

// Bytes of a u8 plane of this pitch and these rows in an arena: the fused warp of a refinement iteration fetches a tap's dword AT
// the tap's byte (lk_body_warp.h), so every plane is followed by 64 readable bytes.
inline size_t plane_bytes(int pitch, int rows) { return align_up((size_t)pitch * (size_t)rows + 64, kAlign); }

// Levels of 16 Mpx and more do not stay cached between their two uses: the LK launches fetch their rows two steps ahead through LDS
// (lk_plan.h: iter_deep_fetch, tick_deep_fetch), and such a session's iterations run one per launch.
inline bool deep_fetch_by_size(long px) { return px >= 16l * 1000 * 1000; }
inline bool iter_deep_fetch(int iter_dma, long largest_px); // lk_plan.h (included below): the iteration launch's rule

// The launches that also write the warped image address a level's planes and its flow rows through buffer resources with 32-bit
// offsets (lk_body_buf.h): both must stay below 2 GB.
inline bool fits_buffer_offsets(long long plane_rows, int pitch, long long flow_rows, int w)
{
    return plane_rows * pitch < (1ll << 31) && flow_rows * w * 8 < (1ll << 31);
}

// The switches a session reads from the environment, once per ofx_session_create (session_switches_from_env, session.cpp).
struct SessionSwitches {
    bool iter_fused = true;                          // OFX_ITER_FUSED=0 keeps one ofx_warp_levels launch per refinement iteration
    bool iter_pairs = OFX_ITER_PAIRS_DEFAULT != 0;   // OFX_ITER_PAIRS=0 / 1: the stream pipeline's iterations two per launch
    bool iter_dma = false;                           // OFX_ITER_DMA > 0: the iterations are forced onto the deep fetch, which has no two-iteration form
    bool pair_pack = true;                           // OFX_PAIR_PACK=0: one strip per wave in the two-iteration launches
    int pair_waves = 0;                              // OFX_PAIR_WAVES > 0: the wave count of their packed plan (0: the device's)
    int debug_corner_extent = 0;                     // OFX_DEBUG_CORNER_EXTENT: see SessionPlan::debug_extent
};

constexpr size_t kNoOffset = ~(size_t)0; // this pointer of the session stays null

struct LevelPlan {
    int w, h, pitch;
    int own0, own1, buf0, buf1, cmp0, cmp1, fl0, fl1; // rows: see ofx_session (session.h)
    int pw, ph, ppitch;                               // the top-left patch's plane (local_corner / stream_two_stage; else 0)
    size_t plane_bytes, flow_bytes, patch_bytes;      // of one image / shifted / scratch plane, one flow set, one patch plane
};

// Byte offsets from the arena's base, kNoOffset where the session has no such buffer; named and indexed like the session's pointers.
struct ArenaOffsets {
    size_t img[kSets][OFX_MAX_LEVELS], sh[2][OFX_MAX_LEVELS], itsh[kMaxBatch][3][OFX_MAX_LEVELS];
    size_t flowset[kMaxBatch][OFX_MAX_LEVELS], flowset2[kMaxBatch][OFX_MAX_LEVELS];
    size_t pimg[kSets][OFX_MAX_LEVELS], pscr[kMaxBatch][2][OFX_MAX_LEVELS], preloc[kMaxBatch][OFX_MAX_LEVELS];
    size_t status, uv, staging; // the sticky status word, then one word per shift-vector slot; the shift vectors; one 3-channel frame
};

struct SessionPlan {
    ofx_params p;                 // the effective parameters (a single-level session with iterations copies its frames)
    LevelPlan lv[OFX_MAX_LEVELS];
    int B, n_sets, n_iter_sets;   // frames per tick; image sets (the pair-at-a-time paths rotate the first three); iteration scratch planes
    bool repair;                  // a shift that leaves the patch is repaired (ofx_corner_stage.d_patch_reloc)
    int frames_per_slot;          // patch pyramids per corner slot: two frames (stream_two_stage) + the relocated one (repair)
    // Test hook (OFX_DEBUG_CORNER_EXTENT, repairing sessions only): pretend the top-left patch planes are only this many level-0
    // pixels wide and high (never less than the corner itself), so that ordinary frames drive the chain into the relocated
    // planes; the results must not change.
    int debug_extent;
    bool fused_iters, iter_pairs; // see ofx_session
    int pair_pack, pair_waves;    // ofx_pair_opts
    size_t pscr_frame;            // bytes of one patch pyramid of a corner slot (levels 1 and up)
    ArenaOffsets off;
    size_t total; // the arena's size
};

#define OFX_PLAN_REQUIRE(cond, ...)               \
    do {                                          \
        if (!(cond)) {                            \
            snprintf(err, err_len, __VA_ARGS__);  \
            return OFX_E_INVALID;                 \
        }                                         \
    } while (0)

// Pure: no globals, no environment, no HIP.  OFX_OK, or OFX_E_INVALID with the message in err.
inline int session_plan_make(const ofx_params *in, const SessionSwitches &sw, SessionPlan *out, char *err, size_t err_len)
{
    SessionPlan &q = *out;
    // The fused warp's source must be followed by three readable bytes (plane_bytes).  Every plane of a session is; the one warp
    // source that would be a caller's buffer is level 0 of a single-level session on borrowed frames (pair at a time: the stream
    // pipeline needs two levels) -- such a session copies its frames.
    q.p = *in;
    if (q.p.levels == 1 && q.p.iters > 1 && q.p.borrow_frames) q.p.borrow_frames = 0, q.p.stream_two_stage = 0;
    const ofx_params *p = &q.p;
    OFX_PLAN_REQUIRE(p->width > 0 && p->height > 0, "ofx_session_create: bad size %dx%d", p->width, p->height);
    OFX_PLAN_REQUIRE(p->levels >= 1 && p->levels <= OFX_MAX_LEVELS, "ofx_session_create: levels %d out of range", p->levels);
    OFX_PLAN_REQUIRE(p->window >= 3 && (p->window & 1), "ofx_session_create: window must be odd and >= 3");
    OFX_PLAN_REQUIRE(p->mode == OFX_MODE_COMPAT_CPU || p->mode == OFX_MODE_LK_FLOAT || p->mode == OFX_MODE_LK_FLOAT_FAST,
                     "ofx_session_create: bad mode %d", p->mode);
    OFX_PLAN_REQUIRE(p->min_det >= 0.0f, "ofx_session_create: min_det must be >= 0 (0 = the reference's unguarded solve)");
    OFX_PLAN_REQUIRE(p->iters >= 0 && p->iters <= 64, "ofx_session_create: iters %d out of range", p->iters);
    OFX_PLAN_REQUIRE(p->stream_batch >= 0 && p->stream_batch <= OFX_STREAM_MAX_BATCH, "ofx_session_create: stream_batch %d (0 .. %d)",
                     p->stream_batch, OFX_STREAM_MAX_BATCH);
    OFX_PLAN_REQUIRE(p->stream_batch * p->levels <= OFX_MAX_LK_ITEMS, "ofx_session_create: stream_batch %d needs levels <= %d",
                     p->stream_batch, OFX_MAX_LK_ITEMS / (p->stream_batch > 0 ? p->stream_batch : 1));
    OFX_PLAN_REQUIRE(!p->stream_two_stage || p->borrow_frames, "ofx_session_create: stream_two_stage needs borrow_frames (the corner stage reads "
                                                                 "both frames of a pair in the tick in which the second one arrives)");
    OFX_PLAN_REQUIRE(p->iters <= 1 || p->mode != OFX_MODE_COMPAT_CPU, "ofx_session_create: refinement iterations need mode lk_float");
    OFX_PLAN_REQUIRE(p->deep_fetch >= -1 && p->deep_fetch <= 1, "ofx_session_create: deep_fetch must be -1, 0 or +1 (got %d)", p->deep_fetch);
    OFX_PLAN_REQUIRE(!p->frames_partial || (p->sharded && p->local_corner && !p->stream_two_stage),
                     "ofx_session_create: frames_partial describes the frames of a sharded local_corner session (not stream_two_stage)");
    OFX_PLAN_REQUIRE(p->iters <= 1 || !p->sharded || p->local_corner,
                     "ofx_session_create: refinement iterations on a sharded session run through the stream pipeline, which needs local_corner");
    OFX_PLAN_REQUIRE((p->width >> (p->levels - 1)) > 0 && (p->height >> (p->levels - 1)) > 0,
                     "ofx_session_create: %d levels is too many for %dx%d", p->levels, p->width, p->height);
    for (int k = 0; k + 1 < p->levels; ++k)
        OFX_PLAN_REQUIRE(((p->width >> k) & 1) == 0 && ((p->height >> k) & 1) == 0,
                         "ofx_session_create: level %d is %dx%d; every level that is downsampled must have even dimensions "
                         "(the reference assumes a source stride of exactly 2*w, OptFlowCPU.cpp:117)",
                         k, p->width >> k, p->height >> k);

    const int L = p->levels, radius = p->window >> 1;
    const int B = q.B = stream_batch_of(*p), n_sets = q.n_sets = stream_sets(*p);
    // streamed refinement iterations: per flow set three more planes (shifted, warped, warped')
    const int n_iter_sets = q.n_iter_sets = p->iters > 1 ? 3 * B : 0;
    // Two iterations per launch in the stream pipeline (lk_body_pair.h): unsharded lk_float sessions with three iterations or more,
    // windows up to 9x9, levels whose iteration launches may not take the deep fetch, which has no two-iteration form.
    const bool want_pairs = p->iters >= 3 && !p->sharded && (p->mode == OFX_MODE_LK_FLOAT || p->mode == OFX_MODE_LK_FLOAT_FAST) &&
                            radius >= 1 && radius <= 4 && !iter_deep_fetch(sw.iter_dma ? 1 : -1, (long)p->width * p->height) && sw.iter_pairs;

    ArenaOffsets &o = q.off;
    memset(&o, 0xff, sizeof o); // kNoOffset everywhere
    size_t total = 0;
    auto take = [&total](size_t bytes) { // the next `bytes` of the arena
        const size_t at = total;
        total += bytes;
        return at;
    };
    for (int k = 0; k < L; ++k) {
        LevelPlan &l = q.lv[k];
        l = LevelPlan{};
        l.w = p->width >> k;
        l.h = p->height >> k;
        l.pitch = (int)align_up((size_t)l.w, 64);
        if (p->sharded) {
            l.own0 = p->own_y0[k], l.own1 = p->own_y1[k];
            l.buf0 = p->buf_y0[k], l.buf1 = p->buf_y1[k];
            const bool has_comp = p->comp_y1[k] > 0;
            l.cmp0 = has_comp ? p->comp_y0[k] : l.own0;
            l.cmp1 = has_comp ? p->comp_y1[k] : l.own1;
            OFX_PLAN_REQUIRE(0 <= l.buf0 && l.buf0 <= l.own0 && l.own0 <= l.own1 && l.own1 <= l.buf1 && l.buf1 <= l.h && l.buf0 < l.buf1 &&
                                 l.buf0 <= l.cmp0 && l.cmp0 <= l.own0 && l.own1 <= l.cmp1 && l.cmp1 <= l.buf1,
                             "ofx_session_create: level %d shard rows own [%d,%d) buf [%d,%d) invalid for height %d", k, l.own0, l.own1,
                             l.buf0, l.buf1, l.h);
        } else {
            l.own0 = l.buf0 = l.cmp0 = 0;
            l.own1 = l.buf1 = l.cmp1 = l.h;
        }
        l.fl0 = l.own0;
        l.fl1 = l.own1;
        if (p->sharded && p->iters > 1) { // the flow buffers hold (radius + 1) * (iters - 1) rows either side of the own rows (session.h)
            const int reach = radius + 1, ext = reach * (p->iters - 1);
            l.fl0 = l.own0 - ext > 0 ? l.own0 - ext : 0;
            l.fl1 = l.own1 + ext < l.h ? l.own1 + ext : l.h;
            const int lo = l.fl0 - reach > 0 ? l.fl0 - reach : 0, hi = l.fl1 + reach < l.h ? l.fl1 + reach : l.h;
            OFX_PLAN_REQUIRE(lo >= l.buf0 && hi <= l.buf1,
                             "ofx_session_create: level %d: %d iterations need rows [%d,%d) in the buffers (own rows +- (radius + 1) * iters), "
                             "they hold [%d,%d): plan the shard with its iterations (ShardPlan(iters=...))", k, p->iters, lo, hi, l.buf0, l.buf1);
        }
        l.plane_bytes = plane_bytes(l.pitch, l.buf1 - l.buf0);
        for (int t = 0; t < n_sets; ++t) o.img[t][k] = take(l.plane_bytes);
        for (int t = 0; t < 2; ++t) o.sh[t][k] = take(l.plane_bytes);
        for (int t = 0; t < n_iter_sets; ++t) o.itsh[t / 3][t % 3][k] = take(l.plane_bytes);
        const size_t flow_rows = (size_t)(l.fl1 - l.fl0);
        l.flow_bytes = align_up((flow_rows ? flow_rows : 1) * (size_t)l.w * 2 * sizeof(float), kAlign);
        // a B-frame stream tick writes the flows of B pairs: B sets; the sets a session of fewer frames per tick never writes are set 0
        for (int t = 0; t < B; ++t) o.flowset[t][k] = take(l.flow_bytes);
        for (int t = 1; t < kMaxBatch; ++t)
            if (t >= p->stream_batch) o.flowset[t][k] = o.flowset[0][k];
    }
    q.repair = false;
    q.pscr_frame = 0;
    const bool patch = p->local_corner || p->stream_two_stage;
    if (patch) {
        const int step = 1 << (L - 1), lc = L - 1;
        int side = p->patch_size > 0 ? p->patch_size : step * (radius + 2 + 8);
        if (p->patch_size <= 0 && side < 256) side = 256;
        side = (int)align_up((size_t)side, (size_t)step);
        const int pw0 = side < p->width ? side : p->width, ph0 = side < p->height ? side : p->height;
        for (int k = 0; k < L; ++k) {
            LevelPlan &l = q.lv[k];
            l.pw = pw0 >> k;
            l.ph = ph0 >> k;
            l.ppitch = (int)align_up((size_t)l.pw, 64);
            l.patch_bytes = plane_bytes(l.ppitch, l.ph);
        }
        const LevelPlan &c = q.lv[lc];
        const int need = radius + 2;
        OFX_PLAN_REQUIRE(c.pw >= (need < c.w ? need : c.w) && c.ph >= (need < c.h ? need : c.h),
                         "ofx_session_create: patch_size %d leaves %dx%d at the coarsest level, the corner needs %d", side, c.pw, c.ph, need);
        // With the frames borrowed the whole next frame is at hand when the chain runs: a shift that leaves the patch is repaired
        // (ofx_corner_stage.d_patch_reloc) -- provided the patch leaves room at the coarsest level to be placed around any
        // target (radius + 3 pixels of stencils + the plane's first column / row); a smaller patch (patch_size) keeps the
        // status bit.
        const int need_r = radius + 5;
        const bool room = (c.pw >= need_r || c.pw >= c.w) && (c.ph >= need_r || c.ph >= c.h);
        q.repair = p->borrow_frames && !p->frames_partial && L >= 3 && room;
    }
    q.debug_extent = q.repair ? sw.debug_corner_extent : 0;
    q.frames_per_slot = (p->stream_two_stage ? 2 : 0) + (q.repair ? 1 : 0);
    if (patch) {
        // (stream_two_stage: no patch pyramids per image set, the corner blocks build what they read)
        for (int k = 0; k < L && !p->stream_two_stage; ++k)
            for (int t = 0; t < n_sets; ++t) o.pimg[t][k] = take(q.lv[k].patch_bytes);
        // the corner slots' patch pyramids: slot i, frame f at (frames_per_slot * i + f) * pscr_frame, its levels 1 and up one after the other
        for (int k = 1; k < L; ++k) q.pscr_frame += q.lv[k].patch_bytes;
        for (int i = 0; i < B; ++i)
            for (int f = 0; f < q.frames_per_slot; ++f) {
                size_t at = take(q.pscr_frame);
                for (int k = 1; k < L; at += q.lv[k].patch_bytes, ++k) {
                    if (f < 2 && p->stream_two_stage) o.pscr[i][f][k] = at;
                    if (f == q.frames_per_slot - 1 && q.repair) o.preloc[i][k] = at;
                }
            }
    }
    o.status = take(align_up(sizeof(int) * (size_t)(1 + kUvSlots), kAlign));
    o.uv = take(align_up((size_t)OFX_MAX_LEVELS * 2 * sizeof(float) * kUvSlots, kAlign));
    if (!p->sharded) o.staging = take(align_up((size_t)p->width * (size_t)p->height * 3, kAlign)); // for ofx_session_set_frame_host_3ch
    // the second flow set of every pair slot, behind everything else: the first sets lie where they do without it
    for (int k = 0; k < L && want_pairs; ++k)
        for (int t = 0; t < B; ++t) o.flowset2[t][k] = take(q.lv[k].flow_bytes);
    q.total = total;

    // a session whose level 0 does not fit the buffer march keeps the warp launch + the old accumulating march
    const LevelPlan &l0 = q.lv[0];
    q.fused_iters = p->iters > 1 && sw.iter_fused && fits_buffer_offsets(l0.buf1 - l0.buf0, l0.pitch, l0.buf1 - l0.buf0, l0.w);
    q.iter_pairs = want_pairs && q.fused_iters;
    q.pair_pack = sw.pair_pack ? 1 : 0;
    q.pair_waves = sw.pair_waves;
    return OFX_OK;
}

#undef OFX_PLAN_REQUIRE

} // namespace ofx_plan

#include "lk_plan.h" // iter_deep_fetch
