// Device-resident session: the frame loop of main.cu:192-272 with every buffer living in HBM.  The session's state and what its two
// units share: session.cpp (create / destroy, the pair-at-a-time and the pipelined path) and session_stream.cpp (the stream pipeline).
//
// One hipMalloc arena holds, per pyramid level: the previous and the next frame's 1-channel planes, a scratch
// plane for the shifted next frame, the flow field, and the 2-float shift vector.  Nothing is allocated or freed
// while frames flow (the reference does 58 cudaMalloc/cudaFree calls per level).  What a session of given
// ofx_params holds, which paths it takes and where in the arena every buffer lies is decided in session_plan.h (host code
// without HIP; tools/session_plan_main.cpp prints it): ofx_session_create allocates the plan's total and points the fields
// below at base + offset.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "iter_plan.h"
#include "ofx_internal.h"
#include "out_ring.h"
#include "session_plan.h"

using ofx_plan::align_up;
using ofx_plan::kAlign;
using ofx_plan::kMaxBatch;
using ofx_plan::kSets;
using ofx_plan::kUvSlots;

struct ofx_session {
    ofx_params p{};
    int w[OFX_MAX_LEVELS]{}, h[OFX_MAX_LEVELS]{}, pitch[OFX_MAX_LEVELS]{};
    int own0[OFX_MAX_LEVELS]{}, own1[OFX_MAX_LEVELS]{}; // rows this rank computes
    int buf0[OFX_MAX_LEVELS]{}, buf1[OFX_MAX_LEVELS]{}; // rows the plane buffers hold
    int cmp0[OFX_MAX_LEVELS]{}, cmp1[OFX_MAX_LEVELS]{}; // rows this rank downsamples itself
    // rows the flow buffers hold: the own rows, or -- sharded sessions with refinement iterations -- the own rows plus
    // (radius + 1) * (iters - 1) either side: iteration j is computed on (radius + 1) * (iters - j) extra rows so that the
    // warp of iteration j + 1 finds the flow of every row its LK stencils touch without asking a neighbour (stream_tick)
    int fl0[OFX_MAX_LEVELS]{}, fl1[OFX_MAX_LEVELS]{};
    size_t flow_own_offset(int k) const { return (size_t)(own0[k] - fl0[k]) * (size_t)w[k] * 2; } // floats from a flow set to the own rows
    // storage: three image sets rotate through the roles prev -> (free) -> next, two shifted-scratch sets alternate, so
    // that the pipelined path can build frame i+1's pyramid / corner / shift while pair i's LK launch is running
    uint8_t *img[kSets][OFX_MAX_LEVELS]{};              // see kSets
    uint8_t *sh[2][OFX_MAX_LEVELS]{};
    // refinement iterations in the stream pipeline: per flow set (pair p -> set p mod B) the shifted and the warped next image
    uint8_t *itsh[kMaxBatch][3][OFX_MAX_LEVELS]{};
    bool fused_iters = false; // the accumulating launches also write the next iteration's warped image (lk_body_warp.h)
    // the stream pipeline runs the iterations after the tick's two per launch (lk_body_pair.h): such a launch reads one flow set and
    // writes another, so every pair slot has a second set (flowset2); the last launch of a tick always writes flowset
    bool iter_pairs = false;
    // the schedule of iterations 2 .. iters (iter_plan.h), made once: the stream tick's (two per launch with iter_pairs; the flow set
    // its LK stage writes is the first pass's fin) and the pair-at-a-time path's (always one per launch, in place)
    ofx_plan::IterPass iter_plan[ofx_plan::kMaxIterPasses], iter_plan1[ofx_plan::kMaxIterPasses];
    int n_iter_pass = 0, n_iter_pass1 = 0;
    // the fused launches' plan (lk_launch.h): waves of equal steps (OFX_PAIR_PACK=0: one strip per wave, as before), the wave count
    // OFX_PAIR_WAVES forces on that plan (0: the device's), and the plans this session has made (freed with it)
    ofx_pair_opts pair_opts{1, 0, nullptr};
    ofx_pair_cache *pair_cache = nullptr;
    float *flowset2[kMaxBatch][OFX_MAX_LEVELS]{};
    int cur = 0, sht = 0;                               // img[cur] = previous frame, img[(cur+1)%3] = next frame
    uint8_t *plane[3][OFX_MAX_LEVELS]{};                // role view: 0 prev, 1 next, 2 shifted scratch
    hipStream_t aux = nullptr;                          // pipelined path: staging stream owned by the session
    hipEvent_t ev_ready = nullptr;                      // staging of the next pair finished (aux -> main)
    hipEvent_t ev_set_done[3] = {nullptr, nullptr, nullptr}; // last LK launch that read img[i] as `prev` finished
    bool set_busy[3] = {false, false, false};
    bool staged = false;
    int uv_slot = 0; // shift-vector slot of the pair in progress; alternates per pair so that the staging of the next
                     // pair (aux stream) never overwrites vectors the running LK launch still reads
    float *uv_cur() { return uv + (size_t)uv_slot * 2 * OFX_MAX_LEVELS; }
    long stream_n = -1;      // ticks of the stream pipeline so far (-1: not streaming)
    long stream_frames = -1; // total frames, known once draining starts (-1: still receiving)
    int pitch0_next() const { return pitch[0]; }
    // local_corner: the top-left patch of every frame as a pyramid of its own (same 5 sets as img)
    uint8_t *pimg[kSets][OFX_MAX_LEVELS]{};
    int pw[OFX_MAX_LEVELS]{}, ph[OFX_MAX_LEVELS]{}, ppitch[OFX_MAX_LEVELS]{};
    // stream_two_stage: the patch planes the corner block of slot i builds for its pair (frame 0: previous, 1: next)
    uint8_t *pscr[kMaxBatch][2][OFX_MAX_LEVELS]{};
    // the repair of a shift that leaves the patch (ofx_corner_stage.d_patch_reloc): per corner slot one more set of patch planes,
    // for the next frame's pyramid rebuilt around the shifted corner.  Allocated where the whole frames stay at hand
    // (borrow_frames) and the chain reads a patch (stream_two_stage, local_corner).
    uint8_t *preloc[kMaxBatch][OFX_MAX_LEVELS]{};
    bool repair = false;
    int debug_extent = 0; // test hook (OFX_DEBUG_CORNER_EXTENT): the chain may only read this many level-0 columns / rows of its patch planes
    int *corner_status = nullptr;
    int *pair_status = nullptr; // one word per shift-vector slot (pair p -> slot p mod 2B)
    const uint8_t *pframe[3] = {nullptr, nullptr, nullptr}; // borrow_frames, pair-at-a-time: the caller's frame behind img[i]'s level 0
    float *flow[OFX_MAX_LEVELS]{};       // where results are read from: flowset[0], or the newest pair's set in a two-frame stream
    float *flowset[kMaxBatch][OFX_MAX_LEVELS]{}; // stream pipeline: pair p's flow goes to set p mod stream_batch
    const uint8_t *held_frame[kMaxBatch]{};      // multi-frame stream tick: the frames waiting for the tick to fill
    int held_pitch[kMaxBatch]{};
    int n_held = 0;
    const uint8_t *bframe[kSets]{}; // borrow_frames: the caller's buffer behind image set i (level 0 is read from there)
    int bpitch[kSets]{};
    long reported = 0;                   // highest pair reported complete by the stream pipeline
    long corner_newest = 0;              // highest pair whose corner stage has been enqueued (ofx_session_pair_status)
    float *uv = nullptr;        // 2 floats per level
    uint8_t *staging = nullptr; // one tightly packed 3ch level-0 frame for host uploads
    void *arena = nullptr;
    size_t arena_bytes = 0;
    bool have_next = false, have_prev = false;
    // optional timing of the level-0 fused LK launch: event pairs recorded on the launch stream
    bool timing = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_kind; // OFX_TIME_* of event pair i
    size_t ev_used = 0;
    hipEvent_t ev_frame = nullptr; // staged path: the caller's frame is complete (caller's stream -> aux)
    int n_sets = 0;                // image sets allocated (3B + 2; the pair-at-a-time paths rotate the first three)
    // The output stages of the stream pipeline: each writes the pairs a call completes into a ring of the caller's (out_ring.h).  All
    // rings are in `out`, so that ofx_session_stream_begin resets every one; a stage's level, scale, pitch and grid stay next to it.
    enum { RING_COMPOSE, RING_ARROWS, RING_TRACKS, RING_MOTION, RING_DISP, N_RINGS };
    ofx_ring::OutRing out[N_RINGS];
    int ring_level = 0; // ofx_session_stream_compose: out[RING_COMPOSE] holds composed fields
    // ofx_session_stream_arrows / _stream_tracks (sample_ring.hip): out[RING_ARROWS] holds arrow fields and its `newest` is the one
    // counter of both (only the arrows have an accessor); the points and statuses (trk_points nullptr: tracks off) and, optional,
    // out[RING_TRACKS], the history of the points' positions
    int arrow_level = 0, arrow_offset = 0, arrow_ny = 0, arrow_nx = 0;
    float *trk_points = nullptr;
    int32_t *trk_status = nullptr;
    int trk_n = 0, trk_level = 0;
    // ofx_session_stream_motion (motion_ring.hip): out[RING_MOTION] holds images (its base may be nullptr) and gives the slot count
    // and the newest pair of the stats ring as well: pair p's four words are at mc_stats + 4 * index(p).  Both nullptr: off
    int64_t *mc_stats = nullptr;
    int mc_pitch = 0, mc_level = 0;
    float mc_scale = 0.0f;
    bool motion_on() const { return out[RING_MOTION].on() || mc_stats; }
    // ofx_session_stream_displacement (interp.hip): out[RING_DISP] holds displacement fields
    int disp_level = 0;
    float disp_scale = 0.0f;
    // ofx_session_stream_frontend: colour frames through the front end (frontend.hip).  fe_mode: what a frame gets
    // (OFX_FRONTEND_GREY / _BILATERAL / _BILATERAL_FAST), 0 = off; frame 0 of a stream gets OFX_FRONTEND_GREY with
    // OFX_FRONTEND_FLAG_FIRST_GREY.  borrow_frames: the filtered plane of image set i (fplane[i], at pitch[0]) stands in for the
    // borrowed frame; otherwise the front end writes img[i][0] and the pyramid stage does not copy level 0.
    int fe_mode = 0, fe_flags = 0;
    ofx_frontend_tables *fe = nullptr;
    void *fe_arena = nullptr;
    uint8_t *fplane[kSets]{};
    int stream_input = 0; // what the stream in progress has received: 0 = nothing yet, 1 = grey frames, 2 = colour frames
};

// Runs `launch` bracketed by a pair of timing events of kind `kind` when the session is armed (ofx_session_timing).
template <typename F>
inline int timed_launch(ofx_session *s, int kind, void *stream, F &&launch)
{
    static const char *const names[OFX_TIME_KINDS] = {"ofx.lk_levels", "ofx.lk_levels_accumulate", "ofx.warp_levels", "ofx.stream_tick",
                                                      "ofx.shift_levels", "ofx.corner_flows", "ofx.pyramid", "ofx.lk_levels_accumulate_warp",
                                                      "ofx.compose_ring"};
    OfxRange range(names[kind]); // (roctx, OFX_ROCTX=1: the launch's enqueue on the host side of a --marker-trace timeline)
    const bool timed = s->timing && s->ev_used + 2 <= s->ev.size();
    if (timed) OFX_HIP(hipEventRecord(s->ev[s->ev_used], ofx_stream(stream)));
    OFX_TRY(launch());
    if (timed) {
        OFX_HIP(hipEventRecord(s->ev[s->ev_used + 1], ofx_stream(stream)));
        s->ev_kind[s->ev_used / 2] = kind;
        s->ev_used += 2;
    }
    return OFX_OK;
}

inline ofx_geom level_geom(const ofx_session *s, int k, int out0, int out1)
{
    ofx_geom g;
    g.w = s->w[k];
    g.h = s->h[k];
    g.pitch = s->pitch[k];
    g.row0 = s->buf0[k];
    g.rows = s->buf1[k] - s->buf0[k];
    g.out_y0 = out0;
    g.out_y1 = out1;
    return g;
}

// per level: the image rows the LK stencils of this shard's own rows touch (before the shift) and the rows its buffers hold
inline void shard_reach(const ofx_session *s, int (*rows)[4])
{
    const int reach = s->p.window / 2 + 1; // the LK stencil of the rows it computes reaches radius + 1 rows beyond them
    for (int k = 0; k < s->p.levels; ++k) {
        const int n0 = s->fl0[k] - reach, n1 = s->fl1[k] + reach;
        rows[k][0] = n0 < 0 ? 0 : n0;
        rows[k][1] = n1 > s->h[k] ? s->h[k] : n1;
        rows[k][2] = s->buf0[k]; // (rows outside comp but inside buf are the caller's to fill: the halo exchange)
        rows[k][3] = s->buf1[k];
    }
}

inline int stream_batch_of(const ofx_session *s) { return ofx_plan::stream_batch_of(s->p); }
inline int stream_sets(const ofx_session *s) { return ofx_plan::stream_sets(s->p); }
