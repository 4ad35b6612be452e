// The stream pipeline of a session (session.h): ticks, submit and drain, flow_of, the colour front end, and the ring outputs.
#include "session.h"

// ---- stream pipeline: one launch per tick of B frames ----------------------------------------------------------------
// Frame f (0-based) belongs to tick f / B (B = stream_batch: 1, 2 or 4).  Pair p is (frame p-1 -> frame p).  The tick
// whose first frame is f0 runs, side by side in one grid,
//     pyramid(frames f0 .. f0+B-1) | corner(pairs f0-B .. f0-1) | LK(pairs f0-2B .. f0-B-1, shift fused)
// (with ofx_params.stream_two_stage: pyramid(f0 .. f0+B-1) | corner(pairs f0 .. f0+B-1, on patch pyramids the corner blocks
// build themselves) | LK(pairs f0-B .. f0-1): 2B + 2 image sets, a pair done one tick earlier)
// so every stage consumes what earlier ticks wrote and the ticks are ordered by the stream.  Frame f lives in image set
// f mod (3B+2) and pair p's shift vectors in slot p mod 2B: a set is last read by LK(pair f+1), at the latest in the tick
// that starts with frame f+2B+1, and rewritten by the tick that holds frame f+3B+2; a slot is read by LK(pair p) one tick
// after the corner stage wrote it and rewritten two ticks after.  The flows of pair p go to flow set p mod B.  After a
// tick every pair <= f0-B-1 is done.

// One launch composing pairs first .. last (the pairs a call of the pipeline completes) into their ring slots.
static int compose_ring(ofx_session *s, long first, long last, void *stream)
{
    const int B = stream_batch_of(s), lv = s->ring_level;
    ofx_ring::OutRing &ring = s->out[ofx_session::RING_COMPOSE];
    static thread_local ofx_compose_batch cb; // (1.7 KB)
    memset(&cb, 0, sizeof cb);
    cb.w = s->w[lv];
    cb.rows = s->own1[lv] - s->own0[lv];
    cb.n_px = (unsigned)((size_t)cb.w * (size_t)cb.rows);
    cb.levels = s->p.levels;
    cb.level = lv;
    for (int k = 0; k < s->p.levels; ++k) cb.own0[k] = s->own0[k];
    for (long p = first; p <= last; ++p, ++cb.n) {
        for (int k = lv; k < s->p.levels; ++k) cb.lv[cb.n][k] = s->flowset[p % B][k] + s->flow_own_offset(k);
        cb.dst[cb.n] = reinterpret_cast<float *>(ring.slot(p));
    }
    ring.newest = last;
    return timed_launch(s, OFX_TIME_COMPOSE, stream, [&] { return ofx_compose_batch_launch(&cb, stream); });
}

// One launch sampling pairs first .. last: their arrow fields into the arrow ring, the tracked points through them in order.
static int sample_ring(ofx_session *s, long first, long last, void *stream)
{
    const int B = stream_batch_of(s);
    ofx_ring::OutRing &arrows = s->out[ofx_session::RING_ARROWS], &hist = s->out[ofx_session::RING_TRACKS];
    static thread_local ofx_sample_batch sb; // (2 KB)
    memset(&sb, 0, sizeof sb);
    sb.levels = s->p.levels;
    for (int k = 0; k < s->p.levels; ++k) sb.own0[k] = s->own0[k];
    if (arrows.on()) {
        sb.a_level = s->arrow_level, sb.a_w = s->w[s->arrow_level], sb.a_h = s->h[s->arrow_level];
        sb.a_offset = s->arrow_offset, sb.a_ny = s->arrow_ny, sb.a_nx = s->arrow_nx;
    }
    if (s->trk_points) {
        sb.points = s->trk_points, sb.status = s->trk_status, sb.n_points = s->trk_n;
        sb.t_level = s->trk_level, sb.t_w = s->w[s->trk_level], sb.t_h = s->h[s->trk_level];
        sb.pair0 = (int)first;
    }
    for (long p = first; p <= last; ++p, ++sb.n) {
        for (int k = 0; k < s->p.levels; ++k) sb.lv[sb.n][k] = s->flowset[p % B][k] + s->flow_own_offset(k);
        if (arrows.on()) sb.arrows[sb.n] = reinterpret_cast<int32_t *>(arrows.slot(p));
        if (s->trk_points && hist.on()) sb.hist[sb.n] = reinterpret_cast<float *>(hist.slot(p));
    }
    arrows.newest = hist.newest = last; // (the stage's one counter, whichever of the two is on)
    OfxRange range("ofx.sample_ring");
    return ofx_sample_batch_launch(&sb, stream);
}

// What the stages of one tick share: the tick's place in the stream and how a frame or a pair maps to the session's storage.
struct Tick {
    ofx_session *s;
    // D = ticks between a frame's arrival and the LK stage of the pair it completes: 2 (pyramid | corner | LK), or 1 with
    // stream_two_stage (the corner stage runs in the frame's own tick, on patch pyramids it builds itself)
    int B, D, sets, slots, L;
    long f0, last_frame; // the first frame of this tick; the last frame the stream has (so far)
    int set_of(long frame) const { return (int)(frame % sets); }
    float *uvslot(long pair) const { return s->uv + (size_t)(pair % slots) * 2 * OFX_MAX_LEVELS; }
    float *flow_in(int set, int b, int k) const { return (set ? s->flowset2 : s->flowset)[b][k]; }
    // level k of a frame as the LK / corner stages see it: the session's plane, or (borrow_frames, level 0) the caller's buffer
    const uint8_t *plane_of(long frame, int k) const
    {
        const int set = set_of(frame);
        return k == 0 && s->p.borrow_frames ? s->bframe[set] + (size_t)s->buf0[0] * (size_t)s->bpitch[set] : s->img[set][k];
    }
    const uint8_t *patch_of(long frame, int k) const { return k == 0 && s->p.borrow_frames ? s->bframe[set_of(frame)] : s->pimg[set_of(frame)][k]; }
    int pitch_of(long frame, int k, bool patch) const { return k == 0 && s->p.borrow_frames ? s->bpitch[set_of(frame)] : patch ? s->ppitch[k] : s->pitch[k]; }
    // columns / rows of level k's patch planes the corner chain may read (all of them, unless the test hook narrows them)
    int chain_extent(int k, int full) const
    {
        if (s->debug_extent <= 0 || k == 0) return full;
        const int need = (s->p.window >> 1) + 2, lim = s->debug_extent >> k;
        const int e = lim > need ? lim : need;
        return e < full ? e : full;
    }
    // the pairs whose LK stage (iteration 1) and further iterations this tick runs: the B pairs from f0 - D B on, clipped to those
    // that exist (1 .. last_frame).  false (and -1, -1): none
    bool lk_pairs(long *first, long *last) const
    {
        const long a = f0 - (long)D * B, e = a + B - 1;
        *first = a < 1 ? 1 : a, *last = e > last_frame ? last_frame : e;
        if (*first > *last) *first = *last = -1;
        return *last >= 1;
    }
};

// One launch for pairs first .. last (the pairs a call of the pipeline completes): each pair's motion-compensated next image into
// its ring slot and its four sums into its stats slot (ofx_session_stream_motion).  Reads what the call's own LK stage read -- both
// frames' planes of the level, each with the pitch its frame came with, and the pair's shift vector -- and the final flow (flowset: the last
// launch of a tick always writes it, whichever set the tick started in).
static int motion_ring(const Tick &t, long first, long last, void *stream)
{
    ofx_session *s = t.s;
    const int lv = s->mc_level;
    ofx_ring::OutRing &ring = s->out[ofx_session::RING_MOTION];
    static thread_local ofx_motion_batch mb; // (1 KB)
    memset(&mb, 0, sizeof mb);
    mb.w = s->w[lv], mb.h = s->h[lv], mb.scale = s->mc_scale;
    mb.dst_pitch = s->mc_pitch, mb.dst_dwords = 1; // (ofx_session_stream_motion checked the alignment)
    for (long p = first; p <= last; ++p, ++mb.n) {
        mb.prev[mb.n] = t.plane_of(p - 1, lv), mb.prev_pitch[mb.n] = t.pitch_of(p - 1, lv, false);
        mb.next[mb.n] = t.plane_of(p, lv), mb.next_pitch[mb.n] = t.pitch_of(p, lv, false);
        mb.flow[mb.n] = s->flowset[p % t.B][lv];
        mb.uv[mb.n] = lv == t.L - 1 ? nullptr : t.uvslot(p) + 2 * lv; // (the coarsest level is not shifted)
        if (ring.on()) mb.dst[mb.n] = reinterpret_cast<uint8_t *>(ring.slot(p));
        if (s->mc_stats) mb.stats[mb.n] = reinterpret_cast<unsigned long long *>(s->mc_stats + 4 * ring.index(p));
    }
    {
        OfxRange range("ofx.motion_ring");
        OFX_TRY(ofx_motion_batch_launch(&mb, stream)); // (zeroes the pairs' stats slots, then the one kernel launch)
    }
    ring.newest = last;
    return OFX_OK;
}

// One launch for pairs first .. last: each pair's pixel displacement at the stage's level into its ring slot
// (ofx_session_stream_displacement).  Reads the pair's shift vector and the final flow, as motion_ring does.
static int displacement_ring(const Tick &t, long first, long last, void *stream)
{
    ofx_session *s = t.s;
    const int lv = s->disp_level;
    static thread_local ofx_displacement_batch db;
    memset(&db, 0, sizeof db);
    db.w = s->w[lv], db.h = s->h[lv], db.scale = s->disp_scale;
    for (long p = first; p <= last; ++p, ++db.n) {
        db.flow[db.n] = s->flowset[p % t.B][lv];
        db.uv[db.n] = lv == t.L - 1 ? nullptr : t.uvslot(p) + 2 * lv; // (the coarsest level is not shifted)
        db.dst[db.n] = reinterpret_cast<float *>(s->out[ofx_session::RING_DISP].slot(p));
    }
    {
        OfxRange range("ofx.displacement_ring");
        OFX_TRY(ofx_displacement_batch_launch(&db, stream));
    }
    s->out[ofx_session::RING_DISP].newest = last;
    return OFX_OK;
}

// pyramid(frame f0 + i) for the tick's frames
static int pyramid_stages(const Tick &t, const uint8_t *const *frames, const int *pitches, int n_frames, ofx_stream_stages &g)
{
    ofx_session *s = t.s;
    for (int i = 0; i < n_frames; ++i) {
        OFX_REQUIRE(pitches[i] >= s->w[0] && (pitches[i] & 3) == 0 && ((uintptr_t)frames[i] & 3) == 0,
                    "ofx_session_stream_submit: frame must be 4-byte aligned with a pitch multiple of 4 and >= width");
        if (s->p.borrow_frames && t.f0 + i >= 1)
            OFX_REQUIRE(pitches[i] == s->bpitch[t.set_of(t.f0 + i - 1)] || (i > 0 && pitches[i] == pitches[i - 1]),
                        "ofx_session_stream_submit: borrowed frames must all have the same pitch");
        ofx_pyramid_stage &P = g.pyr[g.n_pyr++];
        const int set = t.set_of(t.f0 + i);
        P.d_frame = frames[i];
        P.frame_pitch = pitches[i];
        P.w = s->w[0];
        P.h = s->h[0];
        P.levels = t.L;
        P.windowed = s->p.sharded ? 1 : 0;
        for (int k = 0; k < t.L; ++k) {
            P.d_levels[k] = s->img[set][k];
            P.pitches[k] = s->pitch[k];
            P.row0[k] = s->buf0[k];
            P.rows[k] = s->buf1[k] - s->buf0[k];
        }
        if (s->p.local_corner && t.D == 2) { // the same frame's top-left patch, as a pyramid of its own
            P.patch_w = s->pw[0];
            P.patch_h = s->ph[0];
            P.patch_levels = t.L;
            for (int k = 0; k < t.L; ++k) {
                P.d_patch_levels[k] = s->pimg[set][k];
                P.patch_pitches[k] = s->ppitch[k];
            }
        }
        if (s->p.borrow_frames) { // no copies of level 0: the later stages read the caller's buffer
            s->bframe[set] = frames[i];
            s->bpitch[set] = pitches[i];
            P.d_levels[0] = nullptr;
            P.d_patch_levels[0] = nullptr;
        } else if (s->stream_input == 2) { // the front end wrote level 0 of the set itself (frontend_tick): nothing to copy
            P.d_levels[0] = nullptr;
        }
    }
    return OFX_OK;
}

// corner(pair pc), two stages: the pair's second frame arrived with this tick; the block builds the patch pyramids of both frames
// (levels >= 1) into its slot's planes and walks the chain on them (level 0: the frames themselves, borrowed)
static void corner_stage_two(const Tick &t, long pc, int slot_i, ofx_corner_stage &C)
{
    ofx_session *s = t.s;
    C.build_patch = 1;
    C.patch_w = s->pw[0];
    C.patch_h = s->ph[0];
    for (int f = 0; f < 2; ++f) {
        C.d_patch_src[f] = s->bframe[t.set_of(pc - 1 + f)];
        C.patch_src_pitch[f] = s->bpitch[t.set_of(pc - 1 + f)];
    }
    for (int k = 0; k < t.L; ++k) {
        C.patch_pitch[k] = s->ppitch[k];
        C.d_patch[0][k] = s->pscr[slot_i][0][k];
        C.d_patch[1][k] = s->pscr[slot_i][1][k];
        C.d_patch_reloc[k] = s->repair ? s->preloc[slot_i][k] : nullptr;
        const uint8_t *pp = k ? s->pscr[slot_i][0][k] : C.d_patch_src[0], *pn = k ? s->pscr[slot_i][1][k] : C.d_patch_src[1];
        // level 0 is the frames themselves, whole (every rank of a sharded stream is handed whole frames)
        ofx_geom pg{s->w[k], s->h[k], k ? s->ppitch[k] : C.patch_src_pitch[1], 0, k ? t.chain_extent(k, s->ph[k]) : s->h[0], 0,
                    k ? t.chain_extent(k, s->ph[k]) : s->h[0]};
        C.level[k] = ofx_lk_desc{pp, pn, pg, nullptr, 0, nullptr, 0, s->p.min_det};
        C.cols[k] = k ? t.chain_extent(k, s->pw[k]) : 0;
    }
}

// corner(pair pc), three stages: both pyramids are complete since the previous tick
static void corner_stage_three(const Tick &t, long pc, int slot_i, ofx_corner_stage &C)
{
    ofx_session *s = t.s;
    for (int k = 0; k < t.L; ++k) {
        // (both frames of a pair come through the same API with the same pitch; a borrowed level 0 uses the caller's)
        if (s->p.local_corner) {
            // (a borrowed level 0 is the whole frame: the chain may read all of it, and the repair rebuilds from it)
            const bool whole0 = k == 0 && s->p.borrow_frames && !s->p.frames_partial; // (partial frames: the patch's extent only)
            const int rows_k = whole0 ? s->h[0] : t.chain_extent(k, s->ph[k]);
            ofx_geom pg{s->w[k], s->h[k], t.pitch_of(pc, k, true), 0, rows_k, 0, rows_k};
            C.level[k] = ofx_lk_desc{t.patch_of(pc - 1, k), t.patch_of(pc, k), pg, nullptr, 0, nullptr, 0, s->p.min_det};
            C.cols[k] = whole0 ? 0 : t.chain_extent(k, s->pw[k]);
        } else {
            ofx_geom cg = level_geom(s, k, 0, s->h[k]);
            cg.pitch = t.pitch_of(pc, k, false);
            C.level[k] = ofx_lk_desc{t.plane_of(pc - 1, k), t.plane_of(pc, k), cg, nullptr, 0, nullptr, 0, s->p.min_det};
        }
    }
    if (s->p.local_corner && s->repair) {
        C.patch_w = s->pw[0];
        C.patch_h = s->ph[0];
        for (int k = 0; k < t.L; ++k) {
            C.patch_pitch[k] = s->ppitch[k];
            C.d_patch_reloc[k] = s->preloc[slot_i][k];
        }
    }
}

// corner(pairs f0 - (D - 1) B ..): their shift vectors, for the LK stage of the next tick
static void corner_stages(const Tick &t, ofx_stream_stages &g)
{
    ofx_session *s = t.s;
    for (long pc = t.f0 - (t.D - 1) * t.B; pc < t.f0 - (t.D - 2) * t.B; ++pc) {
        if (pc < 1 || pc > t.last_frame) continue;
        const int slot_i = g.n_corner;
        if (pc > s->corner_newest) s->corner_newest = pc;
        ofx_corner_stage &C = g.corner[g.n_corner++];
        C.levels = t.L;
        C.d_uv = t.uvslot(pc);
        C.d_pair_status = s->pair_status + (pc % t.slots);
        if (t.D == 1 || s->p.local_corner) { // the chain walks a patch: a shift that leaves it, or a shard's halo, is reported
            C.d_status = s->corner_status;
            if (s->p.sharded) shard_reach(s, C.shard_rows);
        }
        if (t.D == 1)
            corner_stage_two(t, pc, slot_i, C);
        else
            corner_stage_three(t, pc, slot_i, C);
    }
}

// LK(pairs first .. last): iteration 1 of each.  With fused iterations behind it, it is preceded by the launch that makes the
// globally shifted next images.
static int lk_stage(const Tick &t, long first, long last, ofx_stream_stages &g, void *stream)
{
    ofx_session *s = t.s;
    static thread_local ofx_shift_desc sd0[OFX_MAX_LK_ITEMS];
    const int set1 = s->n_iter_pass ? s->iter_plan[0].fin : 0; // the flow set the schedule of the iterations starts in
    int ns0 = 0;
    for (long pl = first; pl <= last; ++pl) {
        const int b = (int)(pl % t.B);
        // (the launches of the iterations address a level's planes -- the frame, read in place where it is borrowed, the shifted and
        // the warped image -- with ONE pitch, so borrowed frames must have the session's)
        if (s->p.iters > 1)
            OFX_REQUIRE(!s->p.borrow_frames || (t.pitch_of(pl, 0, false) == s->pitch[0] && t.pitch_of(pl - 1, 0, false) == s->pitch[0]),
                        "ofx_session_stream_submit: with refinement iterations borrowed frames need a row pitch of %d bytes (the "
                        "width rounded up to 64), got %d", s->pitch[0], t.pitch_of(pl, 0, false));
        for (int k = t.L - 1; k >= 0; --k) {
            ofx_geom lg = level_geom(s, k, s->fl0[k], s->fl1[k]); // (the own rows, unless iterations follow on a shard)
            lg.pitch = t.pitch_of(pl, k, false);
            ofx_lk_desc &d = g.lk[g.n_lk++];
            d = ofx_lk_desc{t.plane_of(pl - 1, k), t.plane_of(pl, k), lg, t.flow_in(set1, b, k), s->fl0[k],
                            k == t.L - 1 ? nullptr : t.uvslot(pl) + 2 * k, 0, s->p.min_det};
            if (s->fused_iters) {
                // refinement iterations follow (lk_body_warp.h): the LK stage is iteration 1 of the pair and also writes the warped
                // image of iteration 2, so the globally shifted next image (the warp's source) is made BEFORE the tick -- its
                // vectors are a tick old -- and the LK stage reads it as it is instead of shifting on the fly
                const uint8_t *src = d.d_next;
                if (k != t.L - 1) {
                    sd0[ns0++] = ofx_shift_desc{d.d_next, s->itsh[b][0][k], level_geom(s, k, s->buf0[k], s->buf1[k]), t.uvslot(pl) + 2 * k};
                    src = s->itsh[b][0][k];
                }
                d.d_next = src, d.d_uv = nullptr;
                d.d_warp_src = src, d.d_warp_out = s->itsh[b][1][k], d.warp_scale = OFX_ITER_SCALE;
                if (s->p.sharded) d.d_warp_status = s->corner_status, d.warp_status_bit = 16 + k; // (a tap row beyond the halo rows)
            }
        }
    }
    if (ns0) OFX_TRY(timed_launch(s, OFX_TIME_SHIFT, stream, [&] { return ofx_shift_levels(sd0, ns0, stream); }));
    return OFX_OK;
}

// Extension (lk_iter): the tick's LK stage was iteration 1 of its pairs.  Every further iteration is
// one warp launch and one accumulating LK launch over ALL levels of ALL those pairs (B x levels items: the strips are B
// times as tall as in the pair-at-a-time path), after one launch that materialises the globally shifted next images the
// warp reads.  Same arithmetic, same bits as ofx_session_run_flow with iters > 1.  Which launches there are, and the flow set
// and warped plane (itsh[b][1] / [2]) each reads and writes, is the session's schedule (iter_plan.h).
static int iter_passes(const Tick &t, long first, long last, void *stream)
{
    ofx_session *s = t.s;
    static thread_local ofx_shift_desc sd[OFX_MAX_LK_ITEMS];
    static thread_local ofx_warp_desc wd[OFX_MAX_LK_ITEMS];
    static thread_local ofx_lk_desc ld[OFX_MAX_LK_ITEMS];
    static thread_local const float *fin[OFX_MAX_LK_ITEMS];
    const int reach = s->p.window / 2 + 1;
    auto clip = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    for (int i = 0; i < s->n_iter_pass; ++i) {
        const ofx_plan::IterPass &q = s->iter_plan[i];
        int ns = 0, nw = 0;
        for (long pl = first; pl <= last; ++pl) {
            const int b = (int)(pl % t.B);
            for (int k = t.L - 1; k >= 0; --k) {
                // rows of this iteration on a shard: the own rows + (radius + 1) * (iters - 1 - it) either side, so that the
                // next warp finds the flow of every row its LK touches (whole levels: everything)
                const int ext = s->p.sharded ? reach * (s->p.iters - 1 - q.it) : 0;
                const int a = clip(s->own0[k] - ext, 0, s->h[k]), e = clip(s->own1[k] + ext, 0, s->h[k]);
                const int wa = clip(a - reach, s->buf0[k], s->buf1[k]), we = clip(e + reach, s->buf0[k], s->buf1[k]);
                const uint8_t *next_k = t.plane_of(pl, k);
                const uint8_t *src = next_k;
                if (k != t.L - 1) {
                    // the globally shifted next image, every row the buffers hold (once per pair, before iteration 2)
                    if (q.shift) sd[ns++] = ofx_shift_desc{next_k, s->itsh[b][0][k], level_geom(s, k, s->buf0[k], s->buf1[k]), t.uvslot(pl) + 2 * k};
                    src = s->itsh[b][0][k];
                }
                float *const fcur = t.flow_in(q.fin, b, k);
                uint8_t *const warped = s->itsh[b][1 + q.win][k];
                wd[nw] = ofx_warp_desc{src, warped, level_geom(s, k, wa, we), fcur, s->fl0[k], OFX_ITER_SCALE,
                                       s->p.sharded ? s->corner_status : nullptr, 16 + k};
                ld[nw] = ofx_lk_desc{t.plane_of(pl - 1, k), warped, level_geom(s, k, a, e), fcur, s->fl0[k], nullptr, 1, s->p.min_det};
                if (q.count == 2) { // reads fcur, writes the slot's other set; its first iteration's warp needs the source either way
                    fin[nw] = fcur;
                    ld[nw].d_flow = t.flow_in(q.fout, b, k);
                    ld[nw].d_warp_src = src, ld[nw].warp_scale = OFX_ITER_SCALE;
                }
                if (q.wout) {
                    ld[nw].d_warp_src = src, ld[nw].d_warp_out = s->itsh[b][1 + q.wo][k], ld[nw].warp_scale = OFX_ITER_SCALE;
                    if (s->p.sharded) ld[nw].d_warp_status = s->corner_status, ld[nw].warp_status_bit = 16 + k;
                }
                ++nw;
            }
        }
        if (ns) OFX_TRY(timed_launch(s, OFX_TIME_SHIFT, stream, [&] { return ofx_shift_levels(sd, ns, stream); }));
        if (q.warp) OFX_TRY(timed_launch(s, OFX_TIME_WARP, stream, [&] { return ofx_warp_levels(wd, nw, stream); }));
        OFX_TRY(timed_launch(s, q.wout ? OFX_TIME_LK_ACC_WARP : OFX_TIME_LK_ACC, stream, [&] {
            return q.count == 2 ? ofx_lk_levels_pair(ld, fin, nw, s->p.window, s->p.mode, &s->pair_opts, stream)
                                : ofx_lk_levels(ld, nw, s->p.window, s->p.mode, stream);
        }));
    }
    return OFX_OK;
}

// One tick: the launches it puts on the stream, in order.
static int stream_tick(ofx_session *s, const uint8_t *const *frames, const int *pitches, int n_frames, void *stream, int *completed_pair)
{
    const int B = stream_batch_of(s), D = s->p.stream_two_stage ? 1 : 2;
    const Tick t{s, B, D, stream_sets(s), 2 * B, s->p.levels, s->stream_n, s->stream_frames >= 0 ? s->stream_frames - 1 : s->stream_n + n_frames - 1};
    // the stages struct is several KB: keep it off the stack of callers with small stacks
    static thread_local ofx_stream_stages g;
    memset(&g, 0, sizeof g);
    OFX_TRY(pyramid_stages(t, frames, pitches, n_frames, g));
    corner_stages(t, g);
    long oldest, newest; // the pairs this call completes: oldest .. newest (-1: none)
    if (t.lk_pairs(&oldest, &newest)) OFX_TRY(lk_stage(t, oldest, newest, g, stream)); // (fused iterations: the shift launch)
    *completed_pair = -1;
    if (newest > s->reported) {
        *completed_pair = (int)newest;
        s->reported = newest;
        for (int k = 0; k < t.L; ++k) s->flow[k] = s->flowset[newest % t.B][k];
    }
    bool time_it = g.n_lk > 0;
    g.deep_fetch = s->p.deep_fetch; // (ofx_params.deep_fetch: where the caller's frames come from)
#ifdef OFX_EXPERIMENTS
    // stage ablation for timing experiments (tools/stream_timeline.py): the flows reported complete are then NOT computed, so
    // the knob only exists in builds made with -DOFX_EXPERIMENTS (OFX_BUILD_DEFS)
    static const int skip = [] { const char *e = getenv("OFX_STREAM_SKIP"); return e ? atoi(e) : 0; }();
    if (skip & 1) g.n_pyr = 0;
    if (skip & 2) g.n_corner = 0;
    if (skip & 8) g.n_lk = 0;
    time_it = time_it || (skip & 8);
#endif
    // the tick itself: pyramid | corner | LK side by side in one grid
    if (time_it)
        OFX_TRY(timed_launch(s, OFX_TIME_STREAM, stream, [&] { return ofx_stream_launch(&g, s->p.window, s->p.mode, stream); }));
    else
        OFX_TRY(ofx_stream_launch(&g, s->p.window, s->p.mode, stream));
    // iterations 2 .. iters of the tick's pairs
    if (newest >= 1) OFX_TRY(iter_passes(t, oldest, newest, stream));
    // the output stage (ofx_session_stream_compose): behind the tick's last launch on the same stream, before the next tick
    // rewrites flow set p mod B
    if (s->out[ofx_session::RING_COMPOSE].on() && newest >= 1) OFX_TRY(compose_ring(s, oldest, newest, stream));
    // the sampled output stage (ofx_session_stream_arrows / _stream_tracks): one launch, under the same rule
    if ((s->out[ofx_session::RING_ARROWS].on() || s->trk_points) && newest >= 1) OFX_TRY(sample_ring(s, oldest, newest, stream));
    // the motion-compensation stage (ofx_session_stream_motion): one launch, under the same rule
    if (s->motion_on() && newest >= 1) OFX_TRY(motion_ring(t, oldest, newest, stream));
    // the displacement stage (ofx_session_stream_displacement): one launch, under the same rule
    if (s->out[ofx_session::RING_DISP].on() && newest >= 1) OFX_TRY(displacement_ring(t, oldest, newest, stream));
    s->stream_n = t.f0 + t.B;
    return OFX_OK;
}

extern "C" int ofx_session_stream_begin(ofx_session *s)
{
    OFX_REQUIRE(s, "ofx_session_stream_begin: null session");
    OFX_REQUIRE(!s->p.sharded || s->p.local_corner,
                "ofx_session_stream_begin: on a sharded session the stream pipeline needs local_corner (the corner flows "
                "computed from each frame's top-left patch); otherwise drive the staged API");
    OFX_REQUIRE(s->p.levels >= 2 && s->p.levels - 1 <= 6, "ofx_session_stream_begin: %d levels unsupported (2..7)", s->p.levels);
    // staging work of the pair-at-a-time pipelined path may still be in flight on the session's own stream; the stream
    // pipeline is about to reuse the same image sets from the caller's stream
    if (s->aux) OFX_HIP(hipStreamSynchronize(s->aux));
    for (bool &b : s->set_busy) b = false;
    s->stream_n = 0;
    s->stream_frames = -1;
    s->n_held = 0;
    s->reported = 0;
    s->corner_newest = 0;
    for (ofx_ring::OutRing &r : s->out) r.reset();
    s->stream_input = 0;
    s->have_prev = s->have_next = s->staged = false;
    for (int k = 0; k < s->p.levels; ++k) s->flow[k] = s->flowset[0][k];
    return OFX_OK;
}

// A tick of colour frames: ONE front-end launch writes the filtered planes of the tick's frames (the sets they are assigned to,
// frame f -> set f mod stream_sets), then the tick runs on those planes as its frames.
static int frontend_tick(ofx_session *s, const uint8_t *const *img3, const int *pitch3, int n, void *stream, int *completed_pair)
{
    const uint8_t *fr[kMaxBatch];
    int pt[kMaxBatch];
    if (n > 0) {
        uint8_t *dst[kMaxBatch];
        int dp[kMaxBatch], md[kMaxBatch];
        const int sets = stream_sets(s);
        for (int i = 0; i < n; ++i) {
            const long f = s->stream_n + i;
            dst[i] = s->p.borrow_frames ? s->fplane[f % sets] : s->img[f % sets][0];
            dp[i] = s->pitch[0];
            md[i] = f == 0 && (s->fe_flags & OFX_FRONTEND_FLAG_FIRST_GREY) ? OFX_FRONTEND_GREY : s->fe_mode;
            fr[i] = dst[i];
            pt[i] = s->pitch[0];
        }
        OfxRange range("ofx.frontend");
        OFX_TRY(ofx_frontend_run(s->fe, img3, pitch3, dst, dp, md, n, s->w[0], s->h[0], ofx_stream(stream)));
    }
    return stream_tick(s, fr, pt, n, stream, completed_pair);
}

// Submit the next frame of the stream (input 1: a grey frame, 2: a colour frame for the front end).  *completed_pair (may be
// NULL) receives the highest pair (frame p-1 -> frame p, frames counted from 0) whose flow is complete after this call in `stream`
// order, or -1 when the call completed none.
static int stream_submit(ofx_session *s, const uint8_t *frame, int pitch, void *stream, int *completed_pair, int input, const char *who)
{
    OFX_REQUIRE(s && frame, "%s: null argument", who);
    if (s->stream_n < 0) {
        ofx_set_error("%s: call ofx_session_stream_begin first", who);
        return OFX_E_STATE;
    }
    OFX_REQUIRE(s->stream_frames < 0, "%s: the stream is being drained", who);
    if (input == 2 && !s->fe_mode) {
        ofx_set_error("%s: colour frames need the front end (ofx_session_stream_frontend)", who);
        return OFX_E_STATE;
    }
    if (s->stream_input != 0 && s->stream_input != input) {
        ofx_set_error("%s: this stream has received %s frames; a stream takes grey frames or colour frames, not both", who,
                      s->stream_input == 1 ? "grey" : "colour");
        return OFX_E_STATE;
    }
    if (input == 2)
        OFX_REQUIRE(pitch >= 3 * s->w[0] && ((uintptr_t)frame & 3) == 0,
                    "%s: a colour frame must be 4-byte aligned with a pitch of at least 3 * %d bytes (got %d)", who, s->w[0], pitch);
    s->stream_input = input;
    int dummy = -1;
    if (!completed_pair) completed_pair = &dummy;
    const int B = stream_batch_of(s);
    if (s->n_held + 1 < B) { // the tick is not full yet: remember the frame
        s->held_frame[s->n_held] = frame;
        s->held_pitch[s->n_held] = pitch;
        ++s->n_held;
        *completed_pair = -1;
        return OFX_OK;
    }
    const uint8_t *fr[kMaxBatch];
    int pt[kMaxBatch];
    for (int i = 0; i < s->n_held; ++i) fr[i] = s->held_frame[i], pt[i] = s->held_pitch[i];
    fr[s->n_held] = frame;
    pt[s->n_held] = pitch;
    const int n = s->n_held + 1;
    s->n_held = 0;
    return input == 2 ? frontend_tick(s, fr, pt, n, stream, completed_pair) : stream_tick(s, fr, pt, n, stream, completed_pair);
}

extern "C" int ofx_session_stream_submit(ofx_session *s, const uint8_t *d_gray1, int pitch, void *stream, int *completed_pair)
{
    return stream_submit(s, d_gray1, pitch, stream, completed_pair, 1, "ofx_session_stream_submit");
}

extern "C" int ofx_session_stream_submit_3ch(ofx_session *s, const uint8_t *d_img3, int pitch, void *stream, int *completed_pair)
{
    return stream_submit(s, d_img3, pitch, stream, completed_pair, 2, "ofx_session_stream_submit_3ch");
}

extern "C" int ofx_session_stream_submit_frames_3ch(ofx_session *s, const uint8_t *const *d_img3, const int *pitches, int pitch0, int n,
                                                    void *stream, int *completed_pair)
{
    OFX_REQUIRE(s && d_img3 && n >= 1, "ofx_session_stream_submit_frames_3ch: bad arguments");
    int newest = -1;
    for (int i = 0; i < n; ++i) {
        int done = -1;
        OFX_TRY(ofx_session_stream_submit_3ch(s, d_img3[i], pitches ? pitches[i] : pitch0, stream, &done));
        newest = done > newest ? done : newest;
    }
    if (completed_pair) *completed_pair = newest;
    return OFX_OK;
}

extern "C" int ofx_session_stream_frontend(ofx_session *s, int mode, int window, double sigma_s, double sigma_b, int flags)
{
    OFX_REQUIRE(s, "ofx_session_stream_frontend: null session");
    if (s->p.sharded) {
        ofx_set_error("ofx_session_stream_frontend: not on a sharded session (each rank would filter the whole frame)");
        return OFX_E_UNSUPPORTED;
    }
    if (s->stream_n > 0 || s->n_held > 0) {
        ofx_set_error("ofx_session_stream_frontend: the stream has frames already; set the front end before the first frame of a stream");
        return OFX_E_STATE;
    }
    OFX_REQUIRE(mode == OFX_FRONTEND_OFF || mode == OFX_FRONTEND_GREY || mode == OFX_FRONTEND_BILATERAL,
                "ofx_session_stream_frontend: mode %d (OFX_FRONTEND_OFF / _GREY / _BILATERAL)", mode);
    OFX_REQUIRE((flags & ~(OFX_FRONTEND_FLAG_FAST | OFX_FRONTEND_FLAG_FIRST_GREY)) == 0, "ofx_session_stream_frontend: unknown flags %#x", flags);
    OFX_HIP(hipSetDevice(s->p.device));
    if (mode == OFX_FRONTEND_OFF) {
        ofx_frontend_tables_free(s->fe);
        s->fe = nullptr;
        s->fe_mode = s->fe_flags = 0;
        for (uint8_t *&pl : s->fplane) pl = nullptr;
        void *a = s->fe_arena;
        s->fe_arena = nullptr;
        if (a) OFX_HIP(hipFree(a));
        return OFX_OK;
    }
    ofx_frontend_tables *t = nullptr;
    OFX_TRY(ofx_frontend_tables_make(mode == OFX_FRONTEND_BILATERAL ? window : 0, sigma_s, sigma_b, &t));
    if (s->p.borrow_frames && !s->fe_arena) {
        // one plane per image set at the level-0 pitch, plus the three readable bytes the fused warp may fetch past level 0
        const size_t plane = ofx_plan::plane_bytes(s->pitch[0], s->h[0]);
        const hipError_t e = hipMalloc(&s->fe_arena, plane * (size_t)s->n_sets);
        if (e != hipSuccess) {
            ofx_frontend_tables_free(t);
            s->fe_arena = nullptr;
            ofx_set_error("ofx_session_stream_frontend: hipMalloc(%zu bytes): %s", plane * (size_t)s->n_sets, hipGetErrorString(e));
            return OFX_E_HIP;
        }
        for (int i = 0; i < s->n_sets; ++i) s->fplane[i] = static_cast<uint8_t *>(s->fe_arena) + plane * (size_t)i;
    }
    ofx_frontend_tables_free(s->fe);
    s->fe = t;
    s->fe_mode = mode == OFX_FRONTEND_GREY ? OFX_FRONTEND_GREY : (flags & OFX_FRONTEND_FLAG_FAST) ? OFX_FRONTEND_BILATERAL_FAST : OFX_FRONTEND_BILATERAL;
    s->fe_flags = flags;
    return OFX_OK;
}

extern "C" int ofx_session_stream_submit_frames(ofx_session *s, const uint8_t *const *d_gray1, const int *pitches, int pitch0, int n,
                                                void *stream, int *completed_pair)
{
    OFX_REQUIRE(s && d_gray1 && n >= 1, "ofx_session_stream_submit_frames: bad arguments");
    int newest = -1;
    for (int i = 0; i < n; ++i) {
        int done = -1;
        OFX_TRY(ofx_session_stream_submit(s, d_gray1[i], pitches ? pitches[i] : pitch0, stream, &done));
        newest = done > newest ? done : newest;
    }
    if (completed_pair) *completed_pair = newest;
    return OFX_OK;
}

// Run one more tick without a new frame (frames still waiting for their tick to fill go out with it); call until it
// reports -2 in *completed_pair (pipeline empty).  Two ticks drain a full pipeline.
extern "C" int ofx_session_stream_drain(ofx_session *s, void *stream, int *completed_pair)
{
    OFX_REQUIRE(s && completed_pair, "ofx_session_stream_drain: null argument");
    if (s->stream_n < 0) {
        ofx_set_error("ofx_session_stream_drain: not streaming");
        return OFX_E_STATE;
    }
    const uint8_t *fr[kMaxBatch];
    int pt[kMaxBatch];
    const int n = s->n_held;
    for (int i = 0; i < n; ++i) fr[i] = s->held_frame[i], pt[i] = s->held_pitch[i];
    s->n_held = 0;
    if (s->stream_frames < 0) s->stream_frames = s->stream_n + n; // number of frames the stream received
    if (n == 0 && s->reported >= s->stream_frames - 1) { // every pair (the last one is stream_frames - 1) has been reported
        *completed_pair = -2;
        s->stream_n = -1;
        s->stream_frames = -1;
        return OFX_OK;
    }
    return s->stream_input == 2 ? frontend_tick(s, fr, pt, n, stream, completed_pair) : stream_tick(s, fr, pt, n, stream, completed_pair);
}

extern "C" int ofx_session_flow_of(ofx_session *s, int pair, int level, float **d_ptr, int *row0, int *rows)
{
    OFX_REQUIRE(s && level >= 0 && level < s->p.levels, "ofx_session_flow_of: bad arguments");
    const int B = stream_batch_of(s);
    OFX_REQUIRE(pair >= 1 && pair <= s->reported && pair > s->reported - B,
                "ofx_session_flow_of: pair %d is not among the newest %d completed pairs (newest: %ld)", pair, B, s->reported);
    if (d_ptr) *d_ptr = s->flowset[pair % B][level] + s->flow_own_offset(level);
    if (row0) *row0 = s->own0[level];
    if (rows) *rows = s->own1[level] - s->own0[level];
    return OFX_OK;
}

// ---- the ring outputs (out_ring.h) ---------------------------------------------------------------------------------------------
// What every setter of an output stage asks first: an output is set before the first frame of a stream.
static int output_settable(const ofx_session *s, const char *who)
{
    if (s->stream_n > 0 || s->n_held > 0) {
        ofx_set_error("%s: the stream has frames already; set the output before the first frame of a stream", who);
        return OFX_E_STATE;
    }
    return OFX_OK;
}

// ... and of the caller's ring: a slot for each pair one call completes, 16-byte aligned, slots a multiple of 16 bytes apart that hold
// slot_bytes each
static int ring_fits(const ofx_session *s, const void *ring, size_t stride, size_t slot_bytes, int n_slots, const char *who)
{
    const int B = stream_batch_of(s);
    OFX_REQUIRE(n_slots >= B, "%s: %d slots, the ring needs at least stream_batch = %d (the pairs one call completes)", who, n_slots, B);
    OFX_REQUIRE(((uintptr_t)ring & 15) == 0, "%s: the ring must be 16-byte aligned", who);
    OFX_REQUIRE(stride % 16 == 0 && stride >= slot_bytes, "%s: slot stride %zu bytes must be a multiple of 16 and at least the slot's %zu bytes", who,
                stride, slot_bytes);
    return OFX_OK;
}

extern "C" int ofx_session_stream_compose(ofx_session *s, int level, float *d_ring, size_t slot_stride_bytes, int n_slots)
{
    const char *who = "ofx_session_stream_compose";
    OFX_REQUIRE(s, "%s: null session", who);
    OFX_TRY(output_settable(s, who));
    if (!d_ring) {
        s->out[ofx_session::RING_COMPOSE].set(nullptr, 0, 0);
        return OFX_OK;
    }
    OFX_REQUIRE(level >= 0 && level < s->p.levels, "%s: level %d out of range (0 .. %d)", who, level, s->p.levels - 1);
    const size_t slot_bytes = (size_t)(s->own1[level] - s->own0[level]) * (size_t)s->w[level] * 2 * sizeof(float);
    OFX_TRY(ring_fits(s, d_ring, slot_stride_bytes, slot_bytes, n_slots, who));
    if (slot_bytes / 8 >= ((size_t)1 << 31)) {
        ofx_set_error("ofx_session_stream_compose: a slot of %zu pixels is more than this build composes (2^31)", slot_bytes / 8);
        return OFX_E_UNSUPPORTED;
    }
    // a rank composes its own rows: own row y at `level` reads row y >> (k - level) of level k, which must be one of the rows the
    // rank computes there (ShardPlan's rows are the coarsest level's, doubled per level)
    for (int k = level + 1; k < s->p.levels && s->own1[level] > s->own0[level]; ++k) {
        const int sc = k - level;
        if ((s->own0[level] >> sc) < s->own0[k] || ((s->own1[level] - 1) >> sc) >= s->own1[k]) {
            ofx_set_error("ofx_session_stream_compose: own rows [%d,%d) of level %d read rows [%d,%d] of level %d, which owns [%d,%d)", s->own0[level],
                          s->own1[level], level, s->own0[level] >> sc, (s->own1[level] - 1) >> sc, k, s->own0[k], s->own1[k]);
            return OFX_E_UNSUPPORTED;
        }
    }
    s->out[ofx_session::RING_COMPOSE].set(d_ring, slot_stride_bytes, n_slots);
    s->ring_level = level;
    return OFX_OK;
}

extern "C" int ofx_session_composed_of(ofx_session *s, int pair, float **d_ptr, int *row0, int *rows)
{
    OFX_REQUIRE(s, "ofx_session_composed_of: null session");
    const ofx_ring::OutRing &ring = s->out[ofx_session::RING_COMPOSE];
    if (!ring.on()) {
        ofx_set_error("ofx_session_composed_of: no ring set (ofx_session_stream_compose)");
        return OFX_E_STATE;
    }
    OFX_REQUIRE(ring.holds(pair), "ofx_session_composed_of: pair %d is not among the newest %d composed pairs (newest: %ld)", pair, ring.slots,
                ring.newest);
    const int lv = s->ring_level;
    if (d_ptr) *d_ptr = reinterpret_cast<float *>(ring.slot(pair));
    if (row0) *row0 = s->own0[lv];
    if (rows) *rows = s->own1[lv] - s->own0[lv];
    return OFX_OK;
}

// what ofx_session_stream_arrows / _stream_tracks share: the session may take a new output setting
static int sampled_settable(ofx_session *s, const char *who)
{
    OFX_TRY(output_settable(s, who));
    if (s->p.sharded) {
        ofx_set_error("%s: not on a sharded session (sampled positions cross shard boundaries)", who);
        return OFX_E_UNSUPPORTED;
    }
    return OFX_OK;
}

extern "C" int ofx_session_stream_arrows(ofx_session *s, int level, int arrow_res, int32_t *d_ring, size_t slot_stride_bytes, int n_slots)
{
    const char *who = "ofx_session_stream_arrows";
    OFX_REQUIRE(s, "%s: null session", who);
    OFX_TRY(sampled_settable(s, who));
    if (!d_ring) {
        s->out[ofx_session::RING_ARROWS].set(nullptr, 0, 0);
        return OFX_OK;
    }
    OFX_REQUIRE(level >= 0 && level < s->p.levels, "%s: level %d out of range (0 .. %d)", who, level, s->p.levels - 1);
    int offset, ny, nx;
    OFX_TRY(ofx_arrow_grid(s->w[level], s->h[level], arrow_res, &offset, &ny, &nx, who));
    OFX_TRY(ofx_check_sample_pyramid(s->w[level], s->h[level], s->p.levels, level, who));
    OFX_TRY(ring_fits(s, d_ring, slot_stride_bytes, (size_t)ny * (size_t)nx * 16, n_slots, who));
    s->out[ofx_session::RING_ARROWS].set(d_ring, slot_stride_bytes, n_slots);
    s->arrow_level = level;
    s->arrow_offset = offset, s->arrow_ny = ny, s->arrow_nx = nx;
    return OFX_OK;
}

extern "C" int ofx_session_arrows_of(ofx_session *s, int pair, int32_t **d_ptr, int *ny, int *nx)
{
    OFX_REQUIRE(s, "ofx_session_arrows_of: null session");
    const ofx_ring::OutRing &ring = s->out[ofx_session::RING_ARROWS];
    if (!ring.on()) {
        ofx_set_error("ofx_session_arrows_of: no ring set (ofx_session_stream_arrows)");
        return OFX_E_STATE;
    }
    OFX_REQUIRE(ring.holds(pair), "ofx_session_arrows_of: pair %d is not among the newest %d sampled pairs (newest: %ld)", pair, ring.slots, ring.newest);
    if (d_ptr) *d_ptr = reinterpret_cast<int32_t *>(ring.slot(pair));
    if (ny) *ny = s->arrow_ny;
    if (nx) *nx = s->arrow_nx;
    return OFX_OK;
}

extern "C" int ofx_session_stream_tracks(ofx_session *s, int level, float *d_points, int32_t *d_status, int n_points, float *d_history,
                                         size_t slot_stride_bytes, int n_slots)
{
    const char *who = "ofx_session_stream_tracks";
    OFX_REQUIRE(s, "%s: null session", who);
    OFX_TRY(sampled_settable(s, who));
    ofx_ring::OutRing &hist = s->out[ofx_session::RING_TRACKS];
    if (!d_points) { // (the arrows keep their counter)
        s->trk_points = nullptr, s->trk_status = nullptr;
        hist.set(nullptr, 0, 0);
        return OFX_OK;
    }
    OFX_REQUIRE(level >= 0 && level < s->p.levels, "%s: level %d out of range (0 .. %d)", who, level, s->p.levels - 1);
    OFX_REQUIRE(d_status && n_points >= 1, "%s: %d points need a status word each", who, n_points);
    OFX_REQUIRE(((uintptr_t)d_points & 7) == 0 && ((uintptr_t)d_status & 3) == 0, "%s: points must be 8-byte, statuses 4-byte aligned", who);
    OFX_TRY(ofx_check_sample_pyramid(s->w[level], s->h[level], s->p.levels, level, who));
    if (d_history) OFX_TRY(ring_fits(s, d_history, slot_stride_bytes, (size_t)n_points * 8, n_slots, who));
    s->trk_points = d_points;
    s->trk_status = d_status;
    s->trk_n = n_points;
    s->trk_level = level;
    hist.set(d_history, d_history ? slot_stride_bytes : 0, d_history ? n_slots : 0); // (optional)
    return OFX_OK;
}

extern "C" int ofx_session_stream_motion(ofx_session *s, int level, float scale, uint8_t *d_ring, int row_pitch, size_t slot_stride_bytes,
                                         int n_slots, int64_t *d_stats_ring)
{
    const char *who = "ofx_session_stream_motion";
    OFX_REQUIRE(s, "%s: null session", who);
    OFX_TRY(output_settable(s, who));
    if (!d_ring && !d_stats_ring) {
        s->out[ofx_session::RING_MOTION].set(nullptr, 0, 0);
        s->mc_stats = nullptr;
        return OFX_OK;
    }
    if (s->p.sharded || s->p.frames_partial) {
        ofx_set_error("%s: not on a sharded session or with partial frames (a warp crosses shard rows)", who);
        return OFX_E_UNSUPPORTED;
    }
    OFX_REQUIRE(level >= 0 && level < s->p.levels, "%s: level %d out of range (0 .. %d)", who, level, s->p.levels - 1);
    if (d_ring)
        OFX_REQUIRE(row_pitch >= s->w[level] && (row_pitch & 3) == 0, "%s: row pitch %d must be a multiple of 4 and at least the level's width %d", who,
                    row_pitch, s->w[level]);
    // (both rings have n_slots slots; without an image ring there is no stride to check)
    OFX_TRY(ring_fits(s, d_ring, d_ring ? slot_stride_bytes : 0, d_ring ? (size_t)s->h[level] * (size_t)row_pitch : 0, n_slots, who));
    OFX_REQUIRE(((uintptr_t)d_stats_ring & 7) == 0, "%s: the stats ring must be 8-byte aligned", who);
    s->out[ofx_session::RING_MOTION].set(d_ring, d_ring ? slot_stride_bytes : 0, n_slots);
    s->mc_stats = d_stats_ring;
    s->mc_pitch = d_ring ? row_pitch : 0;
    s->mc_level = level;
    s->mc_scale = scale;
    return OFX_OK;
}

extern "C" int ofx_session_motion_of(ofx_session *s, int pair, uint8_t **d_ptr, int *row_pitch, int64_t **d_stats)
{
    OFX_REQUIRE(s, "ofx_session_motion_of: null session");
    const ofx_ring::OutRing &ring = s->out[ofx_session::RING_MOTION];
    if (!s->motion_on()) {
        ofx_set_error("ofx_session_motion_of: the stage is off (ofx_session_stream_motion)");
        return OFX_E_STATE;
    }
    OFX_REQUIRE(ring.holds(pair), "ofx_session_motion_of: pair %d is not among the newest %d pairs of the stage (newest: %ld)", pair, ring.slots,
                ring.newest);
    if (d_ptr) *d_ptr = ring.on() ? reinterpret_cast<uint8_t *>(ring.slot(pair)) : nullptr;
    if (row_pitch) *row_pitch = s->mc_pitch;
    if (d_stats) *d_stats = s->mc_stats ? s->mc_stats + 4 * ring.index(pair) : nullptr;
    return OFX_OK;
}

extern "C" int ofx_session_stream_displacement(ofx_session *s, int level, float scale, float *d_ring, size_t slot_stride_bytes, int n_slots)
{
    const char *who = "ofx_session_stream_displacement";
    OFX_REQUIRE(s, "%s: null session", who);
    OFX_TRY(output_settable(s, who));
    if (!d_ring) {
        s->out[ofx_session::RING_DISP].set(nullptr, 0, 0);
        return OFX_OK;
    }
    if (s->p.sharded || s->p.frames_partial) {
        ofx_set_error("%s: not on a sharded session or with partial frames", who);
        return OFX_E_UNSUPPORTED;
    }
    OFX_REQUIRE(level >= 0 && level < s->p.levels, "%s: level %d out of range (0 .. %d)", who, level, s->p.levels - 1);
    OFX_REQUIRE(__builtin_isfinite(scale), "%s: the scale must be finite", who);
    OFX_TRY(ring_fits(s, d_ring, slot_stride_bytes, (size_t)s->h[level] * (size_t)s->w[level] * 8, n_slots, who));
    s->out[ofx_session::RING_DISP].set(d_ring, slot_stride_bytes, n_slots);
    s->disp_level = level;
    s->disp_scale = scale;
    return OFX_OK;
}

extern "C" int ofx_session_displacement_of(ofx_session *s, int pair, float **d_ptr)
{
    OFX_REQUIRE(s, "ofx_session_displacement_of: null session");
    const ofx_ring::OutRing &ring = s->out[ofx_session::RING_DISP];
    if (!ring.on()) {
        ofx_set_error("ofx_session_displacement_of: the stage is off (ofx_session_stream_displacement)");
        return OFX_E_STATE;
    }
    OFX_REQUIRE(ring.holds(pair), "ofx_session_displacement_of: pair %d is not among the newest %d pairs of the stage (newest: %ld)", pair, ring.slots,
                ring.newest);
    if (d_ptr) *d_ptr = reinterpret_cast<float *>(ring.slot(pair));
    return OFX_OK;
}
