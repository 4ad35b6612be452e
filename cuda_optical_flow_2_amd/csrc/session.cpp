// Device-resident session: the frame loop of main.cu:192-272 with every buffer living in HBM.
//
// One hipMalloc arena holds, per pyramid level: the previous and the next frame's 1-channel planes, a scratch
// plane for the shifted next frame, the flow field, and the 2-float shift vector.  Nothing is allocated or freed
// while frames flow (the reference does 58 cudaMalloc/cudaFree calls per level).  What the arena holds and where is the
// plan's (session_plan.h); ofx_session_create walks it.
#include <memory>
#include <new>

#include "compat_scratch.h"
#include "session.h"

static void repoint(ofx_session *s)
{
    for (int k = 0; k < s->p.levels; ++k) {
        s->plane[0][k] = s->img[s->cur][k];
        s->plane[1][k] = s->img[(s->cur + 1) % 3][k];
        s->plane[2][k] = s->sh[s->sht][k];
    }
    // borrowed frames: level 0 is the caller's buffer (same pitch as the session's plane; only ever read)
    const size_t skip = (size_t)s->buf0[0] * (size_t)s->pitch[0];
    if (s->pframe[s->cur]) s->plane[0][0] = const_cast<uint8_t *>(s->pframe[s->cur]) + skip;
    if (s->pframe[(s->cur + 1) % 3]) s->plane[1][0] = const_cast<uint8_t *>(s->pframe[(s->cur + 1) % 3]) + skip;
}

// The environment of a session (ofx_plan::SessionSwitches says what each switch does), read once per ofx_session_create.
static ofx_plan::SessionSwitches session_switches_from_env()
{
    auto env = [](const char *name, int dflt) {
        const char *e = getenv(name);
        return e ? atoi(e) : dflt;
    };
    ofx_plan::SessionSwitches sw;
    sw.iter_fused = env("OFX_ITER_FUSED", 1) != 0;
    sw.iter_pairs = env("OFX_ITER_PAIRS", sw.iter_pairs) != 0;
    sw.iter_dma = env("OFX_ITER_DMA", 0) > 0;
    sw.pair_pack = env("OFX_PAIR_PACK", 1) != 0;
    const int waves = env("OFX_PAIR_WAVES", 0);
    sw.pair_waves = waves > 0 ? waves : 0;
    sw.debug_corner_extent = env("OFX_DEBUG_CORNER_EXTENT", 0);
    return sw;
}

// Frees what a session under construction holds: ofx_session_create's one exit for every failure.
struct SessionDeleter {
    void operator()(ofx_session *s) const
    {
        if (s->arena) (void)hipFree(s->arena);
        delete s;
    }
};

extern "C" int ofx_session_create(const ofx_params *p_in, ofx_session **out)
{
    OFX_REQUIRE(p_in && out, "ofx_session_create: null argument");
    ofx_plan::SessionPlan plan;
    char err[512];
    if (const int rc = ofx_plan::session_plan_make(p_in, session_switches_from_env(), &plan, err, sizeof err)) {
        ofx_set_error("%s", err);
        return rc;
    }
    OFX_HIP(hipSetDevice(plan.p.device));
    std::unique_ptr<ofx_session, SessionDeleter> guard(new (std::nothrow) ofx_session());
    ofx_session *s = guard.get();
    OFX_REQUIRE(s != nullptr, "ofx_session_create: out of host memory");
    hipError_t e = hipMalloc(&s->arena, plan.total);
    if (e != hipSuccess) {
        s->arena = nullptr;
        ofx_set_error("ofx_session_create: hipMalloc(%zu bytes): %s", plan.total, hipGetErrorString(e));
        return OFX_E_HIP;
    }
    s->arena_bytes = plan.total;
    e = hipMemset(s->arena, 0, plan.total);
    if (e != hipSuccess) {
        ofx_set_error("ofx_session_create: hipMemset: %s", hipGetErrorString(e));
        return OFX_E_HIP;
    }
    // every pointer of the session: base + its offset in the plan (null where the plan has none)
    uint8_t *const base = static_cast<uint8_t *>(s->arena);
    auto at = [base](size_t off) { return off == ofx_plan::kNoOffset ? nullptr : base + off; };
    auto flt = [&at](size_t off) { return reinterpret_cast<float *>(at(off)); };
    const ofx_plan::ArenaOffsets &o = plan.off;
    for (int k = 0; k < plan.p.levels; ++k) {
        for (int t = 0; t < kSets; ++t) s->img[t][k] = at(o.img[t][k]), s->pimg[t][k] = at(o.pimg[t][k]);
        for (int t = 0; t < 2; ++t) s->sh[t][k] = at(o.sh[t][k]);
        for (int t = 0; t < kMaxBatch; ++t) {
            for (int j = 0; j < 3; ++j) s->itsh[t][j][k] = at(o.itsh[t][j][k]);
            for (int f = 0; f < 2; ++f) s->pscr[t][f][k] = at(o.pscr[t][f][k]);
            s->preloc[t][k] = at(o.preloc[t][k]);
            s->flowset[t][k] = flt(o.flowset[t][k]);
            s->flowset2[t][k] = flt(o.flowset2[t][k]);
        }
        s->flow[k] = s->flowset[0][k];
    }
    s->corner_status = reinterpret_cast<int *>(at(o.status));
    s->pair_status = s->corner_status + 1;
    s->uv = flt(o.uv);
    s->staging = at(o.staging);
    // geometry and flags
    s->p = plan.p;
    s->n_sets = plan.n_sets;
    for (int k = 0; k < plan.p.levels; ++k) {
        const ofx_plan::LevelPlan &l = plan.lv[k];
        s->w[k] = l.w, s->h[k] = l.h, s->pitch[k] = l.pitch;
        s->own0[k] = l.own0, s->own1[k] = l.own1, s->buf0[k] = l.buf0, s->buf1[k] = l.buf1;
        s->cmp0[k] = l.cmp0, s->cmp1[k] = l.cmp1, s->fl0[k] = l.fl0, s->fl1[k] = l.fl1;
        s->pw[k] = l.pw, s->ph[k] = l.ph, s->ppitch[k] = l.ppitch;
    }
    s->repair = plan.repair;
    s->debug_extent = plan.debug_extent;
    s->fused_iters = plan.fused_iters;
    s->iter_pairs = plan.iter_pairs;
    s->n_iter_pass = ofx_plan::iter_plan_make(plan.p.iters, s->fused_iters, s->iter_pairs, s->iter_plan);
    s->n_iter_pass1 = ofx_plan::iter_plan_make(plan.p.iters, s->fused_iters, false, s->iter_plan1);
    s->pair_opts = ofx_pair_opts{plan.pair_pack, plan.pair_waves, &s->pair_cache};
    repoint(s);
    *out = guard.release();
    return OFX_OK;
}

extern "C" int ofx_session_destroy(ofx_session *s)
{
    if (!s) return OFX_OK;
    hipError_t e = hipSuccess;
    (void)hipSetDevice(s->p.device);
    for (hipEvent_t ev : s->ev) (void)hipEventDestroy(ev);
    if (s->ev_frame) (void)hipEventDestroy(s->ev_frame);
    if (s->ev_ready) (void)hipEventDestroy(s->ev_ready);
    for (hipEvent_t ev : s->ev_set_done)
        if (ev) (void)hipEventDestroy(ev);
    if (s->aux) (void)hipStreamDestroy(s->aux);
    if (s->arena) e = hipFree(s->arena);
    if (s->fe_arena && e == hipSuccess) e = hipFree(s->fe_arena);
    ofx_frontend_tables_free(s->fe);
    ofx_pair_cache_free(s->pair_cache);
    delete s;
    if (e != hipSuccess) {
        ofx_set_error("ofx_session_destroy: hipFree: %s", hipGetErrorString(e));
        return OFX_E_HIP;
    }
    return OFX_OK;
}

// copy rows [buf0,buf1) of a tightly packed w-bytes-per-row frame into the level-0 `next` plane
static int load_level0(ofx_session *s, const uint8_t *src, bool src_is_host, int src_pitch, hipStream_t st)
{
    const int rows = s->buf1[0] - s->buf0[0];
    if (s->pframe[(s->cur + 1) % 3]) { // (a borrowing session that is handed a host frame, or staged: back to its own plane)
        s->pframe[(s->cur + 1) % 3] = nullptr;
        repoint(s);
    }
    OFX_HIP(hipMemcpy2DAsync(s->plane[1][0], (size_t)s->pitch[0], src + (size_t)s->buf0[0] * (size_t)src_pitch, (size_t)src_pitch,
                             (size_t)s->w[0], (size_t)rows, src_is_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    s->have_next = true;
    return OFX_OK;
}

extern "C" int ofx_session_set_frame_host(ofx_session *s, const uint8_t *h_gray1, void *stream)
{
    OFX_REQUIRE(s && h_gray1, "ofx_session_set_frame_host: null argument");
    return load_level0(s, h_gray1, true, s->w[0], ofx_stream(stream));
}

extern "C" int ofx_session_set_frame_device(ofx_session *s, const uint8_t *d_gray1, int pitch, void *stream)
{
    OFX_REQUIRE(s && d_gray1, "ofx_session_set_frame_device: null argument");
    OFX_REQUIRE(pitch >= s->w[0], "ofx_session_set_frame_device: pitch %d < width %d", pitch, s->w[0]);
    if (s->p.borrow_frames) {
        // no copy: the pyramid, corner and LK launches read the caller's buffer in place -- until the run_flow of the pair in
        // which this frame is the PREVIOUS one has run (include/ofx.h, borrow_frames)
        OFX_REQUIRE(pitch == s->pitch[0] && ((uintptr_t)d_gray1 & 3) == 0,
                    "ofx_session_set_frame_device: a borrowed frame needs the session's level-0 pitch (%d bytes: the width rounded up to 64; "
                    "got %d) and a 4-byte aligned address", s->pitch[0], pitch);
        s->pframe[(s->cur + 1) % 3] = d_gray1;
        repoint(s);
        s->have_next = true;
        return OFX_OK;
    }
    return load_level0(s, d_gray1, false, pitch, ofx_stream(stream));
}

extern "C" int ofx_session_set_frame_host_3ch(ofx_session *s, const uint8_t *h_img3, void *stream)
{
    OFX_REQUIRE(s && h_img3, "ofx_session_set_frame_host_3ch: null argument");
    OFX_REQUIRE(!s->p.sharded, "ofx_session_set_frame_host_3ch: not available on a sharded session");
    hipStream_t st = ofx_stream(stream);
    if (s->pframe[(s->cur + 1) % 3]) {
        s->pframe[(s->cur + 1) % 3] = nullptr;
        repoint(s);
    }
    OFX_HIP(hipMemcpyAsync(s->staging, h_img3, (size_t)s->w[0] * (size_t)s->h[0] * 3, hipMemcpyHostToDevice, st));
    // the reference reads channel 0 only (OptFlowCPU.cpp:102, OptFlowGpu.cu:1079)
    OFX_TRY(ofx_extract_ch0(s->staging, s->plane[1][0], s->w[0], s->h[0], s->pitch[0], stream));
    s->have_next = true;
    return OFX_OK;
}

extern "C" int ofx_session_downsample_level(ofx_session *s, int k, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_downsample_level: null session");
    OFX_REQUIRE(k >= 1 && k < s->p.levels, "ofx_session_downsample_level: level %d out of range", k);
    OFX_REQUIRE(s->have_next, "ofx_session_downsample_level: no frame loaded");
    const ofx_geom g = level_geom(s, k, s->cmp0[k], s->cmp1[k]);
    return ofx_downsample_1ch(s->plane[1][k - 1], s->pitch[k - 1], s->buf0[k - 1], s->buf1[k - 1] - s->buf0[k - 1],
                              s->plane[1][k], &g, stream);
}

static int build_pyramid(ofx_session *s, void *stream)
{
    if (s->p.levels == 1) return OFX_OK;
    if (!s->p.sharded && s->p.levels - 1 <= 6) { // whole levels: one fused launch
        uint8_t *lv[OFX_MAX_LEVELS] = {};
        int pitches[OFX_MAX_LEVELS] = {};
        for (int k = 1; k < s->p.levels; ++k) {
            lv[k] = s->plane[1][k];
            pitches[k] = s->pitch[k];
        }
        return timed_launch(s, OFX_TIME_PYRAMID, stream,
                            [&] { return ofx_pyramid_1ch(s->plane[1][0], s->pitch0_next(), s->w[0], s->h[0], lv, pitches, s->p.levels, stream); });
    }
    for (int k = 1; k < s->p.levels; ++k) OFX_TRY(ofx_session_downsample_level(s, k, stream));
    return OFX_OK;
}

extern "C" int ofx_session_build_pyramid(ofx_session *s, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_build_pyramid: null session");
    if (!s->have_next) {
        ofx_set_error("ofx_session_build_pyramid: no frame loaded");
        return OFX_E_STATE;
    }
    return build_pyramid(s, stream);
}

extern "C" int ofx_session_compute_uv(ofx_session *s, int level, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_compute_uv: null session");
    OFX_REQUIRE(level >= 0 && level < s->p.levels, "ofx_session_compute_uv: level %d out of range", level);
    if (level == s->p.levels - 1) return OFX_OK; // top level is not shifted (OptFlowCPU.cpp:321)
    const float *lv[OFX_MAX_LEVELS] = {};
    for (int k = 0; k < s->p.levels; ++k) lv[k] = s->flow[k];
    return ofx_shift_vector(lv, level, s->p.levels, s->uv_cur() + 2 * level, stream);
}

extern "C" int ofx_session_run_level(ofx_session *s, int level, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_run_level: null session");
    OFX_REQUIRE(level >= 0 && level < s->p.levels, "ofx_session_run_level: level %d out of range", level);
    if (!s->have_prev || !s->have_next) {
        ofx_set_error("ofx_session_run_level: need a previous and a next frame (load, build, swap, load, build)");
        return OFX_E_STATE;
    }
    // (the flow buffers of such a session start above the own rows -- fl0 < own0 -- and only the stream pipeline addresses them so)
    OFX_REQUIRE(!(s->p.sharded && s->p.iters > 1), "ofx_session_run_level: refinement iterations on a sharded session run through the stream "
                                                    "pipeline (ofx_session_stream_*)");
    const uint8_t *next = s->plane[1][level];
    if (level != s->p.levels - 1) {
        // shift every row the LK stencil will read: own rows +- (radius + 1), clipped to the buffer
        const int halo = (s->p.window >> 1) + 1;
        int y0 = s->own0[level] - halo, y1 = s->own1[level] + halo;
        if (y0 < s->buf0[level]) y0 = s->buf0[level];
        if (y1 > s->buf1[level]) y1 = s->buf1[level];
        const ofx_geom gs = level_geom(s, level, y0, y1);
        OFX_TRY(ofx_shift_1ch(s->plane[1][level], s->plane[2][level], &gs, s->uv_cur() + 2 * level, stream));
        next = s->plane[2][level];
    }
    const ofx_geom g = level_geom(s, level, s->own0[level], s->own1[level]);
    auto launch = [&] { return ofx_lk_level(s->plane[0][level], next, &g, s->p.window, s->p.mode, s->flow[level], s->own0[level], stream); };
    if (level != 0) return launch();
    return timed_launch(s, OFX_TIME_LK, stream, launch);
}

extern "C" int ofx_session_timing(ofx_session *s, int max_launches)
{
    OFX_REQUIRE(s && max_launches >= 0, "ofx_session_timing: bad arguments");
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    s->ev.clear();
    s->ev_kind.assign((size_t)max_launches, 0);
    s->ev_used = 0;
    s->timing = max_launches > 0;
    for (int i = 0; i < 2 * max_launches; ++i) {
        hipEvent_t e;
        OFX_HIP(hipEventCreate(&e));
        s->ev.push_back(e);
    }
    return OFX_OK;
}

// average / minimum over the recorded launches whose kind is in `kind_mask` (bit OFX_TIME_*); does not re-arm
static int timing_stats(ofx_session *s, unsigned kind_mask, double *avg_us, double *min_us, int *launches)
{
    double sum = 0, mn = 1e30;
    int n = 0;
    for (size_t i = 0; i < s->ev_used / 2; ++i) {
        if (!((kind_mask >> s->ev_kind[i]) & 1u)) continue;
        OFX_HIP(hipEventSynchronize(s->ev[2 * i + 1]));
        float ms = 0;
        OFX_HIP(hipEventElapsedTime(&ms, s->ev[2 * i], s->ev[2 * i + 1]));
        sum += ms * 1e3;
        if (ms * 1e3 < mn) mn = ms * 1e3;
        ++n;
    }
    *avg_us = n ? sum / n : 0.0;
    if (min_us) *min_us = n ? mn : 0.0;
    *launches = n;
    return OFX_OK;
}

extern "C" int ofx_session_timing_read(ofx_session *s, double *avg_us, double *min_us, int *launches)
{
    OFX_REQUIRE(s && avg_us && launches, "ofx_session_timing_read: bad arguments");
    // the dominant launches: the fused LK launches of the pair-at-a-time paths, the stream tick of the stream pipeline
    OFX_TRY(timing_stats(s, (1u << OFX_TIME_LK) | (1u << OFX_TIME_LK_ACC) | (1u << OFX_TIME_LK_ACC_WARP) | (1u << OFX_TIME_STREAM), avg_us, min_us, launches));
    s->ev_used = 0;
    return OFX_OK;
}

extern "C" int ofx_session_timing_read_kind(ofx_session *s, int kind, double *avg_us, double *min_us, int *launches)
{
    OFX_REQUIRE(s && avg_us && launches && kind >= 0 && kind < OFX_TIME_KINDS, "ofx_session_timing_read_kind: bad arguments");
    return timing_stats(s, 1u << kind, avg_us, min_us, launches);
}

// Shift vectors of every level at once (ofx_corner_flows); meaningful on the rank whose buffers start at row 0.
extern "C" int ofx_session_corner_flows(ofx_session *s, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_corner_flows: null session");
    if (!s->have_prev || !s->have_next) {
        ofx_set_error("ofx_session_corner_flows: need a previous and a next frame");
        return OFX_E_STATE;
    }
    ofx_lk_desc d[OFX_MAX_LEVELS];
    for (int k = 0; k < s->p.levels; ++k)
        d[k] = ofx_lk_desc{s->plane[0][k], s->plane[1][k], level_geom(s, k, s->own0[k], s->own1[k]), nullptr, s->own0[k], nullptr, 0, s->p.min_det};
    return timed_launch(s, OFX_TIME_CORNER, stream, [&] { return ofx_corner_flows(d, s->p.levels, s->p.window, s->p.mode, s->uv_cur(), stream); });
}

// Every level's fused LK in one launch, using the uv slots as they stand; below the top level the kernel reads `next`
// through the global shift (no separate shift pass, no shifted planes).
// one multi-level LK launch, bracketed by timing events when the session is armed (ofx_session_timing)
static int timed_lk_launch(ofx_session *s, const ofx_lk_desc *lk, int nl, void *stream)
{
    return timed_launch(s, lk[0].accumulate ? (lk[0].d_warp_out ? OFX_TIME_LK_ACC_WARP : OFX_TIME_LK_ACC) : OFX_TIME_LK, stream,
                        [&] { return ofx_lk_levels(lk, nl, s->p.window, s->p.mode, stream); });
}

// k_lo: the finest level of the launches (0: the whole pyramid; levels - 1: the top level alone, which has no shift and reads no uv)
static int lk_all_levels(ofx_session *s, const float *uv, void *stream, int k_lo = 0)
{
    const int L = s->p.levels;
    ofx_lk_desc lk[OFX_MAX_LEVELS];
    if (s->p.iters <= 1) {
        int nl = 0;
        for (int k = L - 1; k >= k_lo; --k) // coarse levels first: their few waves start at once and finish early
            lk[nl++] = ofx_lk_desc{s->plane[0][k], s->plane[1][k], level_geom(s, k, s->own0[k], s->own1[k]), s->flow[k], s->own0[k],
                                   k == L - 1 ? nullptr : uv + 2 * k, 0, s->p.min_det};
        return timed_lk_launch(s, lk, nl, stream);
    }
    OFX_REQUIRE(!s->p.sharded, "refinement iterations on a sharded session run through the stream pipeline (ofx_session_stream_*)");
    // Extension (DESIGN.md "lk_iter"): iteration 1 is the reference level; every further iteration warps
    // the shifted next image by the flow so far (bilinear, rounded to u8) and adds the flow of (prev, warped).
    // sh[0] holds the globally shifted next image (the warp source), sh[1] the warped image.
    ofx_shift_desc sd[OFX_MAX_LEVELS];
    int ns = 0;
    for (int k = L - 2; k >= k_lo; --k)
        sd[ns++] = ofx_shift_desc{s->plane[1][k], s->sh[0][k], level_geom(s, k, 0, s->h[k]), uv + 2 * k};
    if (ns) OFX_TRY(timed_launch(s, OFX_TIME_SHIFT, stream, [&] { return ofx_shift_levels(sd, ns, stream); }));
    auto src = [&](int k) { return k == L - 1 ? s->plane[1][k] : s->sh[0][k]; };
    // The warped image alternates between two planes (sh[1] and the iteration scratch's third): fused (lk_body_warp.h), every launch
    // but the last writes the warped image the iteration after it reads, from the flow it has in registers -- no warp launch at all.
    // Which plane a launch reads and writes is the schedule's (iter_plan.h); iteration 1 writes plane 0.
    uint8_t *const *wbuf[2] = {s->sh[1], s->itsh[0][2]};
    int nl = 0;
    for (int k = L - 1; k >= k_lo; --k) {
        lk[nl] = ofx_lk_desc{s->plane[0][k], src(k), level_geom(s, k, 0, s->h[k]), s->flow[k], 0, nullptr, 0, s->p.min_det};
        if (s->fused_iters) lk[nl].d_warp_src = src(k), lk[nl].d_warp_out = wbuf[0][k], lk[nl].warp_scale = OFX_ITER_SCALE;
        ++nl;
    }
    OFX_TRY(timed_lk_launch(s, lk, nl, stream));
    for (int i = 0; i < s->n_iter_pass1; ++i) {
        const ofx_plan::IterPass &q = s->iter_plan1[i];
        ofx_warp_desc wd[OFX_MAX_LEVELS];
        nl = 0;
        for (int k = L - 1; k >= k_lo; --k) {
            wd[nl] = ofx_warp_desc{src(k), wbuf[q.win][k], level_geom(s, k, 0, s->h[k]), s->flow[k], 0, OFX_ITER_SCALE, nullptr, 0};
            lk[nl] = ofx_lk_desc{s->plane[0][k], wbuf[q.win][k], level_geom(s, k, 0, s->h[k]), s->flow[k], 0, nullptr, 1, s->p.min_det};
            if (q.wout) lk[nl].d_warp_src = src(k), lk[nl].d_warp_out = wbuf[q.wo][k], lk[nl].warp_scale = OFX_ITER_SCALE;
            ++nl;
        }
        if (q.warp) OFX_TRY(timed_launch(s, OFX_TIME_WARP, stream, [&] { return ofx_warp_levels(wd, nl, stream); }));
        OFX_TRY(timed_lk_launch(s, lk, nl, stream));
    }
    return OFX_OK;
}

extern "C" int ofx_session_run_levels(ofx_session *s, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_run_levels: null session");
    if (!s->have_prev || !s->have_next) {
        ofx_set_error("ofx_session_run_levels: need a previous and a next frame");
        return OFX_E_STATE;
    }
    if (s->p.sharded && !s->p.local_corner && s->p.levels > 1) {
        // the shift vectors were computed elsewhere (rank 0's corner kernel, then the broadcast): check them against this
        // shard's halo on the device, without a host round trip (ofx_session_corner_status reads the word)
        int rows[OFX_MAX_LEVELS][4];
        shard_reach(s, rows);
        OFX_TRY(ofx_shard_margin_check(s->uv_cur(), s->p.levels, s->h, &rows[0][0], s->corner_status, stream));
    }
    return lk_all_levels(s, s->uv_cur(), stream);
}

extern "C" int ofx_session_run_flow(ofx_session *s, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_run_flow: null session");
    OFX_REQUIRE(!s->p.sharded || s->buf0[0] == 0, "ofx_session_run_flow: on a sharded session only the rank holding row 0 can "
                                                   "form the shift vectors; use corner_flows + broadcast + run_levels");
    OFX_TRY(ofx_session_corner_flows(s, stream));
    return ofx_session_run_levels(s, stream);
}

// what both dense calls require of the session and of max_px before anything is enqueued; `who` names the entry point
static int dense_check(ofx_session *s, const char *who, float max_px)
{
    OFX_REQUIRE(s, "%s: null session", who);
    OFX_REQUIRE(__builtin_isfinite(max_px) && max_px >= 0.0f, "%s: max_px must be finite and >= 0 (0 = off)", who);
    auto unsupported = [who](const char *what) {
        ofx_set_error("%s: %s", who, what);
        return OFX_E_UNSUPPORTED;
    };
    if (s->p.sharded) return unsupported("not available on a sharded session (a level's warp crosses shard rows)");
    if (s->p.mode == OFX_MODE_COMPAT_CPU) return unsupported("needs mode lk_float or lk_float_fast (the accumulating launches)");
    if (s->p.borrow_frames)
        return unsupported("not available with borrow_frames (level 0 of the next frame is a warp source, which must be followed by three readable bytes)");
    if (!s->have_prev || !s->have_next) {
        ofx_set_error("%s: need a previous and a next frame (load, build, swap, load, build)", who);
        return OFX_E_STATE;
    }
    const int L = s->p.levels, iters = s->p.iters > 1 ? s->p.iters : 1;
    for (int k = 0; k + 1 < L; ++k) // (the launches that also write the warped image address a level through 32-bit offsets)
        if (iters > 1 && !ofx_plan::fits_buffer_offsets(s->h[k], s->pitch[k], s->h[k], s->w[k])) return unsupported("a level of 2 GB or more");
    return OFX_OK;
}

// The pair's dense flow ("coarse-to-fine propagation", include/ofx.h): the top level as run_flow runs it, then level by level one
// prolongation (which also writes the first warped image) and `iters` accumulating single-level LK launches.  The warped images
// alternate between sh[0][k] and sh[1][k]: nothing is shifted here, so both are free.
extern "C" int ofx_session_run_flow_dense(ofx_session *s, float max_px, void *stream)
{
    OFX_TRY(dense_check(s, "ofx_session_run_flow_dense", max_px));
    const int L = s->p.levels, iters = s->p.iters > 1 ? s->p.iters : 1;
    OFX_TRY(lk_all_levels(s, s->uv_cur(), stream, L - 1));
    for (int k = L - 2; k >= 0; --k) {
        const ofx_prolong_desc pd{s->flow[k + 1], s->w[k + 1], s->h[k + 1], s->flow[k], s->w[k], s->h[k], OFX_ITER_SCALE, max_px,
                                  s->plane[1][k], s->pitch[k], s->sh[0][k], s->pitch[k]};
        OFX_TRY(timed_launch(s, OFX_TIME_WARP, stream, [&] { return ofx_flow_prolong(&pd, 1, stream); }));
        for (int i = 0; i < iters; ++i) {
            ofx_lk_desc lk{s->plane[0][k], s->sh[i & 1][k], level_geom(s, k, 0, s->h[k]), s->flow[k], 0, nullptr, 1, s->p.min_det};
            if (i + 1 < iters) lk.d_warp_src = s->plane[1][k], lk.d_warp_out = s->sh[(i + 1) & 1][k], lk.warp_scale = OFX_ITER_SCALE;
            OFX_TRY(timed_lk_launch(s, &lk, 1, stream));
        }
    }
    return OFX_OK;
}

// the caller's second flow pyramid of ofx_session_run_flow_dense_median: level k at the sum of the sizes of the levels below it
static size_t median_scratch_offset(const ofx_session *s, int k)
{
    size_t o = 0;
    for (int j = 0; j < k; ++j) o += (size_t)s->w[j] * (size_t)s->h[j] * 8;
    return o;
}

extern "C" int ofx_session_dense_median_scratch_bytes(ofx_session *s, size_t *bytes)
{
    OFX_REQUIRE(s && bytes, "ofx_session_dense_median_scratch_bytes: bad arguments");
    *bytes = median_scratch_offset(s, s->p.levels);
    return OFX_OK;
}

// "A pair's dense flow with median" (the block "flow median", include/ofx.h): run_flow_dense's calls, with one ofx_flow_median after
// the top level and after every accumulating launch below it.  The median is out of place: a level's flow alternates between
// flow[k] and the caller's scratch, starting where `iters` flips end in flow[k]; the medians, not the LK launches, write the next
// warped image (from the filtered vectors).
extern "C" int ofx_session_run_flow_dense_median(ofx_session *s, float max_px, int radius, void *d_scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "ofx_session_run_flow_dense_median";
    OFX_TRY(dense_check(s, who, max_px));
    OFX_REQUIRE(radius == 1 || radius == 2, "%s: the radius %d is not 1 (3x3) or 2 (5x5)", who, radius);
    OFX_REQUIRE(d_scratch, "%s: the scratch is null", who);
    OFX_REQUIRE(((uintptr_t)d_scratch & 7) == 0, "%s: the scratch must be 8-byte aligned", who);
    const int L = s->p.levels, iters = s->p.iters > 1 ? s->p.iters : 1;
    OFX_REQUIRE(scratch_bytes >= median_scratch_offset(s, L), "%s: the scratch holds %zu bytes, the flow pyramid has %zu (ofx_session_dense_median_scratch_bytes)",
                who, scratch_bytes, median_scratch_offset(s, L));
    auto scratch = [&](int k) { return reinterpret_cast<float *>(static_cast<char *>(d_scratch) + median_scratch_offset(s, k)); };
    auto median = [&](int k, const float *from, float *to, uint8_t *warped) {
        const ofx_median_desc md{from, to, s->w[k], s->h[k], radius, OFX_ITER_SCALE, warped ? s->plane[1][k] : nullptr, warped ? s->pitch[k] : 0,
                                 warped, warped ? s->pitch[k] : 0};
        return timed_launch(s, OFX_TIME_WARP, stream, [&] { return ofx_flow_median(&md, 1, stream); });
    };
    OFX_TRY(lk_all_levels(s, s->uv_cur(), stream, L - 1));
    OFX_TRY(median(L - 1, s->flow[L - 1], scratch(L - 1), nullptr));
    OFX_HIP(hipMemcpyAsync(s->flow[L - 1], scratch(L - 1), (size_t)s->w[L - 1] * (size_t)s->h[L - 1] * 8, hipMemcpyDeviceToDevice, ofx_stream(stream)));
    for (int k = L - 2; k >= 0; --k) {
        float *buf[2] = {s->flow[k], scratch(k)};
        int cur = iters & 1; // (iters flips from here end in buf[0], the session's plane)
        const ofx_prolong_desc pd{s->flow[k + 1], s->w[k + 1], s->h[k + 1], buf[cur], s->w[k], s->h[k], OFX_ITER_SCALE, max_px,
                                  s->plane[1][k], s->pitch[k], s->sh[0][k], s->pitch[k]};
        OFX_TRY(timed_launch(s, OFX_TIME_WARP, stream, [&] { return ofx_flow_prolong(&pd, 1, stream); }));
        for (int i = 0; i < iters; ++i) {
            const ofx_lk_desc lk{s->plane[0][k], s->sh[i & 1][k], level_geom(s, k, 0, s->h[k]), buf[cur], 0, nullptr, 1, s->p.min_det};
            OFX_TRY(timed_lk_launch(s, &lk, 1, stream));
            OFX_TRY(median(k, buf[cur], buf[cur ^ 1], i + 1 < iters ? s->sh[(i + 1) & 1][k] : nullptr));
            cur ^= 1;
        }
    }
    return OFX_OK;
}

// The reference's literal sequence (one level after the other, main.cu:256-262); kept for comparison and tests.
extern "C" int ofx_session_run_flow_sequential(ofx_session *s, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_run_flow_sequential: null session");
    for (int k = s->p.levels - 1; k >= 0; --k) {
        OFX_TRY(ofx_session_compute_uv(s, k, stream));
        OFX_TRY(ofx_session_run_level(s, k, stream));
    }
    return OFX_OK;
}

extern "C" int ofx_session_swap(ofx_session *s)
{
    OFX_REQUIRE(s, "ofx_session_swap: null session");
    s->cur = (s->cur + 1) % 3;
    s->uv_slot ^= 1;
    repoint(s);
    s->have_prev = s->have_next;
    s->have_next = false;
    s->staged = false;
    return OFX_OK;
}

// ---- pipelined path ---------------------------------------------------------------------------------------------------
// A pair is split in two halves that run on different streams:
//   staging (aux stream):  load the new frame, build its pyramid, corner flows, shift of every level
//   solve   (main stream): the multi-level LK launch
// The LK launch of pair i is VALU-bound and fills the chip; the staging kernels of pair i+1 are small and latency-bound,
// so running them underneath it hides them almost entirely.  Hazards are covered by two events: `ev_ready` (staging ->
// LK of the same pair) and `ev_set_done[x]` (LK that read image set x as `prev` -> the staging that overwrites set x two
// pairs later; the same event also orders the reuse of the shifted-scratch set).
static int ensure_pipeline(ofx_session *s)
{
    if (s->ev_ready) return OFX_OK;
    OFX_HIP(hipEventCreateWithFlags(&s->ev_ready, hipEventDisableTiming));
    OFX_HIP(hipEventCreateWithFlags(&s->ev_frame, hipEventDisableTiming));
    for (int i = 0; i < 3; ++i) OFX_HIP(hipEventCreateWithFlags(&s->ev_set_done[i], hipEventDisableTiming));
    // highest priority: the staging kernels are tiny and must slip in between the LK waves of the previous pair
    int prio_lo = 0, prio_hi = 0;
    OFX_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    OFX_HIP(hipStreamCreateWithPriority(&s->aux, hipStreamNonBlocking, prio_hi));
    return OFX_OK;
}

extern "C" int ofx_session_aux_stream(ofx_session *s, void **stream)
{
    OFX_REQUIRE(s && stream, "ofx_session_aux_stream: null argument");
    OFX_TRY(ensure_pipeline(s));
    *stream = s->aux;
    return OFX_OK;
}

// staging, part 1: frame -> next image set, pyramid.  `d_gray1` is read on the staging stream: the caller orders that stream
// behind the frame's producer (ofx_session_submit_device does it with an event on its `stream` argument).
extern "C" int ofx_session_stage_frame(ofx_session *s, const uint8_t *d_gray1, int pitch, void *aux_stream)
{
    OFX_REQUIRE(s && d_gray1, "ofx_session_stage_frame: null argument");
    OFX_REQUIRE(pitch >= s->w[0], "ofx_session_stage_frame: pitch %d < width %d", pitch, s->w[0]);
    if (!s->have_prev) {
        ofx_set_error("ofx_session_stage_frame: no previous frame (load, build, swap first)");
        return OFX_E_STATE;
    }
    OFX_TRY(ensure_pipeline(s));
    hipStream_t aux = aux_stream ? ofx_stream(aux_stream) : s->aux;
    const int nxt = (s->cur + 1) % 3;
    if (s->set_busy[nxt]) OFX_HIP(hipStreamWaitEvent(aux, s->ev_set_done[nxt], 0));
    OFX_TRY(load_level0(s, d_gray1, false, pitch, aux));
    return build_pyramid(s, aux);
}

// staging, part 2 (after the corner flows / the broadcast of the shift vectors): signal the solve half.  (The shift
// itself is fused into the LK launch; the name is kept from when it was a separate pass.)
extern "C" int ofx_session_stage_shift(ofx_session *s, void *aux_stream)
{
    OFX_REQUIRE(s, "ofx_session_stage_shift: null session");
    if (!s->have_prev || !s->have_next) {
        ofx_set_error("ofx_session_stage_shift: stage a frame first");
        return OFX_E_STATE;
    }
    OFX_TRY(ensure_pipeline(s));
    hipStream_t aux = aux_stream ? ofx_stream(aux_stream) : s->aux;
    OFX_HIP(hipEventRecord(s->ev_ready, aux));
    s->staged = true;
    return OFX_OK;
}

// solve half: one multi-level LK launch on the caller's stream, then the staged frame becomes the previous frame.
extern "C" int ofx_session_solve_staged(ofx_session *s, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_solve_staged: null session");
    if (!s->staged) {
        ofx_set_error("ofx_session_solve_staged: nothing staged (stage_frame, corner_flows, stage_shift first)");
        return OFX_E_STATE;
    }
    hipStream_t st = ofx_stream(stream);
    OFX_HIP(hipStreamWaitEvent(st, s->ev_ready, 0));
    OFX_TRY(lk_all_levels(s, s->uv_cur(), stream));
    OFX_HIP(hipEventRecord(s->ev_set_done[s->cur], st));
    s->set_busy[s->cur] = true;
    return ofx_session_swap(s);
}

// Whole pair, pipelined: staging on the session's aux stream, solve on `stream`; on return the new frame is the
// previous frame.  Equivalent to set_frame_device + build_pyramid + run_flow + swap, bit for bit.
extern "C" int ofx_session_submit_device(ofx_session *s, const uint8_t *d_gray1, int pitch, void *stream)
{
    OFX_REQUIRE(s, "ofx_session_submit_device: null session");
    OFX_REQUIRE(!s->p.sharded || s->buf0[0] == 0, "ofx_session_submit_device: on a sharded session drive the halves yourself "
                                                   "(stage_frame, corner_flows on the rank holding row 0, broadcast, stage_shift, "
                                                   "solve_staged)");
    // the frame may still be in production on the caller's stream (an async upload, a decoder or grayscale kernel): the
    // staging stream reads it, so it is ordered behind everything enqueued on `stream` so far
    OFX_TRY(ensure_pipeline(s));
    OFX_HIP(hipEventRecord(s->ev_frame, ofx_stream(stream)));
    OFX_HIP(hipStreamWaitEvent(s->aux, s->ev_frame, 0));
    OFX_TRY(ofx_session_stage_frame(s, d_gray1, pitch, nullptr));
    OFX_TRY(ofx_session_corner_flows(s, s->aux));
    OFX_TRY(ofx_session_stage_shift(s, nullptr));
    return ofx_session_solve_staged(s, stream);
}

extern "C" int ofx_session_plane(ofx_session *s, int which, int level, uint8_t **d_ptr, ofx_geom *geom)
{
    OFX_REQUIRE(s && which >= 0 && which < 3 && level >= 0 && level < s->p.levels, "ofx_session_plane: bad arguments");
    if (d_ptr) *d_ptr = s->plane[which][level];
    if (geom) *geom = level_geom(s, level, s->own0[level], s->own1[level]);
    return OFX_OK;
}

extern "C" int ofx_session_flow(ofx_session *s, int level, float **d_ptr, int *row0, int *rows)
{
    OFX_REQUIRE(s && level >= 0 && level < s->p.levels, "ofx_session_flow: bad arguments");
    if (d_ptr) *d_ptr = s->flow[level] + s->flow_own_offset(level);
    if (row0) *row0 = s->own0[level];
    if (rows) *rows = s->own1[level] - s->own0[level];
    return OFX_OK;
}

extern "C" int ofx_session_shift_uv(ofx_session *s, int level, float **d_uv)
{
    OFX_REQUIRE(s && d_uv && level >= 0 && level < s->p.levels, "ofx_session_shift_uv: bad arguments");
    *d_uv = s->uv_cur() + 2 * level; // slot of the pair in progress (alternates per pair)
    return OFX_OK;
}

extern "C" int ofx_session_get_flow_host(ofx_session *s, int level, float *h_dst, void *stream)
{
    OFX_REQUIRE(s && h_dst && level >= 0 && level < s->p.levels, "ofx_session_get_flow_host: bad arguments");
    const size_t bytes = (size_t)(s->own1[level] - s->own0[level]) * (size_t)s->w[level] * 2 * sizeof(float);
    hipStream_t st = ofx_stream(stream);
    OFX_HIP(hipMemcpyAsync(h_dst, s->flow[level] + s->flow_own_offset(level), bytes, hipMemcpyDeviceToHost, st));
    OFX_HIP(hipStreamSynchronize(st));
    return OFX_OK;
}

extern "C" int ofx_session_corner_status(ofx_session *s, int *h_status, void *stream)
{
    OFX_REQUIRE(s && h_status, "ofx_session_corner_status: null argument");
    hipStream_t st = ofx_stream(stream);
    OFX_HIP(hipMemcpyAsync(h_status, s->corner_status, sizeof(int), hipMemcpyDeviceToHost, st));
    OFX_HIP(hipMemsetAsync(s->corner_status, 0, sizeof(int), st));
    OFX_HIP(hipStreamSynchronize(st));
    return OFX_OK;
}

extern "C" int ofx_session_pair_status(ofx_session *s, int pair, int *h_status, void *stream)
{
    OFX_REQUIRE(s && h_status, "ofx_session_pair_status: null argument");
    const int slots = 2 * stream_batch_of(s);
    OFX_REQUIRE(pair >= 1, "ofx_session_pair_status: pairs are counted from 1 (frame 0 -> frame 1)");
    OFX_REQUIRE(pair <= s->corner_newest && pair > s->corner_newest - slots,
                "ofx_session_pair_status: pair %d is not among the newest %d pairs whose corner stage has run (newest: %ld)", pair, slots, s->corner_newest);
    hipStream_t st = ofx_stream(stream);
    OFX_HIP(hipMemcpyAsync(h_status, s->pair_status + (pair % slots), sizeof(int), hipMemcpyDeviceToHost, st));
    OFX_HIP(hipStreamSynchronize(st));
    return OFX_OK;
}
// gpu::calc_opt_flow (OptFlowGpu.cuh:33, OptFlowGpu.cu:1909-1979) with host pointers: upload both images and the
// two floats of every coarser flow level that the shift reads, run one level on the device, download its flow.
extern "C" int ofx_calc_opt_flow_host(const uint8_t *h_prev3, const uint8_t *h_next3, int w, int h, float **h_flow_pyr, int level,
                                      int max_level, int window, int mode)
{
    OFX_REQUIRE(h_prev3 && h_next3 && h_flow_pyr && w > 0 && h > 0, "ofx_calc_opt_flow_host: bad arguments");
    OFX_REQUIRE(max_level >= 1 && max_level <= OFX_MAX_LEVELS && level >= 0 && level < max_level,
                "ofx_calc_opt_flow_host: bad level %d of %d", level, max_level);
    OFX_REQUIRE(h_flow_pyr[level] != nullptr, "ofx_calc_opt_flow_host: flow level %d is null", level);
    const size_t n = (size_t)w * (size_t)h;
    const int pitch = (int)align_up((size_t)w, 64);
    const size_t plane = (size_t)pitch * (size_t)h + 64;
    // buffers come from the calling thread's cached arena (compat_scratch.h): no allocation per call in a frame loop
    ofx_compat::Scratch sc;
    uint8_t *d_p1 = sc.alloc<uint8_t>(plane), *d_n1 = sc.alloc<uint8_t>(plane), *d_s1 = sc.alloc<uint8_t>(plane);
    float *d_flow = sc.alloc<float>(2 * n);
    float *d_coarse = sc.alloc<float>(2 * OFX_MAX_LEVELS + 2); // 2 floats per level, then the shift vector
    if (!sc.ok()) return sc.rc();
    float *d_uv = d_coarse + 2 * OFX_MAX_LEVELS;
    // the reference reads channel 0 only (OptFlowGpu.cu:1079): it is picked out while the images are staged, a third of the bytes
    OFX_TRY(ofx_compat::stage_h2d_ch0(d_p1, pitch, h_prev3, w, h));
    OFX_TRY(ofx_compat::stage_h2d_ch0(d_n1, pitch, h_next3, w, h));
    ofx_geom g{w, h, pitch, 0, h, 0, h};
    const uint8_t *d_next = d_n1;
    if (level != max_level - 1) {
        float coarse[2 * OFX_MAX_LEVELS] = {};
        const float *lv[OFX_MAX_LEVELS] = {};
        for (int k = level + 1; k < max_level; ++k) {
            OFX_REQUIRE(h_flow_pyr[k] != nullptr, "ofx_calc_opt_flow_host: flow level %d is null", k);
            coarse[2 * k] = h_flow_pyr[k][0];
            coarse[2 * k + 1] = h_flow_pyr[k][1];
            lv[k] = d_coarse + 2 * k;
        }
        OFX_HIP(hipMemcpy(d_coarse, coarse, sizeof coarse, hipMemcpyHostToDevice));
        OFX_TRY(ofx_shift_vector(lv, level, max_level, d_uv, nullptr));
        // (ofx_shift_1ch writes every pixel: shifted byte, own byte or the zero of the reference's fresh scratch pages)
        OFX_TRY(ofx_shift_1ch(d_n1, d_s1, &g, d_uv, nullptr));
        d_next = d_s1;
    }
    OFX_TRY(ofx_lk_level(d_p1, d_next, &g, window, mode, d_flow, 0, nullptr));
    sc.download(h_flow_pyr[level], d_flow, 2 * n);
    return sc.rc();
}


// main.cu:138-147 with host pointers: the dense field at `level` that visualizeFlowField samples for its arrows --
// sum over k >= level of 2^(k-level) * flow_k(y >> (k-level), x >> (k-level)) -- composed on the device.
extern "C" int ofx_compose_flow_host(float *const *h_flow_pyr, int w, int h, int levels, int level, float *h_dst)
{
    OFX_REQUIRE(h_flow_pyr && h_dst && w > 0 && h > 0, "ofx_compose_flow_host: bad arguments");
    OFX_REQUIRE(levels >= 1 && levels <= OFX_MAX_LEVELS && level >= 0 && level < levels, "ofx_compose_flow_host: bad level");
    // level k is uploaded as (w >> s) x (h >> s), s = k - level, and the kernel reads its row i >> s for i < h: with h not a
    // multiple of 2^s that is one row past the upload (the reference has the same overrun, on host memory, main.cu:138-147)
    OFX_REQUIRE(w % (1 << (levels - 1 - level)) == 0 && h % (1 << (levels - 1 - level)) == 0,
                "ofx_compose_flow_host: %dx%d is not a multiple of %d (the coarsest level's scale)", w, h, 1 << (levels - 1 - level));
    ofx_compat::Scratch sc;
    const float *d_lv[OFX_MAX_LEVELS] = {};
    for (int k = level; k < levels; ++k) {
        OFX_REQUIRE(h_flow_pyr[k] != nullptr, "ofx_compose_flow_host: flow level %d is null", k);
        // level k of a pyramid whose level `level` is w x h
        d_lv[k] = sc.upload(h_flow_pyr[k], 2 * (size_t)(w >> (k - level)) * (size_t)(h >> (k - level)));
    }
    float *d_dst = sc.alloc<float>(2 * (size_t)w * (size_t)h);
    if (sc.ok()) sc.run(ofx_compose_flow(d_lv, w, h, levels, level, d_dst, nullptr));
    sc.download(h_dst, d_dst, 2 * (size_t)w * (size_t)h);
    return sc.rc();
}
