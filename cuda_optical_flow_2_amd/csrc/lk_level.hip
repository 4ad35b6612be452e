// Fused dense Lucas-Kanade level kernel for gfx950 (MI355X).
//
// One kernel does what the reference does in ten launches plus two host loops per level
// (OptFlowGpu.cu:1930-1964 / OptFlowCPU.cpp:329-384): 3x3 derivative stencils, the five windowed sums of
// products and the 2x2 solve.  Algorithmic HBM traffic: 2 bytes read + 8 bytes written per pixel.
//
// Structure (DESIGN.md "lk_level"):
//   * one 64-lane wave per workgroup; a lane owns 4 adjacent columns, so a wave spans 256 image columns and
//     every global load is one aligned dword per lane (256 B per wave instruction), every flow store 32 B per lane.
//   * the wave marches DOWN a strip of rows.  Per step it loads one new row of each image, forms the three
//     derivative values of its 4 columns (left/right neighbour columns come from the adjacent lanes through
//     DPP wave shifts, no LDS), and updates 5 x 4 vertical running sums:  V += P(row entering) - P(row leaving).
//     The leaving row's derivatives are recomputed from the image (its rows are L2-resident) in the high halves of the
//     same packed-int16 instructions that compute the entering row's (lk_body.h).
//   * the horizontal half of the box sum is done in registers: in-lane prefix/suffix sums plus whole-lane totals
//     of the neighbouring lanes, again through DPP (a sliding difference per output for windows up to 9x9).
//   * the only use of LDS: each output row is exchanged through it so that both streaming store instructions cover
//     gap-free 128-byte lines (non-temporal stores of 16-byte pieces run at half the write bandwidth).
//   * all sums are exact int32, so results do not depend on strip/tile/shard boundaries.
//   * window radius R and mode are template parameters; the host dispatches.
//
// Border semantics follow the reference exactly: image taps outside the image contribute nothing
// (OptFlowCPU.cpp:98, OptFlowGpu.cu:1066-1075) and window taps outside the image are skipped
// (OptFlowCPU.cpp:182-191) -- i.e. the image and the derivative planes are zero-extended.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lk_launch.h"

namespace ofx_launch {
unsigned long long *g_stream_trace = nullptr; // tools/stream_timeline.py
int g_stream_trace_blocks = 0;
int g_trace_header[2 * OFX_STREAM_MAX_BATCH + 1] = {0};
} // namespace ofx_launch

static int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e && atoi(e) > 0 ? atoi(e) : dflt;
}

// OFX_LK_MIN_STRIP is read at every launch (the tests set it in mid-process), the others once per process.
ofx_plan::LkSwitches ofx_launch::lk_switches()
{
    static const ofx_plan::LkSwitches once = [] {
        ofx_plan::LkSwitches s;
        if (const char *e = getenv("OFX_LK_DMA")) s.lk_dma = atoi(e);
        if (const char *e = getenv("OFX_ITER_DMA")) s.iter_dma = atoi(e);
        s.waves_per_simd = env_int("OFX_LK_WAVES_PER_SIMD", 0);
        s.fill = env_int("OFX_LK_FILL", 0);
        s.target_waves = env_int("OFX_LK_TARGET_WAVES", 0);
        return s;
    }();
    ofx_plan::LkSwitches s = once;
    s.min_strip = env_int("OFX_LK_MIN_STRIP", s.min_strip);
    return s;
}

// ---- the packed plans of the fused two-iteration launch (pair_plan.h), on the device --------------------------------------------
// A session sees a handful of launch shapes (a full tick, the partial ticks at its start and in the drain); each gets its plan the
// first time it is launched -- the planner on the host, one allocation, one blocking copy -- and every later launch finds it here.
struct ofx_pair_cache {
    struct Entry {
        std::vector<int> key; // radius, tile width, wave count, then w, h per item
        PairSeg *d_segs;      // NULL: no plan fits
        int waves;
    };
    std::vector<Entry> entries;
};

void ofx_pair_cache_free(ofx_pair_cache *c)
{
    if (!c) return;
    for (ofx_pair_cache::Entry &e : c->entries)
        if (e.d_segs) (void)hipFree(e.d_segs);
    delete c;
}

int ofx_launch::pair_plan_get(ofx_pair_cache **cache, int radius, int out_w, const LkLevelIn *lv, int n, int min_h, int capacity, PairPlanDev *out)
{
    std::vector<int> key{radius, out_w, capacity};
    for (int i = 0; i < n; ++i) key.push_back(lv[i].a.w), key.push_back(lv[i].a.h);
    if (!*cache) *cache = new ofx_pair_cache;
    for (const ofx_pair_cache::Entry &e : (*cache)->entries)
        if (e.key == key) {
            *out = PairPlanDev{e.d_segs, e.waves};
            return OFX_OK;
        }
    std::vector<ofx_plan::PairItem> items(n);
    for (int i = 0; i < n; ++i) items[i] = ofx_plan::PairItem{lv[i].a.w, lv[i].a.h};
    ofx_plan::PairPlan plan;
    ofx_pair_cache::Entry e{key, nullptr, 0};
    const bool fits = ofx_plan::pair_plan_make(items.data(), n, out_w, pair_seg_steps(radius), min_h, capacity, &plan);
    if (fits) {
        const size_t bytes = plan.segs.size() * sizeof(PairSeg);
        OFX_HIP(hipMalloc(reinterpret_cast<void **>(&e.d_segs), bytes));
        const hipError_t rc = hipMemcpy(e.d_segs, plan.segs.data(), bytes, hipMemcpyHostToDevice);
        if (rc != hipSuccess) {
            (void)hipFree(e.d_segs);
            OFX_HIP(rc);
        }
        e.waves = plan.waves;
    }
    if (getenv("OFX_PAIR_DEBUG")) { // the plan, once per shape
        fprintf(stderr, "ofx pair plan: window %d tile %d items %d capacity %d:", 2 * radius + 1, out_w, n, capacity);
        if (fits) fprintf(stderr, " waves %d segments %d S %d; tile columns", plan.waves, plan.segments, plan.S);
        else fprintf(stderr, " none fits (one strip per wave); tile columns");
        for (int i = 0; i < n; ++i) fprintf(stderr, " %d", ofx_div_up(items[i].w, out_w));
        fprintf(stderr, "\n");
    }
    (*cache)->entries.push_back(e);
    *out = PairPlanDev{e.d_segs, e.waves};
    return OFX_OK;
}

namespace {

int lk_build_levels(const ofx_lk_desc *d, int n, int window, int mode, int32_t *d_sums, LkLevelIn *lv, int *count)
{
    OFX_REQUIRE(d != nullptr && n >= 1 && n <= OFX_MAX_LK_ITEMS, "ofx_lk_levels: bad descriptor count %d", n);
    OFX_REQUIRE(window >= 3 && (window & 1), "ofx_lk_level: window must be odd and >= 3 (got %d)", window);
    OFX_REQUIRE(mode == OFX_MODE_COMPAT_CPU || mode == OFX_MODE_LK_FLOAT || mode == OFX_MODE_LK_FLOAT_FAST, "ofx_lk_level: bad mode %d", mode);
    const int radius = window >> 1;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const ofx_geom *g = &d[i].geom;
        OFX_TRY(ofx_check_geom(g, "ofx_lk_level"));
        OFX_REQUIRE(d[i].d_prev && d[i].d_next && (d[i].d_flow || d_sums), "ofx_lk_level: null pointer");
        OFX_REQUIRE(((uintptr_t)d[i].d_prev & 3) == 0 && ((uintptr_t)d[i].d_next & 3) == 0, "ofx_lk_level: planes must be 4-byte aligned");
        // (the marches store a flow row as 8-byte pairs and as 16-byte pieces declared 8-byte aligned: lk_body.h, lk_body_buf.h)
        OFX_REQUIRE(((uintptr_t)d[i].d_flow & 7) == 0, "ofx_lk_level: d_flow must be 8-byte aligned");
        OFX_REQUIRE(d[i].flow_row0 <= g->out_y0, "ofx_lk_level: flow_row0 %d > out_y0 %d", d[i].flow_row0, g->out_y0);
        OFX_TRY(ofx_check_halo(g, radius + 1, "ofx_lk_level"));
        if (g->out_y1 <= g->out_y0) continue;
        LkArgs a{};
        a.prev = d[i].d_prev;
        a.next = d[i].d_next;
        a.uv = d[i].d_uv;
        a.accumulate = d[i].accumulate;
        a.min_det = d[0].min_det; // one value per launch
        a.flow = d[i].d_flow;
        a.sums = d_sums;
        // plane stride of the inspection output = rows from flow_row0 to out_y1
        a.sums_plane = (size_t)(g->out_y1 - d[i].flow_row0) * (size_t)g->w;
        a.w = g->w;
        a.h = g->h;
        a.pitch = g->pitch;
        a.row0 = g->row0;
        a.row_end = g->row0 + g->rows;
        a.out_y0 = g->out_y0;
        a.out_y1 = g->out_y1;
        a.flow_row0 = d[i].flow_row0;
        OFX_REQUIRE((d[i].d_warp_out != nullptr) == (d[0].d_warp_out != nullptr) && (d[i].accumulate != 0) == (d[0].accumulate != 0),
                    "ofx_lk_levels: accumulate and d_warp_out must be set for all descriptors of a launch or for none");
        if (d[i].d_warp_out) { // the launch also writes the next iteration's warped image (lk_body_warp.h)
            OFX_REQUIRE(!d_sums && d[i].d_warp_src && d[i].d_flow, "ofx_lk_levels: d_warp_out needs d_warp_src and d_flow");
            OFX_REQUIRE(d[i].d_warp_out != d[i].d_next && d[i].d_warp_out != d[i].d_warp_src && d[i].d_warp_out != d[i].d_prev,
                        "ofx_lk_levels: d_warp_out must be a plane of its own");
            OFX_REQUIRE(((uintptr_t)d[i].d_warp_src & 3) == 0 && ((uintptr_t)d[i].d_warp_out & 3) == 0, "ofx_lk_levels: d_warp_src and d_warp_out must be 4-byte aligned");
            a.warp_src = d[i].d_warp_src;
            a.warp_out = d[i].d_warp_out;
            a.warp_scale = d[i].warp_scale;
            a.warp_status = d[i].d_warp_status;
            a.warp_status_bit = d[i].warp_status_bit;
            OFX_REQUIRE(a.warp_status == nullptr || (a.warp_status_bit >= 0 && a.warp_status_bit < 31), "ofx_lk_levels: bad warp_status_bit");
        }
        lv[m].a = a;
        ++m;
    }
    *count = m;
    return OFX_OK;
}

int lk_dispatch(const ofx_lk_desc *d, int n, int window, int mode, int32_t *d_sums, void *stream)
{
    LkLevelIn lv[OFX_MAX_LK_ITEMS];
    int m = 0;
    OFX_TRY(lk_build_levels(d, n, window, mode, d_sums, lv, &m));
    if (m == 0) return OFX_OK;
    ofx_plan::LkItem items[OFX_MAX_LK_ITEMS];
    for (int i = 0; i < m; ++i) items[i] = ofx_launch::lk_item(lv[i].a);
    const int radius = window >> 1;
    ofx_plan::LkVariant v;
    char err[160];
    const int rc = ofx_plan::lk_levels_variant(items, m, radius, mode, d_sums != nullptr, ofx_launch::lk_switches(), &v, err, sizeof err);
    if (rc != OFX_OK) {
        ofx_set_error("%s", err);
        return rc;
    }
    hipStream_t st = ofx_stream(stream);
    if (v.family == ofx_plan::kLkLevels) {
        if (v.mode == OFX_MODE_COMPAT_CPU) return ofx_launch::levels<OFX_MODE_COMPAT_CPU, false>(radius, lv, m, v.sums, st);
        return v.fast ? ofx_launch::levels<OFX_MODE_LK_FLOAT, true>(radius, lv, m, false, st) : ofx_launch::levels<OFX_MODE_LK_FLOAT, false>(radius, lv, m, v.sums, st);
    }
    auto run = [&](auto FAST) {
        constexpr bool F = decltype(FAST)::value;
        switch (v.iter) {
        case ofx_plan::kIterAdd: return ofx_launch::iter<OFX_MODE_LK_FLOAT, F, ofx_plan::kIterAdd>(radius, lv, m, v.deep, st);
        case ofx_plan::kIterAddWarp: return ofx_launch::iter<OFX_MODE_LK_FLOAT, F, ofx_plan::kIterAddWarp>(radius, lv, m, v.deep, st);
        case ofx_plan::kIterSetWarp: return ofx_launch::iter<OFX_MODE_LK_FLOAT, F, ofx_plan::kIterSetWarp>(radius, lv, m, v.deep, st);
        default: return ofx_launch::iter<OFX_MODE_LK_FLOAT, F, ofx_plan::kIterAddWarpRows>(radius, lv, m, v.deep, st);
        }
    };
    return v.fast ? run(std::true_type{}) : run(std::false_type{});
}

} // namespace

extern "C" int ofx_stream_launch(const ofx_stream_stages *g, int window, int mode, void *stream)
{
    OFX_REQUIRE(g != nullptr, "ofx_stream_launch: null argument");
    OFX_REQUIRE(window >= 3 && (window & 1), "ofx_stream_launch: window must be odd and >= 3 (got %d)", window);
    OFX_REQUIRE(mode == OFX_MODE_COMPAT_CPU || mode == OFX_MODE_LK_FLOAT || mode == OFX_MODE_LK_FLOAT_FAST, "ofx_stream_launch: bad mode %d", mode);
    OFX_REQUIRE(g->n_pyr >= 0 && g->n_pyr <= OFX_STREAM_MAX_BATCH && g->n_corner >= 0 && g->n_corner <= OFX_STREAM_MAX_BATCH,
                "ofx_stream_launch: at most %d frames / pairs per tick", OFX_STREAM_MAX_BATCH);
    StreamArgs S{};
    size_t lds = 0;
    int stage_blocks[kPyrStages] = {0};
    int any = 0;
    // marching-pyramid waves wanted per frame: all the frames of the tick together ~0.85 per SIMD (see ofx_pyramid_march_args)
    static const int simds = [] {
        int dev = 0, cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        return 4 * cus;
    }();
    const int pyr_target = g->n_pyr > 0 ? env_int("OFX_PYR_WAVES", simds * 85 / 100) / g->n_pyr : 0;
    for (int i = 0; i < g->n_pyr; ++i) {
        const ofx_pyramid_stage &P = g->pyr[i];
        if (P.levels < 2) continue;
        int items = 0;
        OFX_TRY(ofx_pyramid_march_args(P.d_frame, P.frame_pitch, P.w, P.h, P.d_levels, P.pitches, P.levels, P.d_levels[0], P.pitches[0],
                                       P.windowed ? P.row0 : nullptr, P.windowed ? P.rows : nullptr, pyr_target, &S.pyr[2 * i], &items));
        stage_blocks[2 * i] = ofx_div_up(items, 4);
        if (P.patch_levels >= 2) {
            OFX_REQUIRE(P.patch_w > 0 && P.patch_h > 0 && P.patch_w <= P.w && P.patch_h <= P.h,
                        "ofx_stream_launch: the patch must lie inside the frame");
            OFX_TRY(ofx_pyramid_march_args(P.d_frame, P.frame_pitch, P.patch_w, P.patch_h, P.d_patch_levels, P.patch_pitches, P.patch_levels,
                                           P.d_patch_levels[0], P.patch_pitches[0], nullptr, nullptr, 16, &S.pyr[2 * i + 1], &items));
            stage_blocks[2 * i + 1] = ofx_div_up(items, 4);
        }
        any += stage_blocks[2 * i] + stage_blocks[2 * i + 1];
    }
    int n_clv = 0, n_build = 0;
    for (int i = 0; i < g->n_corner; ++i) {
        const ofx_corner_stage &C = g->corner[i];
        OFX_REQUIRE(C.levels > 0, "ofx_stream_launch: empty corner stage");
        OFX_REQUIRE(n_clv + C.levels <= OFX_MAX_LK_ITEMS, "ofx_stream_launch: the corner stages have more than %d (pair, level) items", OFX_MAX_LK_ITEMS);
        OFX_TRY(ofx_corner_args(C.level, C.levels, window, mode, C.d_uv, C.cols, C.d_status, &C.shard_rows[0][0], &S.corner[i], S.corner_lv + n_clv));
        S.corner[i].lv0 = n_clv;
        n_clv += C.levels;
        const bool reloc = C.levels >= 2 && C.d_patch_reloc[1] != nullptr;
        S.corner[i].pair_status = C.d_pair_status;
        if (C.build_patch || reloc) {
            // the chain's patch pyramids are built (and, when a shift leaves them, rebuilt elsewhere) by its own block: one
            // geometry for all the chains of a launch
            OFX_REQUIRE(C.levels >= 2 && C.patch_w > 0 && C.patch_h > 0, "ofx_stream_launch: corner stage %d: incomplete patch description", i);
            OFX_REQUIRE(!C.build_patch || (C.d_patch_src[0] && C.d_patch_src[1] && C.d_patch[0][1] && C.d_patch[1][1]),
                        "ofx_stream_launch: corner stage %d: incomplete patch description", i);
            uint8_t *const *planes = C.build_patch ? C.d_patch[0] : C.d_patch_reloc; // (the set whose layout defines the offsets)
            PatchBuild pb{};
            pb.n = C.levels - 1;
            pb.frame_stride = C.build_patch ? (int)(C.d_patch[1][1] - C.d_patch[0][1]) : 0;
            for (int k = 0; k < C.levels; ++k) {
                pb.pw[k] = C.patch_w >> k;
                pb.ph[k] = C.patch_h >> k;
                pb.pitch[k] = k ? C.patch_pitch[k] : 0;
                pb.off[k] = k ? (int)(planes[k] - planes[1]) : 0;
                OFX_REQUIRE(pb.pw[k] > 0 && pb.ph[k] > 0, "ofx_stream_launch: the patch is too small for %d levels", C.levels);
                if (k) {
                    OFX_REQUIRE(planes[k] != nullptr && (C.patch_pitch[k] & 3) == 0 && C.patch_pitch[k] >= ((pb.pw[k] + 3) & ~3) && ((uintptr_t)planes[k] & 3) == 0,
                                "ofx_stream_launch: corner stage %d: bad patch plane at level %d", i, k);
                    OFX_REQUIRE(!C.build_patch || C.d_patch[1][k] == C.d_patch[0][k] + pb.frame_stride,
                                "ofx_stream_launch: corner stage %d: bad patch plane at level %d", i, k);
                    OFX_REQUIRE(!reloc || (C.d_patch_reloc[k] != nullptr && C.d_patch_reloc[k] - C.d_patch_reloc[1] == pb.off[k] && ((uintptr_t)C.d_patch_reloc[k] & 3) == 0),
                                "ofx_stream_launch: corner stage %d: the relocated patch planes must be laid out like the patch planes (level %d)", i, k);
                    OFX_REQUIRE(((C.patch_w >> (k - 1)) & 1) == 0 && ((C.patch_h >> (k - 1)) & 1) == 0, "ofx_stream_launch: the patch must have even dimensions below its top level");
                }
            }
            if (C.build_patch)
                for (int f = 0; f < 2; ++f)
                    OFX_REQUIRE((C.patch_src_pitch[f] & 3) == 0 && C.patch_src_pitch[f] >= C.patch_w && ((uintptr_t)C.d_patch_src[f] & 3) == 0,
                                "ofx_stream_launch: corner stage %d: bad patch source", i);
            if (reloc) {
                // the relocated build reads the whole next frame through level 0's descriptor, and the chain must be able to
                // place the patch around any target: whole level-0 planes, a patch inside the frame, room for the window at
                // the coarsest level (its stencils span radius + 3 pixels; one more for the plane's first column / row)
                const ofx_geom &g0 = C.level[0].geom;
                OFX_REQUIRE(g0.row0 == 0 && g0.rows == g0.h && (C.cols[0] == 0 || C.cols[0] >= g0.w),
                            "ofx_stream_launch: corner stage %d: the repair needs level 0 to be the whole frames", i);
                OFX_REQUIRE(C.patch_w <= g0.w && C.patch_h <= g0.h, "ofx_stream_launch: corner stage %d: the patch must lie inside the frame", i);
                const int lc = C.levels - 1, need = (window >> 1) + 5;
                OFX_REQUIRE((pb.pw[lc] >= need || pb.pw[lc] >= (g0.w >> lc)) && (pb.ph[lc] >= need || pb.ph[lc] >= (g0.h >> lc)),
                            "ofx_stream_launch: corner stage %d: a %dx%d patch leaves %dx%d at the coarsest level, the repair needs %d", i, C.patch_w,
                            C.patch_h, pb.pw[lc], pb.ph[lc], need);
                S.corner[i].reloc = C.d_patch_reloc[1];
            }
            if (S.patch.n == 0) S.patch = pb;
            else OFX_REQUIRE(memcmp(&S.patch, &pb, sizeof pb) == 0, "ofx_stream_launch: the corner stages of a launch must share one patch geometry");
            if (C.build_patch) {
                S.patch_slot[i] = PatchBuildSlot{{C.d_patch_src[0], C.d_patch_src[1]}, {C.patch_src_pitch[0], C.patch_src_pitch[1]}, C.d_patch[0][1]};
                ++n_build;
            }
        }
    }
    OFX_REQUIRE(n_build == 0 || n_build == g->n_corner, "ofx_stream_launch: either every corner stage builds its patch or none does");
    S.patch_build = n_build > 0 ? 1 : 0;
    S.n_corner = g->n_corner;
    LkLevelIn lv[OFX_MAX_LK_ITEMS];
    int m = 0;
    if (g->n_lk > 0) {
        OFX_REQUIRE(!g->lk[0].accumulate, "ofx_stream_launch: a tick's LK stage is iteration 1 (no accumulate)");
        OFX_REQUIRE(g->lk[0].d_warp_out == nullptr || mode != OFX_MODE_COMPAT_CPU, "ofx_stream_launch: d_warp_out needs mode lk_float");
        OFX_TRY(lk_build_levels(g->lk, g->n_lk, window, mode, nullptr, lv, &m));
    }
    // the stream kernel's LK stage addresses planes and flow through buffer resources with 32-bit offsets (lk_body_buf.h)
    ofx_plan::LkItem items[OFX_MAX_LK_ITEMS];
    for (int i = 0; i < m; ++i) {
        items[i] = ofx_launch::lk_item(lv[i].a);
        OFX_REQUIRE(ofx_plan::fits_buffer_offsets(items[i]),
                    "ofx_stream_launch: level %dx%d is too large for one launch item (planes and flow rows must stay below 2 GB: "
                    "shard the level by rows)", items[i].w, items[i].h);
    }
    if (any == 0 && m == 0 && g->n_corner == 0) return OFX_OK;
    hipStream_t st = ofx_stream(stream);
    OFX_REQUIRE(g->deep_fetch >= -1 && g->deep_fetch <= 1, "ofx_stream_launch: deep_fetch must be -1, 0 or +1 (got %d)", g->deep_fetch);
    const ofx_plan::LkVariant v = ofx_plan::lk_tick_variant(items, m, mode, g->deep_fetch, ofx_launch::lk_switches());
    const int radius = window >> 1;
    if (v.mode == OFX_MODE_COMPAT_CPU) return ofx_launch::stream<OFX_MODE_COMPAT_CPU, false>(radius, lv, m, v.deep, v.many, S, stage_blocks, lds, st);
    auto tick = [&](auto FAST) {
        constexpr bool F = decltype(FAST)::value;
        switch (v.iter) { // (levels below 2 GB: checked above)
        case ofx_plan::kIterSetWarp: return ofx_launch::stream<OFX_MODE_LK_FLOAT, F, ofx_plan::kIterSetWarp>(radius, lv, m, v.deep, v.many, S, stage_blocks, lds, st);
        case ofx_plan::kIterSetWarpRows: return ofx_launch::stream<OFX_MODE_LK_FLOAT, F, ofx_plan::kIterSetWarpRows>(radius, lv, m, v.deep, v.many, S, stage_blocks, lds, st);
        default: return ofx_launch::stream<OFX_MODE_LK_FLOAT, F>(radius, lv, m, v.deep, v.many, S, stage_blocks, lds, st);
        }
    };
    return v.fast ? tick(std::true_type{}) : tick(std::false_type{});
}

// Debug / measurement hook (tools/stream_timeline.py): with a device buffer of 8 * capacity_blocks uint64 set, every
// wave of every later ofx_stream_launch records its start and end time there; first[] (2 * OFX_STREAM_MAX_BATCH + 1 ints) receives the block ranges of
// the last launch.  d_buf = NULL switches it off.
extern "C" int ofx_debug_stream_trace(unsigned long long *d_buf, int capacity_blocks, int *first)
{
    g_stream_trace = d_buf;
    g_stream_trace_blocks = d_buf ? capacity_blocks : 0;
    if (first)
        for (int i = 0; i <= kPyrStages; ++i) first[i] = g_trace_header[i];
    return OFX_OK;
}

extern "C" int ofx_lk_levels(const ofx_lk_desc *levels, int n, int window, int mode, void *stream)
{
    return lk_dispatch(levels, n, window, mode, nullptr, stream);
}

// Two refinement iterations in one launch (lk_body_pair.h): descriptor i is what ofx_lk_levels takes for the FIRST of them
// (accumulate set, d_next = the warped image of the iteration before), d_flow_in[i] holds the flow so far and d_flow receives the
// flow after the second -- a different buffer: waves read d_flow_in at pixels whose owner may already have stored.  With
// d_warp_out the launch also writes the warped image of the iteration after the second (d_warp_src is needed either way: the
// first iteration's warp runs inside the launch).
int ofx_lk_levels_pair(const ofx_lk_desc *d, const float *const *d_flow_in, int n, int window, int mode, const ofx_pair_opts *opts, void *stream)
{
    LkLevelIn lv[OFX_MAX_LK_ITEMS];
    int m = 0;
    OFX_REQUIRE(d != nullptr && d_flow_in != nullptr && n >= 1 && n <= OFX_MAX_LK_ITEMS, "ofx_lk_levels_pair: bad arguments");
    OFX_REQUIRE(mode == OFX_MODE_LK_FLOAT || mode == OFX_MODE_LK_FLOAT_FAST, "ofx_lk_levels_pair: mode %d not supported", mode);
    OFX_REQUIRE(window >= 3 && (window & 1) && (window >> 1) <= kLkPairMaxR, "ofx_lk_levels_pair: window %d not supported", window);
    OFX_TRY(lk_build_levels(d, n, window, mode, nullptr, lv, &m));
    OFX_REQUIRE(m == n, "ofx_lk_levels_pair: empty level");
    const bool wout = d[0].d_warp_out != nullptr;
    for (int i = 0; i < n; ++i) {
        LkArgs &a = lv[i].a;
        OFX_REQUIRE(a.accumulate && a.uv == nullptr && a.flow != nullptr && d_flow_in[i] != nullptr && d_flow_in[i] != a.flow && d[i].d_warp_src != nullptr,
                    "ofx_lk_levels_pair: needs accumulate, no d_uv, d_warp_src and two distinct flow buffers");
        OFX_REQUIRE(a.row0 == 0 && a.row_end == a.h && a.out_y0 == 0 && a.out_y1 == a.h && a.flow_row0 == 0, "ofx_lk_levels_pair: whole levels only");
        OFX_REQUIRE(ofx_plan::fits_buffer_offsets(ofx_launch::lk_item(a)), "ofx_lk_levels_pair: levels must stay below 2 GB");
        a.flow_in = d_flow_in[i];
        a.warp_src = d[i].d_warp_src;
        a.warp_scale = d[i].warp_scale;
    }
    hipStream_t st = ofx_stream(stream);
    const int radius = window >> 1;
    if (mode == OFX_MODE_LK_FLOAT_FAST) return wout ? ofx_launch::iter_pair<true, true>(radius, lv, n, opts, st) : ofx_launch::iter_pair<true, false>(radius, lv, n, opts, st);
    return wout ? ofx_launch::iter_pair<false, true>(radius, lv, n, opts, st) : ofx_launch::iter_pair<false, false>(radius, lv, n, opts, st);
}

extern "C" int ofx_lk_level(const uint8_t *d_prev, const uint8_t *d_next, const ofx_geom *g, int window, int mode,
                            float *d_flow, int flow_row0, void *stream)
{
    OFX_REQUIRE(d_flow && g, "ofx_lk_level: null argument");
    ofx_lk_desc d{d_prev, d_next, *g, d_flow, flow_row0, nullptr, 0, 0.0f};
    return lk_dispatch(&d, 1, window, mode, nullptr, stream);
}

extern "C" int ofx_lk_level_sums(const uint8_t *d_prev, const uint8_t *d_next, const ofx_geom *g, int window, int mode,
                                 int32_t *d_sums5, int flow_row0, void *stream)
{
    OFX_REQUIRE(d_sums5 && g, "ofx_lk_level_sums: null argument");
    ofx_lk_desc d{d_prev, d_next, *g, nullptr, flow_row0, nullptr, 0, 0.0f};
    return lk_dispatch(&d, 1, window, mode, d_sums5, stream);
}
