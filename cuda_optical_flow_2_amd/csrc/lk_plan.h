// What an LK launch is before it touches the device: which kernel of the lk_inst_*.hip families runs, whether it takes the deep
// fetch, and which strip of which tile column of which item every wave marches.  Plain host code without HIP in it, like iter_plan.h,
// pair_plan.h and session_plan.h: tools/lk_plan_main.cpp prints the variant and the strip table of a launch description,
// tests/test_lk_plan.py checks both against a transcription of the code that used to hold this arithmetic (tests/lk_plan_ref.py).
// lk_level.hip builds the items and reads the switches, lk_launch.h asks the device for its CUs and the kernel's occupancy.
#pragma once

#include <stdio.h>

#include "ofx.h"
#include "session_plan.h"

namespace ofx_plan {

// ITER of lk_wave_buf (lk_body_buf.h), of lk_iter_kernel and -- as WOUT -- of the stream tick's LK stage: what the buffer march does
// with a row's result (refinement iterations of lk_iter).  The values are template arguments of the kernels.
constexpr int kIterSet = 0;         // flow = result: the reference's level, and a tick whose pairs have one iteration
constexpr int kIterAdd = 1;         // flow += result, the row's old flow fetched through the flow's own resource with the step's rows
// the same, and the march also writes the warped image the NEXT iteration reads (lk_body_warp.h): the row's new flow is in registers
// after the add, the warp's first stage runs there and issues its tap loads, the second stage and the row's store follow one step
// later (whole levels)
constexpr int kIterAddWarp = 2;
constexpr int kIterSetWarp = 3;     // iteration 1 of pairs that have more: flow = result, and the warped image of iteration 2
// kIterAddWarp / kIterSetWarp on the row window of a shard: the planes hold rows [row0, row_end) only, a tap row outside them is
// reported (LkArgs::warp_status).  kIterSetWarpRows runs in the stream tick only.
constexpr int kIterAddWarpRows = 4;
constexpr int kIterSetWarpRows = 5;
constexpr bool iter_adds(int iter) { return iter == kIterAdd || iter == kIterAddWarp || iter == kIterAddWarpRows; }
constexpr bool iter_warps(int iter) { return iter >= kIterAddWarp; }
constexpr bool iter_row_window(int iter) { return iter >= kIterAddWarpRows; }

constexpr int lk_max_radius(int mode) { return mode == OFX_MODE_COMPAT_CPU ? 12 : 11; } // windows up to 25x25 / 23x23

// What the decisions read of a launch item (an LkArgs, lk_body.h).
struct LkItem {
    int w, h, pitch, row0, row_end; // the planes hold rows [row0, row_end) of a w x h level
    int out_y0, out_y1, flow_row0;  // the rows the launch writes; the flow buffer's first row
    int accumulate, warp_out;       // flow += result; the launch also writes a warped image (both: all items of a launch or none)
};
inline bool row_window(const LkItem &a) { return a.row0 != 0 || a.row_end != a.h; }
// The buffer march addresses an item's planes and its flow rows through buffer resources with 32-bit offsets (lk_body_buf.h)
inline bool fits_buffer_offsets(const LkItem &a) { return fits_buffer_offsets(a.row_end - a.row0, a.pitch, a.out_y1 - a.flow_row0, a.w); }
inline long largest_level(const LkItem *it, int n)
{
    long px = 0;
    for (int i = 0; i < n; ++i) px = (long)it[i].w * it[i].h > px ? (long)it[i].w * it[i].h : px;
    return px;
}

// The switches the LK launches read from the environment (lk_switches, lk_level.hip): OFX_LK_MIN_STRIP at every launch, the others
// once per process.
struct LkSwitches {
    int lk_dma = -1;        // OFX_LK_DMA = 0 / 1: the tick's deep fetch off / on (< 0: not set)
    int iter_dma = -1;      // OFX_ITER_DMA = 0 / 1: the iteration launches' (< 0: not set)
    int min_strip = 8;      // OFX_LK_MIN_STRIP: no strip below this many rows, so that a strip's priming rows stay a minor cost
    int waves_per_simd = 0; // OFX_LK_WAVES_PER_SIMD, OFX_LK_FILL (per cent), OFX_LK_TARGET_WAVES: planner experiments (0: not set)
    int fill = 0;
    int target_waves = 0;
};

// ---- the deep fetch -------------------------------------------------------------------------------------------------------------
// The rows of a step are fetched two steps ahead through LDS (lk_body_buf.h).  It pays where a step's row loads come from HBM --
// measured on MI355X (profiles/r03_ablation.txt): 8K, two frames per launch: 279 vs 295 us (-5 %); 4K with its frames in the
// Infinity Cache: 247 vs 237 us (+4 %: the form costs ~60 more scalar instructions per step, and the loads are short there) -- so it
// is chosen by the size of the largest level (deep_fetch_by_size).
// An iteration launch (8K, 10 iterations: 15 380 vs 15 110 Mpix/s; 4K: no difference beyond the +-1.5 % between runs): the switch,
// then the size.  session_plan_make asks the same question to decide that a session has no two-iteration form.
inline bool iter_deep_fetch(int iter_dma, long largest_px) { return iter_dma > 0 || (iter_dma < 0 && deep_fetch_by_size(largest_px)); }
// A tick: the switch, then the caller's hint, then the size.  WHERE the rows come from decides, not the level's size as such -- a
// ring of 4K or 1080p frames longer than the Infinity Cache gains 5 % / 3.5 % with the deep fetch, a warm one loses 2 %: the caller
// can say which (ofx_params.deep_fetch: +1 cold, -1 warm, 0 by size).
inline bool tick_deep_fetch(int lk_dma, int hint, long largest_px)
{
    const int want = lk_dma >= 0 ? (lk_dma > 0 ? 1 : -1) : hint;
    return want > 0 || (want == 0 && deep_fetch_by_size(largest_px));
}

// ---- the kernel variant ---------------------------------------------------------------------------------------------------------
enum LkFamily { kLkLevels, kLkIter, kLkStream }; // lk_level_kernel / lk_iter_kernel / stream_kernel (lk_inst_{levels,iter,stream}_*.hip)
struct LkVariant {
    int family;
    int mode;  // the kernel's MODE: OFX_MODE_COMPAT_CPU or OFX_MODE_LK_FLOAT
    bool fast; // ... and its FAST: lk_float's solve in its <= 1 ulp formulation
    bool sums; // kLkLevels: the inspection variant, which does not depend on the solve
    int iter;  // kLkIter: ITER 1..4; kLkStream: WOUT 0, 3 or 5
    bool deep; // kLkIter, kLkStream: the deep fetch
    bool many; // kLkStream: the tick carries two pairs or more (items of item 0's size)
};

// An ofx_lk_levels launch (lk_dispatch).  Refinement iterations -- accumulate and / or warp_out, no sums -- run on the buffer march:
// lk_float, levels below 2 GB; compat_cpu and larger levels accumulate in the old march, which cannot write the warped image.
// OFX_OK, or the code with its message in err.
inline int lk_levels_variant(const LkItem *it, int n, int radius, int mode, bool sums, const LkSwitches &sw, LkVariant *out, char *err, size_t err_len)
{
    LkVariant v{kLkLevels, mode == OFX_MODE_COMPAT_CPU ? OFX_MODE_COMPAT_CPU : OFX_MODE_LK_FLOAT, false, sums, kIterSet, false, false};
    const bool acc = it[0].accumulate != 0, wout = it[0].warp_out != 0;
    if ((acc || wout) && !sums) {
        bool small = true, rowwin = false; // rowwin: a shard's row window, where the warp reports taps it cannot reach
        for (int i = 0; i < n; ++i) small = small && fits_buffer_offsets(it[i]), rowwin = rowwin || row_window(it[i]);
        if (wout && !(small && mode != OFX_MODE_COMPAT_CPU)) {
            snprintf(err, err_len, "ofx_lk_levels: d_warp_out needs mode lk_float and levels below 2 GB");
            return OFX_E_INVALID;
        }
        if (wout && rowwin && !acc) {
            snprintf(err, err_len, "ofx_lk_levels: iteration 1 with d_warp_out on a row window runs in the stream tick only");
            return OFX_E_INVALID;
        }
        if (small && mode != OFX_MODE_COMPAT_CPU) {
            v.family = kLkIter;
            v.iter = wout ? (acc ? (rowwin ? kIterAddWarpRows : kIterAddWarp) : kIterSetWarp) : kIterAdd;
            v.deep = iter_deep_fetch(sw.iter_dma, largest_level(it, n));
        }
    }
    v.fast = mode == OFX_MODE_LK_FLOAT_FAST && (v.family == kLkIter || !sums);
    if (radius < 1 || radius > lk_max_radius(v.mode)) {
        snprintf(err, err_len, "ofx_lk_level: window %d not supported in mode %d", 2 * radius + 1, v.mode);
        return OFX_E_UNSUPPORTED;
    }
    *out = v;
    return OFX_OK;
}

// A stream tick's LK stage (ofx_stream_launch, which has checked the items: iteration 1, lk_float if it writes warped images, below
// 2 GB).  A tick that also writes warped images measured slower with the deep fetch (8K: 440 vs 416 us) and never takes it.
inline LkVariant lk_tick_variant(const LkItem *it, int n, int mode, int hint, const LkSwitches &sw)
{
    LkVariant v{kLkStream, mode == OFX_MODE_COMPAT_CPU ? OFX_MODE_COMPAT_CPU : OFX_MODE_LK_FLOAT, mode == OFX_MODE_LK_FLOAT_FAST, false, kIterSet, false, false};
    bool rowwin = false;
    int pairs = 0;
    for (int i = 0; i < n; ++i) rowwin = rowwin || row_window(it[i]), pairs += it[i].w == it[0].w && it[i].h == it[0].h ? 1 : 0;
    if (v.mode != OFX_MODE_COMPAT_CPU && n > 0 && it[0].warp_out) v.iter = rowwin ? kIterSetWarpRows : kIterSetWarp;
    v.deep = v.iter == kIterSet && tick_deep_fetch(sw.lk_dma, hint, largest_level(it, n));
    v.many = pairs >= 2;
    return v;
}

// ---- the strips -----------------------------------------------------------------------------------------------------------------
// Item i is tiles_x[i] tile columns of out_w output columns; each is cut into strips of strip_h[i] rows from out_y0 on, one per wave.
// The kernels decode wave b of [first_block[i], first_block[i + 1]) as tile b % tiles_x, strip b / tiles_x (b counted from the
// item's first).
struct LkStrips {
    int n, H, blocks; // H: the common strip height
    int tiles_x[OFX_MAX_LK_ITEMS], strip_h[OFX_MAX_LK_ITEMS], first_block[OFX_MAX_LK_ITEMS + 1];
};
inline int div_up(int a, int b) { return (a + b - 1) / b; }

// One strip height for all items (so all waves run about equally long): the smallest that keeps the wave count within `capacity`
// (lk_wave_capacity), but at least min_h; an item with fewer rows is one strip.
// The grid is sized to fit in ONE residency round: every wave runs for the whole kernel, so a second, partly filled
// round would nearly double the run time.  Items with out_y1 > out_y0, min_h >= 1.  Returns the wave count.
inline int lk_strips(const LkItem *it, int n, int out_w, int min_h, int capacity, LkStrips *out)
{
    int max_rows = 1;
    for (int i = 0; i < n; ++i) max_rows = it[i].out_y1 - it[i].out_y0 > max_rows ? it[i].out_y1 - it[i].out_y0 : max_rows;
    auto height = [&](int i, int H) {
        const int hi = H < min_h ? min_h : H, rows = it[i].out_y1 - it[i].out_y0;
        return hi < rows ? hi : rows;
    };
    auto item_waves = [&](int i, int H) { return (long)div_up(it[i].w, out_w) * div_up(it[i].out_y1 - it[i].out_y0, height(i, H)); };
    int H = min_h;
    for (; H < max_rows; ++H) {
        long waves = 0;
        for (int i = 0; i < n; ++i) waves += item_waves(i, H);
        if (waves <= (long)capacity) break;
    }
    LkStrips &s = *out;
    s.n = n, s.H = H, s.blocks = 0;
    for (int i = 0; i < n; ++i) {
        s.tiles_x[i] = div_up(it[i].w, out_w);
        s.strip_h[i] = height(i, H);
        s.first_block[i] = s.blocks;
        s.blocks += s.tiles_x[i] * div_up(it[i].out_y1 - it[i].out_y0, s.strip_h[i]);
    }
    s.first_block[n] = s.blocks;
    return s.blocks;
}

// ---- the capacity ---------------------------------------------------------------------------------------------------------------
// Number of LK waves a launch is planned for, on `cus` CUs of four SIMDs that hold `occ` waves of the kernel each.  Every LK wave runs
// for the whole launch, so what matters is how many of them share a SIMD: fewer leave issue slots empty, more shorten the strips
// (each strip pays its priming rows), and a count that is not a whole number per SIMD makes the fuller SIMDs set the time.  Measured
// on MI355X (one 4K pair, 9x9): with 2R priming steps per strip 3 per SIMD was the optimum; with the folded priming (R + 1 steps,
// lk_body.h) it is 4 -- 48.9 / 42.0 / 40.4 / 41.6 us at 2 / 3 / 4 / 5.  `reserve` slots per SIMD are left to the other stages of
// the stream kernel.  `full_fill`: per cent of the slots a plan that needs every slot may use.
inline int lk_wave_capacity(int cus, int occ, int reserve, int dflt_per_simd, int full_fill, const LkSwitches &sw)
{
    int per_simd = sw.waves_per_simd > 0 ? sw.waves_per_simd : dflt_per_simd;
    if (per_simd > occ - reserve) per_simd = occ - reserve;
    if (per_simd < 1) per_simd = 1;
    // with wave slots to spare the plan may use the whole target (an uneven placement still fits in one round); a plan
    // that needs every slot keeps 5 % back, because a second, mostly empty round would double the run time
    const int fill = sw.fill > 0 ? sw.fill : (per_simd < occ ? 100 : full_fill);
    return sw.target_waves > 0 ? sw.target_waves : (int)((long)cus * 4 * per_simd * fill / 100);
}
// The four call sites: reserve, waves per SIMD, full_fill.
constexpr int kLkFullFill = 95;
constexpr int kLkWavesPerSimd = 4;   // lk_level_kernel and lk_iter_kernel
// Two iterations per launch: two waves per SIMD (a wave holds the registers of two marches), and every slot is planned for: a SIMD
// that gets one wave idles half the launch while the full ones set its time -- measured at 4K, 9x9: 1 945 waves (95 %) 2.137 ms per
// tick, 2 048 waves 1.992, 1 800 waves 2.463 (the block is one wave of 19.1 KB: eight fit every CU, so a plan of cus x 8 waves
// still runs in one round)
constexpr int kPairWavesPerSimd = 2, kPairFullFill = 100;
// Next to the staging blocks of a tick, which get one slot per SIMD, the LK stage does best with 2 waves per SIMD when the tick
// carries one pair and 4 when it carries more (measured, 4K: one pair 58.2 / 59.8 us per frame at 2 / 3; two pairs 59.7 / 57.2 /
// 56.5 at 2 / 3 / 4)
constexpr int kTickReserve = 1;
constexpr int tick_waves_per_simd(bool many) { return many ? 4 : 2; }

} // namespace ofx_plan
