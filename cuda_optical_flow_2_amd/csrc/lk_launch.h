// Kernels, planner and launchers of the fused level kernel and of the stream kernel, as templates: included by lk_level.hip
// (entry points, argument checks) and, through lk_inst.h, by the lk_inst_*.hip translation units, each of which instantiates one
// family (declared at the end of this file) -- the radii 1..12 of a family are ~90 s of hipcc on one core, six families in
// parallel are ~40 s.
#pragma once

#include <stdio.h>

#include "corner_body.h"
#include "lk_body.h"
#include "lk_plan.h"
#include "pair_plan.h"
#include "pyr_march.h"
#include "stages_body.h"

using namespace ofx_dev;

namespace ofx_launch { // types that cross translation units
constexpr int kPyrStages = 2 * OFX_STREAM_MAX_BATCH; // per frame of the tick: its pyramid and its top-left patch pyramid
using ofx_dev::kCornerScratch;                       // LDS of a corner block: the chain's floats, then the cached corners
struct StreamArgs {
    LkTable lk;
    PyrMarchArgs pyr[kPyrStages];
    CornerHead corner[OFX_STREAM_MAX_BATCH];
    CornerLevel corner_lv[OFX_MAX_LK_ITEMS]; // the chains' levels, flat: chain i's level k at [corner[i].lv0 + k]
    // two-stage pipeline: the corner blocks build the patch pyramids their chains read (same geometry for every chain)
    PatchBuild patch;   // geometry of the patch planes (n > 0 when the corner blocks build and / or relocate them)
    int patch_build;    // the corner blocks build the patch pyramids of both frames first (two-stage pipeline)
    PatchBuildSlot patch_slot[OFX_STREAM_MAX_BATCH];
    // blocks [0, OFX_STREAM_MAX_BATCH) = one corner wave each; [.., first[0]) LK (four waves per block);
    // [first[i], first[i+1]) pyramid stage i (four marching waves per block, pyr_march.h).
    // The LK blocks come first and are planned for a whole number of waves per SIMD (lk_wave_capacity): they all start at
    // once and run for the whole launch, while the short staging blocks stream through the remaining slots underneath.
    int first[kPyrStages + 1];
    int n_corner;
    unsigned long long *trace; // optional (ofx_debug_stream_trace): per block, start and end time (100 MHz wall clock)
    int trace_blocks;
};
struct LkLevelIn {
    LkArgs a; // everything but strip_h / tiles_x, which the plan fills in (plan_table_g)
};
using ofx_plan::kPairMaxSegs;
using ofx_plan::PairSeg;
// The packed plan of a fused two-iteration launch (pair_plan.h) on the device: made and uploaded once per launch shape -- the
// radius, the items' sizes and the wave count -- and kept in the caller's cache (lk_level.hip).  segs = NULL: no plan fits (the
// launch keeps one strip per wave).
struct PairPlanDev {
    const PairSeg *segs;
    int waves;
};
int pair_plan_get(ofx_pair_cache **cache, int radius, int out_w, const LkLevelIn *lv, int n, int min_h, int capacity, PairPlanDev *out);
ofx_plan::LkSwitches lk_switches(); // the environment's (lk_level.hip)
inline ofx_plan::LkItem lk_item(const LkArgs &a)
{
    return ofx_plan::LkItem{a.w, a.h, a.pitch, a.row0, a.row_end, a.out_y0, a.out_y1, a.flow_row0, a.accumulate, a.warp_out != nullptr};
}
} // namespace ofx_launch

namespace {
using ofx_plan::kPairMaxSegs;
using ofx_plan::PairSeg;

constexpr int kLkMinWaves = 3; // A/B on MI355X: capping at 128 VGPRs (4 waves) spills in the marching loop and is slower
template <int R, int MODE, bool SUMS, bool FAST>
__global__ __launch_bounds__(64, kLkMinWaves) void lk_level_kernel(const LkTable T)
{
    __shared__ __attribute__((aligned(16))) uint8_t xlds[kLkWaveLds];
    lk_wave<R, MODE, SUMS, true, FAST>(T, (int)blockIdx.x, (int)threadIdx.x, xlds);
}

// A refinement iteration of lk_iter on the buffer march (lk_body_buf.h; ITER: lk_plan.h).
// kIterAddWarp needs 126 VGPRs in interior tiles and 130 in the tiles at the image's left and right edge (128 for 9x9: four waves per
// SIMD, three for the other windows).  Capping it at 128 everywhere spills 2-8 registers and measured 1-3 % slower at 1080p, 4K
// and 8K (profiles/r03_ablation.txt), so the cap stays at three waves.
// DMA: the rows are fetched two steps ahead through LDS (lk_body_buf.h; chosen per launch as for the stream kernel)
// The body is lk_wave's !SUMS && !MAY_ACC branch (lk_body.h), written out: with a call of lk_wave in its place hipcc allocates the
// scalar registers of the level search differently, and every lk_iter_kernel's code object changes.
template <int R, int MODE, bool FAST, int ITER, bool DMA = false>
__global__ __launch_bounds__(64, 3) void lk_iter_kernel(const LkTable T)
{
    __shared__ __attribute__((aligned(16))) uint8_t xlds[DMA ? kLkWaveLdsDma : kLkWaveLdsX];
    const int wave = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (wave >= T.first_block[T.n]) return;
    int level = 0, hi = T.n;
    while (hi - level > 1) {
        const int mid = (level + hi) >> 1;
        if (wave >= T.first_block[mid]) level = mid;
        else hi = mid;
    }
    const int tile = (wave - T.first_block[level]) % T.lv[level].tiles_x;
    const int cb0 = tile * TileGeom<R>::OUT_W - TileGeom<R>::LO_LANE * 4;
    if (cb0 >= 0 && cb0 + 256 <= T.lv[level].w) lk_wave_buf<R, MODE, FAST, true, DMA, ITER>(T, wave, lane, xlds);
    else lk_wave_buf<R, MODE, FAST, false, DMA, ITER>(T, wave, lane, xlds);
}

// Two refinement iterations per launch (lk_body_pair.h): the second trails the first by R + 2 rows in the same wave; flow and warped
// image between them stay in per-wave LDS rings (19.1 KB at 9x9).  Two waves per SIMD, planned for: a wave holds the registers of
// two marches.  WOUT: the second iteration also writes the warped image of the one after it.
// segs: the packed plan (pair_plan.h): wave w marches segments segs[kPairMaxSegs * w ...], one after the other; NULL: the plan of
// plan_table_g in T, one strip per wave.
template <int R, bool FAST, bool WOUT>
__global__ __launch_bounds__(64, 2) void lk_pair_kernel(const LkTable T, const PairSeg *__restrict__ segs)
{
    __shared__ __attribute__((aligned(16))) uint8_t xlds[pair_wave_lds(R)];
    const int wave = (int)blockIdx.x, lane = (int)threadIdx.x;
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const i32x4 *sg = reinterpret_cast<const i32x4 *>(segs) + kPairMaxSegs * wave;
    int nsteps = 0; // of the whole wave: its priority falls along all of its work
    int level = 0;
    if (segs) {
#pragma unroll
        for (int i = 0; i < kPairMaxSegs; ++i) {
            const i32x4 g = sg[i];
            nsteps += g.w > g.z ? g.w - g.z + pair_seg_steps(R) : 0;
        }
    } else {
        if (wave >= T.first_block[T.n]) return;
        int hi = T.n;
        while (hi - level > 1) {
            const int mid = (level + hi) >> 1;
            if (wave >= T.first_block[mid]) level = mid;
            else hi = mid;
        }
    }
    int q1 = 0, q2 = 0, q3 = 0;
    __builtin_amdgcn_s_setprio(3);
#pragma nounroll
    for (int i = 0; i < kPairMaxSegs; ++i) {
        int tile, y0, y1;
        if (segs) {
            const i32x4 g = sg[i];
            level = g.x, tile = g.y, y0 = g.z, y1 = g.w;
            if (y1 <= y0) break;
        } else {
            if (i > 0) break;
            const int block = wave - T.first_block[level];
            tile = block % T.lv[level].tiles_x;
            y0 = T.lv[level].out_y0 + (block / T.lv[level].tiles_x) * T.lv[level].strip_h;
            y1 = min(y0 + T.lv[level].strip_h, T.lv[level].out_y1);
            nsteps = y1 - y0 + pair_seg_steps(R);
        }
        if (i == 0) q1 = nsteps / 4, q2 = nsteps / 2, q3 = nsteps - nsteps / 4;
        else { // the rings and the exchange row are reused: what the segment before still reads of them comes first
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        const int cb0 = tile * TileGeomP<R>::OUT_W - TileGeomP<R>::LO_LANE * 4;
        if (cb0 >= 0 && cb0 + 256 <= T.lv[level].w) lk_wave_pair<R, FAST, true, WOUT>(T, level, tile, y0, y1, lane, xlds, q1, q2, q3);
        else lk_wave_pair<R, FAST, false, WOUT>(T, level, tile, y0, y1, lane, xlds, q1, q2, q3);
        const int done = y1 - y0 + pair_seg_steps(R);
        q1 -= done, q2 -= done, q3 -= done;
    }
}

// ---- the stream kernel: one launch = one pipeline tick ---------------------------------------------------------------
// A tick of a frame stream runs, as disjoint block ranges of ONE grid,
//     pyramid(newest frame(s))  |  corner flows(earlier pair(s))  |  fused LK(still earlier pair(s))
// Each stage consumes what earlier launches wrote, so there is no synchronisation inside the launch and none between
// streams; the small latency-bound stages run in the shadow of the VALU-bound LK stage.  Blocks are 256 threads; an LK
// block is four independent LK waves; the corner block runs one wave per pair.
using ofx_launch::kCornerScratch;
using ofx_launch::kPyrStages;
using ofx_launch::StreamArgs;

} // namespace
namespace ofx_launch { // shared by the translation units that instantiate the kernels (defined in lk_level.hip)
extern unsigned long long *g_stream_trace; // tools/stream_timeline.py
extern int g_stream_trace_blocks;
extern int g_trace_header[2 * OFX_STREAM_MAX_BATCH + 1];
} // namespace ofx_launch
namespace {
using ofx_launch::g_stream_trace;
using ofx_launch::g_stream_trace_blocks;
using ofx_launch::g_trace_header;

constexpr int kPyrPrio = 3; // priority of the marching-pyramid waves next to the LK waves (which go 3 -> 0 along their strips)
// DMA: the LK stage fetches its rows two steps ahead through LDS (lk_body_buf.h); chosen per launch (lk_plan.h: lk_tick_variant)
// WOUT: the LK stage's ITER (lk_plan.h): kIterSet, or kIterSetWarp / kIterSetWarpRows where it is iteration 1 of pairs that have more
// and also writes the warped images of their second iteration (~128 VGPRs: three blocks per CU at least)
// blocks per CU: lk_float fits 5 (<= 96 VGPRs) without scratch for every radius; compat_cpu needs ~120: 4 blocks (<= 128)
constexpr int stream_min_blocks(int mode, int wout)
{
    return wout ? 3 : (mode == OFX_MODE_LK_FLOAT ? 5 : 4);
}
template <int R, int MODE, bool FAST, bool DMA, int WOUT = 0>
__global__ __launch_bounds__(256, stream_min_blocks(MODE, WOUT)) void stream_kernel(const StreamArgs S)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const unsigned long long t_start = S.trace ? wall_clock64() : 0ull;
    // readfirstlane: the wave index is uniform, and everything derived from it (strip rows, row pointers, loop counters)
    // must live in SGPRs as it does in the stand-alone kernel
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (b < OFX_STREAM_MAX_BATCH) {
        // one corner chain per block (wave 0), so that the chains land on different CUs
        // the short latency-bound stages go first whenever they are ready to issue (the LK waves lower their own priority
        // from 3 to 0 as they advance, lk_body.h)
        __builtin_amdgcn_s_setprio(3);
        if (b < S.n_corner) {
            if (S.patch_build) patch_build_block(S.patch, S.patch_slot[b], tid); // (all 256 threads; ends with a barrier)
            // the chain (wave 0) with its repair (all four waves: corner_block; without relocated planes -- S.corner[b].reloc == NULL --
            // the other waves only keep the barriers company).  ONE inlined copy of the chain per kernel: with two (corner_wave
            // next to corner_block) hipcc 7.2 fails with "illegal VGPR to SGPR copy" in the LK branch's pinned scalars.
            corner_block<MODE, FAST>(S.corner[b], S.corner_lv + S.corner[b].lv0, S.patch, tid, wv, reinterpret_cast<float *>(lds), lds + kCornerScratch,
                                     reinterpret_cast<int *>(lds + kCornerScratch - 32));
        }
    } else if (b < S.first[0]) {
        lk_wave<R, MODE, false, false, FAST, DMA, WOUT>(S.lk, 4 * (b - OFX_STREAM_MAX_BATCH) + wv, tid & 63, lds + wv * (DMA ? kLkWaveLdsDma : kLkWaveLdsX));
    } else {
        int i = 0;
        while (i + 1 < kPyrStages && b >= S.first[i + 1]) ++i;
        __builtin_amdgcn_s_setprio(kPyrPrio);
        pyr_march_wave(S.pyr[i], 4 * (b - S.first[i]) + wv, tid & 63);
    }
    if (S.trace && b < S.trace_blocks && (tid & 63) == 0) { // one record per wave: 4 per block
        // where the wave ran: HW_ID (wave / SIMD / CU / SH / SE) in bits 32.., XCC_ID in bits 48.. of the start word's top
        const unsigned hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (15 << 11));  // HW_REG_HW_ID, bits 0..15
        const unsigned xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (3 << 11)); // HW_REG_XCC_ID, bits 0..3
        S.trace[2 * (4 * b + wv)] = t_start;
        S.trace[2 * (4 * b + wv) + 1] = (wall_clock64() & 0x0000ffffffffffffull) | ((unsigned long long)(hw & 0xffffu) << 48);
        S.trace[2 * (4 * b + wv)] = (t_start & 0x0000ffffffffffffull) | ((unsigned long long)(xcc & 0xfu) << 48);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
using ofx_launch::LkLevelIn;

// The launch's table: the items' LkArgs with the strips of the plan (lk_plan.h: lk_strips).  G: the tile's geometry (its OUT_W;
// TileGeom<R> or TileGeomP<R>).  Returns the wave count.
template <typename G>
int plan_table_g(const LkLevelIn *lv, int n, int min_h, int capacity, LkTable *out)
{
    ofx_plan::LkItem items[OFX_MAX_LK_ITEMS];
    for (int i = 0; i < n; ++i) items[i] = ofx_launch::lk_item(lv[i].a);
    ofx_plan::LkStrips s;
    ofx_plan::lk_strips(items, n, G::OUT_W, min_h, capacity, &s);
    LkTable t{};
    t.n = n;
    for (int i = 0; i < n; ++i) {
        t.lv[i] = lv[i].a;
        t.lv[i].tiles_x = s.tiles_x[i];
        t.lv[i].strip_h = s.strip_h[i];
        t.first_block[i] = s.first_block[i];
    }
    t.first_block[n] = s.blocks;
    *out = t;
    return s.blocks;
}

// What lk_wave_capacity (lk_plan.h) needs to know of the device: its CUs, and the waves of `kernel` a SIMD holds.  Asked once per
// kernel instantiation.
struct LkDevice {
    int cus, occ;
};
template <typename K>
LkDevice lk_device(K kernel, int threads, size_t lds)
{
    int dev = 0, cus = 256, per_cu = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess || per_cu <= 0) per_cu = 8 * 64 / threads;
    (void)hipGetLastError();
    return LkDevice{cus, per_cu * (threads / 64) / 4}; // (4 SIMDs per CU)
}

template <int R, int MODE, bool SUMS, bool FAST>
int launch_r(const LkLevelIn *lv, int n, hipStream_t st)
{
    static const LkDevice dev = lk_device(lk_level_kernel<R, MODE, SUMS, FAST>, 64, 0);
    const ofx_plan::LkSwitches sw = ofx_launch::lk_switches();
    LkTable t{};
    const int blocks = plan_table_g<TileGeom<R>>(lv, n, sw.min_strip, ofx_plan::lk_wave_capacity(dev.cus, dev.occ, 0, ofx_plan::kLkWavesPerSimd, ofx_plan::kLkFullFill, sw), &t);
    hipLaunchKernelGGL((lk_level_kernel<R, MODE, SUMS, FAST>), dim3((unsigned)blocks), dim3(64), 0, st, t);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

template <int R, int MODE, bool FAST, int ITER, bool DMA>
int launch_iter_r(const LkLevelIn *lv, int n, hipStream_t st)
{
    static const LkDevice dev = lk_device(lk_iter_kernel<R, MODE, FAST, ITER, DMA>, 64, 0);
    const ofx_plan::LkSwitches sw = ofx_launch::lk_switches();
    LkTable t{};
    const int blocks = plan_table_g<TileGeom<R>>(lv, n, sw.min_strip, ofx_plan::lk_wave_capacity(dev.cus, dev.occ, 0, ofx_plan::kLkWavesPerSimd, ofx_plan::kLkFullFill, sw), &t);
    hipLaunchKernelGGL((lk_iter_kernel<R, MODE, FAST, ITER, DMA>), dim3((unsigned)blocks), dim3(64), 0, st, t);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// two iterations per launch (a launch carries the work of two, so its strips are about twice as tall)
// opts (NULL: none): the caller's plan cache and switches.  With opts->pack the waves carry equal STEPS instead of one strip each
// (pair_plan.h); opts->waves > 0 sets the wave count of that plan.
template <int R, bool FAST, bool WOUT>
int launch_pair_r(const LkLevelIn *lv, int n, const ofx_pair_opts *opts, hipStream_t st)
{
    static const LkDevice dev = lk_device(lk_pair_kernel<R, FAST, WOUT>, 64, 0);
    const ofx_plan::LkSwitches sw = ofx_launch::lk_switches();
    const int capacity = ofx_plan::lk_wave_capacity(dev.cus, dev.occ, 0, ofx_plan::kPairWavesPerSimd, ofx_plan::kPairFullFill, sw);
    LkTable t{};
    int blocks = plan_table_g<TileGeomP<R>>(lv, n, sw.min_strip, capacity, &t);
    ofx_launch::PairPlanDev plan{nullptr, 0};
    if (opts && opts->pack && opts->cache) {
        const int want = opts->waves > 0 && opts->waves < capacity ? opts->waves : capacity;
        OFX_TRY(ofx_launch::pair_plan_get(opts->cache, R, TileGeomP<R>::OUT_W, lv, n, sw.min_strip, want, &plan));
        if (plan.segs) blocks = plan.waves;
    }
    hipLaunchKernelGGL((lk_pair_kernel<R, FAST, WOUT>), dim3((unsigned)blocks), dim3(64), 0, st, t, plan.segs);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// many: the tick carries two pairs or more (lk_plan.h: lk_tick_variant)
template <int R, int MODE, bool FAST, bool DMA, int WOUT>
int launch_stream_r(const LkLevelIn *lv, int n, bool many, StreamArgs &S, const int *stage_blocks, size_t lds, hipStream_t st)
{
    constexpr size_t wave_lds = DMA ? kLkWaveLdsDma : kLkWaveLdsX;
    static const LkDevice dev = lk_device(stream_kernel<R, MODE, FAST, DMA, WOUT>, 256, 4 * wave_lds);
    const ofx_plan::LkSwitches sw = ofx_launch::lk_switches();
    const int capacity = ofx_plan::lk_wave_capacity(dev.cus, dev.occ, ofx_plan::kTickReserve, ofx_plan::tick_waves_per_simd(many), ofx_plan::kLkFullFill, sw);
    int lk_blocks = 0;
    if (n > 0) lk_blocks = ofx_div_up(plan_table_g<TileGeom<R>>(lv, n, sw.min_strip, capacity, &S.lk), 4);
    S.first[0] = OFX_STREAM_MAX_BATCH + lk_blocks;
    for (int i = 0; i < kPyrStages; ++i) S.first[i + 1] = S.first[i] + stage_blocks[i];
    const int blocks = S.first[kPyrStages];
    S.trace = g_stream_trace;
    S.trace_blocks = g_stream_trace_blocks;
    if (g_stream_trace) // header: block ranges of this launch
        for (int i = 0; i <= kPyrStages; ++i) g_trace_header[i] = S.first[i];
    size_t corner_lds = 0; // a corner wave's scratch: the chain's floats and the cached corners of its levels
    for (int i = 0; i < S.n_corner; ++i) {
        const size_t need = (size_t)kCornerScratch + kCornerTileBytes + (size_t)S.corner[i].levels * kCornerCacheBytes;
        corner_lds = need > corner_lds ? need : corner_lds;
    }
    if (lds < corner_lds) lds = corner_lds;
    if (lds < 4 * wave_lds) lds = 4 * wave_lds; // an LK block: four waves, each with its exchange row (and its fetched rows)
    hipLaunchKernelGGL((stream_kernel<R, MODE, FAST, DMA, WOUT>), dim3((unsigned)blocks), dim3(256), lds, st, S);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
}

// Calls f(std::integral_constant<int, R>{}) for R = radius when 1 <= radius <= MAX_R (which instantiates f for every such R);
// false: the radius is outside that range and f was not called.
template <int MAX_R, int R = 1, typename F>
bool dispatch_radius(int radius, F &&f)
{
    if constexpr (R <= MAX_R) {
        if (radius == R) {
            f(std::integral_constant<int, R>{});
            return true;
        }
        return dispatch_radius<MAX_R, R + 1>(radius, f);
    } else {
        return false;
    }
}
using ofx_plan::lk_max_radius;

} // namespace

// The families: lk_level.hip calls them, and each lk_inst_*.hip instantiates one explicitly (lk_inst.h holds the definitions), so
// that the families compile in parallel.  The kernels stay internal to the unit that instantiates them.
namespace ofx_launch {
// all levels of a fused launch (sums: the inspection variant, which does not depend on the solve: FAST = false only)
template <int MODE, bool FAST>
int levels(int radius, const LkLevelIn *lv, int n, bool sums, hipStream_t st);
// refinement iterations on the buffer march (ITER: lk_plan.h, kIterAdd .. kIterAddWarpRows); deep: with the deep fetch
template <int MODE, bool FAST, int ITER>
int iter(int radius, const LkLevelIn *lv, int n, bool deep, hipStream_t st);
// two refinement iterations per launch (lk_body_pair.h; radii 1..kLkPairMaxR, lk_float solves, whole levels): lv[i].a.flow_in is
// the flow set read, .flow the one written; WOUT: the launch also writes the warped images of the iteration after its second
template <bool FAST, bool WOUT>
int iter_pair(int radius, const LkLevelIn *lv, int n, const ofx_pair_opts *opts, hipStream_t st);
// one stream tick (WOUT, deep, many: lk_plan.h, lk_tick_variant; no deep fetch with WOUT)
template <int MODE, bool FAST, int WOUT = ofx_plan::kIterSet>
int stream(int radius, const LkLevelIn *lv, int n, bool deep, bool many, StreamArgs &S, const int *stage_blocks, size_t lds, hipStream_t st);
} // namespace ofx_launch
