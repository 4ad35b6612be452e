// Two refinement iterations of lk_iter in ONE march: a wave carries march A = iteration j and march B =
// iteration j + 1 on the same lane-to-column mapping, B trailing A by LAG = R + 2 output rows inside the same step body.  What
// iteration j + 1 reads of iteration j -- its flow (16 B/px there and back) and the warped image it made (2 B/px) -- never goes to
// memory.  Included by lk_body.h after lk_body_buf.h, whose pieces (resources, kOob rows, the exchanged stores) it uses.
//
//   * A is the accumulating march of ITER = 2 without its stores: old flow from the flow set the launch READS (LkArgs::flow_in),
//     rows of prev and of the warped image of iteration j - 1 through their resources, the warp of lk_body_warp.h in its two
//     stages.  The finished warped row goes into a per-wave LDS ring (kPairWarpRows rows of 256 B; columns outside the image as
//     zeros, which is what the resource's range check and the column mask give a march that reads the image from memory), the
//     row's new flow into a second ring (LAG + 1 rows of 2 KB: a lane's own 4 pixels, read back by the same lane).
//   * B is the accumulating march of ITER = 1 / 2 with `next` taken from the warped ring and the old flow from the flow ring; it
//     reads prev again through the resource (cache hits: A fetched the rows a few steps earlier), stores its flow through the
//     exchange and the streaming stores into the flow set the launch WRITES (LkArgs::flow), and -- WOUT -- the warped image of
//     iteration j + 2 as ITER = 2 does.  A's overlap rows and columns read flow of iteration j - 1 at pixels whose owner's B may
//     already have stored iteration j + 1: hence the two flow sets.
//   * Geometry: B's output lanes are A's minus R + 1 columns either side (TileGeomP), B's strip is [ysB, yeB), A's is
//     [ysB - R - 1, min(yeB + R + 1, h)).  A always starts R + 1 rows above B's strip, also where those rows lie above the image
//     (they read as zeros and their results are never looked at): the step lag between the marches is then the constant
//     kLagSteps = 2R + 3 for every wave, B's register slots rotate on a compile-time index, and every strip of a height takes the
//     same number of steps.
//   * A's step t leaves warped rows up to ysB + t - (2R + 3) in the ring; B's step t - kLagSteps takes exactly that row as the
//     bottom row of its entering window, so B takes its rows at the START of its step (after A's part of the same step), not a
//     step ahead as the marches that read memory do.  LDS operations of a wave execute in order and the rings are private to it.
//   * B does not compute 1 / det again (OFX_PAIR_SHARE_RCP).  det = a d - b b of the 2x2 solve is made of the three window sums of
//     prev's derivatives alone, and B's three sums at a pixel are the very integers A had there: the same lane and column mask,
//     the same row masks (both marches clip the window to the image, and a strip's own limits lie outside every window of a row
//     it emits), sliding sums that are exact in int.  So det and the reciprocal the solve takes of it (lk_solve.h) are identical
//     bit for bit, det == 0 with its +-Inf / NaN included, and no tolerance is involved.  A's emitting step t makes output row
//     ysB - 2R - 2 + t, B's step t - kLagSteps makes ysB - 3R - 4 + t: B is R + 2 joint steps behind on a row, for every wave.
//     The four doubles of a lane's row travel that long in registers: slots that rotate with the three-fold body (written at
//     step t, read or moved on at t + 3 in the same k) give a delay of 3 per slot, a shift chain of (R + 2) % 3 stages the rest:
//     9x9 two slots, 7x7 one slot and two stages, 5x5 one and one, 3x3 one slot; 8 (R + 2) registers, and at 9x9 8 v_mov_b64
//     per step (B uses its value after A's solve of the same step: three values per k are alive, each double moves twice).  Only the reciprocal: the sums or the scaled matrix as well would be 24 - 36 more registers per row
//     of lag.
// Whole levels only (row0 = 0, all rows), no global shift (the shifted image was made before the tick), lk_float solves, R <= 4:
// the host checks (lk_level.hip).  The arithmetic and its order are those of lk_wave_buf: results are bit-identical.
#pragma once

namespace ofx_dev {

template <int R>
struct TileGeomP { // a wave tile of the fused pair: B's output lanes
    // A's results are exact from wave column R + 1 on (derivatives from column 1; hbox4x5's sliding differences are integer, so a
    // lane's columns are each exact or not on their own, also in lanes below TileGeom<R>::LO_LANE), and B's outputs need them R + 1
    // columns either side: B's first exact column is 2R + 2, its last 253 - 2R.  The inset is rounded to whole lanes ONCE.
    static constexpr int FIRST_COL = 2 * R + 2;
    static constexpr int LO_LANE = (FIRST_COL + 3) / 4;
    static constexpr int HI_LANE = 63 - LO_LANE;
    static constexpr int OUT_W = (HI_LANE - LO_LANE + 1) * 4;
    static_assert(4 * LO_LANE >= FIRST_COL && 4 * HI_LANE + 3 <= 253 - 2 * R, "B's output columns have all of A's results they need");
};
static_assert(TileGeomP<4>::LO_LANE == 3 && TileGeomP<4>::HI_LANE == 60 && TileGeomP<4>::OUT_W == 232, "9x9: lanes 3..60");
static_assert(TileGeomP<3>::LO_LANE == 2 && TileGeomP<3>::HI_LANE == 61 && TileGeomP<3>::OUT_W == 240, "7x7: lanes 2..61");
static_assert(TileGeomP<2>::LO_LANE == 2 && TileGeomP<2>::HI_LANE == 61 && TileGeomP<2>::OUT_W == 240, "5x5: lanes 2..61");
static_assert(TileGeomP<1>::LO_LANE == 1 && TileGeomP<1>::HI_LANE == 62 && TileGeomP<1>::OUT_W == 248, "3x3: lanes 1..62");

#ifndef OFX_PAIR_SHARE_RCP
#define OFX_PAIR_SHARE_RCP 1 // march B takes 1 / det from march A (above); 0: both compute it, as two launches would
#endif
// per instance, should one not fit its registers (profiles/pair_rcp_budget.txt: all sixteen do)
constexpr bool pair_share_rcp(int r, bool fast) { return OFX_PAIR_SHARE_RCP != 0; }

// A comment in the listing, no instruction: marks the paths of the joint step that a segment takes a bounded number of times (its
// priming, B's start, A's drain: 3R + 4 steps however many rows it has).  tools/isa_waits.py leaves paths through a marked block out
// when it measures how long the warp's tap loads stay in flight on the steps in between, where both marches emit.
#define OFX_COLD_PATH() asm volatile("; ofx-cold")

constexpr int kLkPairMaxR = 4;
constexpr int pair_warp_rows(int r) { return 2 * r + 4; } // rows [yyB - 2R, yyB + 1] are live in a step: 2R + 2, and slack
constexpr int pair_flow_rows(int r) { return r + 3; }     // LAG + 1
constexpr int pair_wave_lds(int r) { return kLkWaveLds + 256 * pair_warp_rows(r) + 2048 * pair_flow_rows(r); }
static_assert(pair_wave_lds(4) == 19584 && 8 * pair_wave_lds(4) <= 160 * 1024, "two waves per SIMD at 9x9");

constexpr int pair_seg_steps(int r) { return 3 * r + 4; } // what a segment of a wave costs beyond its rows: priming and lag

// One segment of a wave: rows [ysB, yeB) of tile column `tile` of item `level`.  Everything a segment needs is set up here, so a wave
// may march several, one after the other (lk_pair_kernel).  q1..q3: the steps of THIS march at which the wave's priority drops, i.e.
// the quarter points of the wave's whole work less the steps of its earlier segments.
template <int R, bool FAST, bool INTERIOR, bool WOUT>
__device__ __forceinline__ void lk_wave_pair(const LkTable &T, int level, int tile, int ysB, int yeB, int lane, uint8_t *xlds, int q1, int q2, int q3)
{
    constexpr int MODE = OFX_MODE_LK_FLOAT;
    using G = TileGeomP<R>;
    constexpr int NS = 2 * R + 1, H = R - 1, PR = 2 * R - H;
    constexpr int kLagSteps = 2 * R + 3;
    constexpr int WN = pair_warp_rows(R), FN = pair_flow_rows(R);
    static_assert(PR + kLagSteps == pair_seg_steps(R), "a segment of r rows takes r + 3R + 4 steps");
    // A's reciprocals on their way to B, R + 2 steps: QD slots per k = t mod 3 (rq[0]: the younger), then QE chain stages.
    // A segment primes its own line: B's first emitting step, 3R + 4, takes what A's step 2R + 2 >= PR of THIS segment put in (9x9:
    // 16 and 10); what the line holds before that -- nothing, or an earlier segment's values -- moves through it and is never used.
    constexpr bool SHARE = pair_share_rcp(R, FAST);
    constexpr int QD = (R + 2) / 3, QE = (R + 2) % 3;
    static_assert(QD >= 1 && 3 * QD + QE == kLagSteps - (R + 1), "the delay is B's lag behind A on an output row");
    [[maybe_unused]] double rq[QD][3][4], rc[QE > 0 ? QE : 1][4];
    if constexpr (SHARE) { // (volatile: equal asm statements would be merged into one value and copied out of it)
#pragma unroll
        for (int i = 0; i < QD * 3; ++i) asm volatile("" : "=v"(rq[i / 3][i % 3][0]), "=v"(rq[i / 3][i % 3][1]), "=v"(rq[i / 3][i % 3][2]), "=v"(rq[i / 3][i % 3][3]));
#pragma unroll
        for (int i = 0; i < QE; ++i) asm volatile("" : "=v"(rc[i][0]), "=v"(rc[i][1]), "=v"(rc[i][2]), "=v"(rc[i][3]));
    }

    LkArgs A = T.lv[level];
    pin_scalar(A.w);
    pin_scalar(A.h);
    pin_scalar(A.pitch);
    pin_scalar(A.min_det);
    pin_scalar(A.warp_scale);
    const SolveOpts sopt{A.min_det};
    const int cb = tile * G::OUT_W - G::LO_LANE * 4 + 4 * lane; // first of this lane's 4 image columns
    const int ysA = ysB - (R + 1), yeA = min(yeB + R + 1, A.h);

    const int plane_bytes = A.h * A.pitch;
    const __amdgpu_buffer_rsrc_t rs_prev = make_rsrc(A.prev, plane_bytes), rs_next = make_rsrc(A.next, plane_bytes);
    const __amdgpu_buffer_rsrc_t rs_fin = make_rsrc(A.flow_in, A.h * A.w * 8), rs_flow = make_rsrc(A.flow, A.h * A.w * 8);
    const __amdgpu_buffer_rsrc_t rs_wsrc = make_rsrc(A.warp_src, plane_bytes + 3); // (lk_body_warp.h)
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rs_wout = rs_prev;
    if constexpr (WOUT) rs_wout = make_rsrc(A.warp_out, plane_bytes);

    // ---- the lanes' columns: shared by both marches (lk_wave_buf)
    const bool ld_ok = INTERIOR || (cb >= 0 && cb < A.w);
    uint32_t bmask = INTERIOR ? 0xffffffffu : 0u;
    if constexpr (!INTERIOR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = (cb + j) >= 0 && (cb + j) < A.w;
            bmask |= in ? (0xffu << (8 * j)) : 0u;
        }
    }
    uint32_t col_off = ld_ok ? (uint32_t)cb : 0u;
    uint32_t nat_off = (uint32_t)cb * 8u;
    auto finish_row = [&](uint32_t raw) -> uint32_t {
        if constexpr (INTERIOR) return raw;
        else return raw & bmask;
    };
    // B's stores: the exchanged layout of an output row
    const int x0 = tile * G::OUT_W;
    const int nv = min(x0 + G::OUT_W, A.w) - x0;
    uint32_t l16 = 16u * (uint32_t)lane;
    const int lim = 8 * nv - 16, c16 = 16 * lane;
    const bool st_lo4 = c16 <= lim, st_lo2 = c16 == lim + 8, st_hi4 = c16 <= lim - 1024, st_hi2 = c16 == lim + 8 - 1024;
    const uint32_t vo_lo = st_lo4 ? l16 : (uint32_t)kOob, vo_hi = st_hi4 ? l16 + 1024u : (uint32_t)kOob;
    const bool ragged = __any(st_lo2 || st_hi2) != 0;
    const lds_ptr xl_w = (lds_ptr)xlds + 32 * lane;
    const lds_ptr xl_base = (lds_ptr)xlds + 32 * G::LO_LANE;
    // the rings
    const lds_ptr wring = (lds_ptr)xlds + kLkWaveLds + 4 * lane;          // this lane's dword of warped ring row 0
    const lds_ptr fring = (lds_ptr)xlds + kLkWaveLds + 256 * WN + 32 * lane; // this lane's 32 bytes of flow ring row 0
    // (rows from -(R + 2) on are looked up; the slot of a row is wave-uniform)
    auto wslot = [&](int y) -> int { return __builtin_amdgcn_readfirstlane((int)((uint32_t)(y + 2 * WN) % (uint32_t)WN) * 256); };
    auto fslot = [&](int y) -> int { return __builtin_amdgcn_readfirstlane((int)((uint32_t)(y + 4 * FN) % (uint32_t)FN) * 2048); };
    // B's warp output
    [[maybe_unused]] uint32_t wvo = (uint32_t)kOob;
    if constexpr (WOUT) {
        const bool out_lane = lane >= G::LO_LANE && lane <= G::HI_LANE && cb < A.w;
        wvo = out_lane ? (uint32_t)cb : (uint32_t)kOob;
    }
    uint32_t wmiss = 0u;
    WarpRowState WA;
    [[maybe_unused]] WarpRowState WB;
    warp_row_clear(WA);
    if constexpr (WOUT) warp_row_clear(WB);
    const s2 two = pk_two();
    const int fstep = A.w * 8;

    // ---- march A: rows of a strip [ysA, yeA) (ysA may lie above the image)
    const int y_limA = min(yeA + R + 1, A.h);
    const int y_firstA = ysA - R, y_lo0A = y_firstA + H;
    const int nstepsA = (yeA - ysA) + PR;
    const int y_min_outA = max(0, y_firstA - 1), span_outA = max(y_limA - y_min_outA, 0);
    auto row_offA = [&](int y) -> int { return (uint32_t)y < (uint32_t)y_limA ? y * A.pitch : kOob; };
    auto row_off_outA = [&](int y) -> int { return (uint32_t)(y - y_min_outA) < (uint32_t)span_outA ? y * A.pitch : kOob; };
    auto load_u32 = [&](const __amdgpu_buffer_rsrc_t &rs, int po) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(rs, col_off, po, 0); };
    RowPk<MODE> wa[3];
    {
        uint32_t pi, ni, po = 0u, no = 0u;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int oi = row_offA(y_lo0A - 1 + t);
            pi = finish_row(load_u32(rs_prev, oi)), ni = finish_row(load_u32(rs_next, oi));
            if constexpr (H > 0) {
                const int oo = row_off_outA(y_firstA - 1 + t);
                po = finish_row(load_u32(rs_prev, oo)), no = finish_row(load_u32(rs_next, oo));
            }
            unpack_pk(pi, ni, po, no, wa[t]);
        }
    }
    int axx[4] = {0, 0, 0, 0}, ayy[4] = {0, 0, 0, 0}, axy[4] = {0, 0, 0, 0}, axt[4] = {0, 0, 0, 0}, ayt[4] = {0, 0, 0, 0};

    // Loaded values that a path must have waited for before it reaches a join (no instruction but the s_waitcnt the compiler puts
    // in front).  Loads complete in order and the compiler counts them per path, but where paths join it keeps the worst count
    // of a register: a value one path still has in flight as its YOUNGEST load costs vmcnt(0) behind the join on every path,
    // also on the one that has just issued the warp's taps.  Only the cold paths have such values.
    auto landed = [](uint32_t &a, uint32_t &b) { asm volatile("; ofx-cold" : "+v"(a), "+v"(b)); };
    auto landed4 = [](uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) { asm volatile("; ofx-cold" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); };
    // a step of A that emits nothing leaves its slot of the line undefined (no copy to keep what it held)
    auto no_rcp = [](double (&q)[4]) {
        if constexpr (SHARE) asm("" : "=v"(q[0]), "=v"(q[1]), "=v"(q[2]), "=v"(q[3])); // (ONE asm: four alike are merged, then copied)
    };
    // the warped row the step before prepared, into the ring (columns outside the image: zeros)
    auto ring_warped = [&](int y) {
        const uint32_t wn = finish_row(warp_row_finish(WA));
        *(__attribute__((address_space(3))) uint32_t *)(wring + wslot(y)) = wn;
    };
    auto stepA = [&](auto K, int s) {
        constexpr int k = decltype(K)::value; // s mod 3
        const int yy = y_lo0A + s, yo = yy - NS;
        const bool folded = H > 0 && s < H;
        const int yh = folded ? y_firstA + s : yo;
        const int ro = (H > 1 && s + 1 < H) ? y_firstA + s + 2 : yo + 2;
        const int po_in = row_offA(yy + 2), po_out = row_off_outA(ro);
        uint32_t pf_ip = load_u32(rs_prev, po_in), pf_in = load_u32(rs_next, po_in);
        uint32_t pf_op = load_u32(rs_prev, po_out), pf_on = load_u32(rs_next, po_out);
        const bool emit = s >= PR;
        const int yw = yy - R; // this step's output row
        f32x4 old_a, old_b;
        asm("" : "=v"(old_a), "=v"(old_b));
        if (emit) {
            const int fnat = __builtin_amdgcn_readfirstlane(yw >= 0 ? yw * fstep : kOob); // (rows above the image: nothing is read)
            if constexpr (INTERIOR) {
                old_a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_fin, nat_off, fnat, 0));
                old_b = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_fin, nat_off + 16u, fnat, 0));
            } else {
                auto off = [&](int j) { return ((bmask >> (8 * j)) & 1u) ? nat_off + 8u * (uint32_t)j : (uint32_t)kOob; };
                const u32x2 p0 = __builtin_amdgcn_raw_buffer_load_b64(rs_fin, off(0), fnat, 0), p1 = __builtin_amdgcn_raw_buffer_load_b64(rs_fin, off(1), fnat, 0);
                const u32x2 p2 = __builtin_amdgcn_raw_buffer_load_b64(rs_fin, off(2), fnat, 0), p3 = __builtin_amdgcn_raw_buffer_load_b64(rs_fin, off(3), fnat, 0);
                old_a = __builtin_bit_cast(f32x4, u32x4{p0.x, p0.y, p1.x, p1.y});
                old_b = __builtin_bit_cast(f32x4, u32x4{p2.x, p2.y, p3.x, p3.y});
            }
        }
        const uint32_t him = folded ? 0x00010000u : (yo >= y_firstA ? 0xffff0000u : 0u);
        uint32_t rowm = ((uint32_t)yy < (uint32_t)A.h ? 0x00000001u : 0u) | ((uint32_t)yh < (uint32_t)A.h ? him : 0u);
        if constexpr (INTERIOR) rowm = (uint32_t)__builtin_amdgcn_readfirstlane((int)rowm);
        uint32_t mm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) mm[j] = INTERIOR ? rowm : ((uint32_t)__builtin_amdgcn_sbfe((int)bmask, 8 * j, 1) & rowm);
        s2 ix[4], iy[4], it[4];
        derivs_pk(wa[k], wa[(k + 1) % 3], wa[(k + 2) % 3], two, ix, iy, it);
        accumulate_pk(ix, iy, it, mm, axx, ayy, axy, axt, ayt);
        if (emit) {
            float uv[8];
            int hb[5][4];
            {
                int va[5][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) va[0][j] = axx[j], va[1][j] = ayy[j], va[2][j] = axy[j], va[3][j] = axt[j], va[4][j] = ayt[j];
                hbox4x5<R>(va, hb);
            }
            if constexpr (SHARE) solve_lane_rcp_out<MODE, FAST>(hb[0], hb[1], hb[2], hb[3], hb[4], sopt, rq[0][k], uv);
            else solve_lane<MODE, FAST>(hb[0], hb[1], hb[2], hb[3], hb[4], sopt, uv);
            uv[0] = old_a.x + uv[0], uv[1] = old_a.y + uv[1], uv[2] = old_a.z + uv[2], uv[3] = old_a.w + uv[3];
            uv[4] = old_b.x + uv[4], uv[5] = old_b.y + uv[5], uv[6] = old_b.z + uv[6], uv[7] = old_b.w + uv[7];
            // the warped row of the step before: second stage, into the ring (the first emitting step has none pending: its row
            // is one B never takes); then this row's first stage, and its flow into the flow ring
            ring_warped(yw - 1);
            const float fu[4] = {uv[0], uv[2], uv[4], uv[6]}, fv[4] = {uv[1], uv[3], uv[5], uv[7]};
            warp_row_prepare<false>(rs_wsrc, A.warp_scale, A.w, A.h, A.pitch, 0, A.h, cb, yw, 4, fu, fv, WA, wmiss);
            const lds_ptr fr = fring + fslot(yw);
            *(__attribute__((address_space(3))) f32x4 *)(fr) = f32x4{uv[0], uv[1], uv[2], uv[3]};
            *(__attribute__((address_space(3))) f32x4 *)(fr + 16) = f32x4{uv[4], uv[5], uv[6], uv[7]};
        } else {
            no_rcp(rq[0][k]);
            // The step's rows are unpacked behind the join.  On the emitting path they are older than the old flow, which has
            // been waited for; on this one they are the youngest loads, and left to the join the compiler waits there for the
            // worse of the two -- which drained the taps eleven instructions after their issue (profiles/warp_taps_isa.txt).
            // So this path waits for its rows itself.
            landed4(pf_ip, pf_in, pf_op, pf_on);
        }
        unpack_pk(finish_row(pf_ip), finish_row(pf_in), finish_row(pf_op), finish_row(pf_on), wa[k]);
        pin_row(wa[k]);
    };

    // ---- march B: strip [ysB, yeB)
    const int y_limB = min(yeB + R + 1, A.h); // (== yeA: A has made every warped row B takes)
    const int y_firstB = ysB - R, y_lo0B = y_firstB + H;
    const int nstepsB = (yeB - ysB) + PR;
    const int y_min_outB = max(0, y_firstB - 1), span_outB = max(y_limB - y_min_outB, 0);
    auto row_offB = [&](int y) -> int { return (uint32_t)y < (uint32_t)y_limB ? y * A.pitch : kOob; };
    auto row_off_outB = [&](int y) -> int { return (uint32_t)(y - y_min_outB) < (uint32_t)span_outB ? y * A.pitch : kOob; };
    // row y of the warped image out of the ring: zeros where a march on memory reads none (po: row_offB / row_off_outB of y)
    auto ring_row = [&](int y, int po) -> uint32_t {
        uint32_t v = 0u;
        if (po != kOob) v = *(const __attribute__((address_space(3))) uint32_t *)(wring + wslot(y));
        return v;
    };
    RowPk<MODE> wb[3];
    // B's rows of prev for the next step, in flight.  B takes them at the top of its part, behind the join of A's paths.  Where A
    // emitted, they are older than loads A has waited for; the two paths on which they are not (A finished, B's priming) wait for
    // them inside the path (`landed`).
    uint32_t pfb_i = 0u, pfb_o = 0u;
    int bxx[4] = {0, 0, 0, 0}, byy[4] = {0, 0, 0, 0}, bxy[4] = {0, 0, 0, 0}, bxt[4] = {0, 0, 0, 0}, byt[4] = {0, 0, 0, 0};
    const int fso0 = __builtin_amdgcn_readfirstlane((ysB * A.w + x0) * 8);
    // the high stream's bottom row of step s (lk_wave_buf fetches it a step earlier: `ro`, and the third priming row)
    auto high_rowB = [&](int s) -> int { return (H > 0 && (s == 0 || s < H)) ? y_firstB + s + 1 : y_lo0B + s - NS + 1; };
    auto primeB = [&]() {
        OFX_COLD_PATH();
        uint32_t pi, ni, po = 0u, no = 0u;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int yi = y_lo0B - 1 + t, oi = row_offB(yi);
            pi = finish_row(load_u32(rs_prev, oi)), ni = ring_row(yi, oi);
            if constexpr (H > 0) {
                const int yo = y_firstB - 1 + t, oo = row_off_outB(yo);
                po = finish_row(load_u32(rs_prev, oo)), no = ring_row(yo, oo);
            }
            unpack_pk(pi, ni, po, no, wb[t]);
        }
        pfb_i = load_u32(rs_prev, row_offB(y_lo0B + 1));
        pfb_o = load_u32(rs_prev, H > 0 ? row_off_outB(high_rowB(0)) : kOob);
        landed(pfb_i, pfb_o); // (step 0 takes them at once; once per segment)
    };
    auto store_row = [&](int s_row, const f32x4 xlo, const f32x4 xhi) {
        const int fso = __builtin_amdgcn_readfirstlane(fso0 + (s_row - PR) * fstep);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, xlo), rs_flow, INTERIOR ? lane_off_var(l16) : vo_lo, fso, kLkStoreAux);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, xhi), rs_flow, vo_hi, fso, kLkStoreAux);
        if (__builtin_expect(ragged, 0)) {
            const u32x4 ql = __builtin_bit_cast(u32x4, xlo), qh = __builtin_bit_cast(u32x4, xhi);
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{ql.x, ql.y}, rs_flow, st_lo2 ? l16 : (uint32_t)kOob, fso, kLkStoreAux);
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{qh.x, qh.y}, rs_flow, st_hi2 ? l16 + 1024u : (uint32_t)kOob, fso, kLkStoreAux);
        }
    };
    auto stepB = [&](auto K, int s, [[maybe_unused]] const double (&rcp)[4]) {
        constexpr int k = decltype(K)::value; // s mod 3
        const int yy = y_lo0B + s, yo = yy - NS;
        const bool folded = H > 0 && s < H;
        const int yh = folded ? y_firstB + s : yo;
        // this step's bottom rows: prev has arrived, the warped rows are in the ring (A's part of this step made yy + 1)
        {
            const int rh = high_rowB(s);
            const int oi = row_offB(yy + 1), oo = (H > 0 || s > 0) ? row_off_outB(rh) : kOob;
            unpack_pk(finish_row(pfb_i), ring_row(yy + 1, oi), finish_row(pfb_o), ring_row(rh, oo), wb[(k + 2) % 3]);
            pin_row(wb[(k + 2) % 3]);
            pfb_i = load_u32(rs_prev, row_offB(yy + 2));
            pfb_o = load_u32(rs_prev, row_off_outB(high_rowB(s + 1)));
        }
        const bool emit = s >= PR;
        const int yw = yy - R;
        f32x4 old_a, old_b;
        asm("" : "=v"(old_a), "=v"(old_b));
        if (emit) {
            const lds_ptr fr = fring + fslot(yw);
            old_a = *(const __attribute__((address_space(3))) f32x4 *)(fr);
            old_b = *(const __attribute__((address_space(3))) f32x4 *)(fr + 16);
        }
        const uint32_t him = folded ? 0x00010000u : (yo >= y_firstB ? 0xffff0000u : 0u);
        uint32_t rowm = ((uint32_t)yy < (uint32_t)A.h ? 0x00000001u : 0u) | ((uint32_t)yh < (uint32_t)A.h ? him : 0u);
        if constexpr (INTERIOR) rowm = (uint32_t)__builtin_amdgcn_readfirstlane((int)rowm);
        uint32_t mm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) mm[j] = INTERIOR ? rowm : ((uint32_t)__builtin_amdgcn_sbfe((int)bmask, 8 * j, 1) & rowm);
        s2 ix[4], iy[4], it[4];
        derivs_pk(wb[k], wb[(k + 1) % 3], wb[(k + 2) % 3], two, ix, iy, it);
        accumulate_pk(ix, iy, it, mm, bxx, byy, bxy, bxt, byt);
        if (emit) {
            float uv[8];
            int hb[5][4];
            {
                int va[5][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) va[0][j] = bxx[j], va[1][j] = byy[j], va[2][j] = bxy[j], va[3][j] = bxt[j], va[4][j] = byt[j];
                hbox4x5<R>(va, hb);
            }
            if constexpr (SHARE) solve_lane_rcp_in<MODE, FAST>(hb[0], hb[1], hb[2], hb[3], hb[4], sopt, rcp, uv);
            else solve_lane<MODE, FAST>(hb[0], hb[1], hb[2], hb[3], hb[4], sopt, uv);
            uv[0] = old_a.x + uv[0], uv[1] = old_a.y + uv[1], uv[2] = old_a.z + uv[2], uv[3] = old_a.w + uv[3];
            uv[4] = old_b.x + uv[4], uv[5] = old_b.y + uv[5], uv[6] = old_b.z + uv[6], uv[7] = old_b.w + uv[7];
            if constexpr (WOUT) { // the warped image of iteration j + 2, as ITER = 2 writes it (lk_wave_buf)
                const uint32_t wn = warp_row_finish(WB);
                const int wso = __builtin_amdgcn_readfirstlane(s > PR ? (yw - 1) * A.pitch : kOob);
                __builtin_amdgcn_raw_buffer_store_b32(wn, rs_wout, wvo, wso, 0);
                const float fu[4] = {uv[0], uv[2], uv[4], uv[6]}, fv[4] = {uv[1], uv[3], uv[5], uv[7]};
                warp_row_prepare<false>(rs_wsrc, A.warp_scale, A.w, A.h, A.pitch, 0, A.h, cb, yw, 4, fu, fv, WB, wmiss);
            }
            *(__attribute__((address_space(3))) f32x4 *)(xl_w) = f32x4{uv[0], uv[1], uv[2], uv[3]};
            *(__attribute__((address_space(3))) f32x4 *)(xl_w + 16) = f32x4{uv[4], uv[5], uv[6], uv[7]};
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const lds_ptr xl_r = xl_base + lane_off_var(l16);
            const f32x4 xlo = *(__attribute__((address_space(3))) f32x4 *)(xl_r);
            const f32x4 xhi = *(__attribute__((address_space(3))) f32x4 *)(xl_r + 1024);
            store_row(s, xlo, xhi);
        } else OFX_COLD_PATH();
    };

    // ---- the joint march: step t is A's step t and B's step t - kLagSteps
    const int nsteps = nstepsB + kLagSteps; // (>= nstepsA + 1: A's last warped row is finished in the step after its last)
    auto body = [&](auto K, int t) {
        constexpr int k = decltype(K)::value;                    // t mod 3
        constexpr int kb = (k + 3 - kLagSteps % 3) % 3;          // (t - kLagSteps) mod 3
        // what A made R + 2 steps ago comes out of the line BEFORE A's part of this step writes slot k again
        [[maybe_unused]] double rcpB[4];
        if constexpr (SHARE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double out = rq[QD - 1][k][j];
                rcpB[j] = QE > 0 ? rc[QE > 0 ? QE - 1 : 0][j] : out;
#pragma unroll
                for (int i = QE - 1; i > 0; --i) rc[i][j] = rc[i - 1][j];
                if constexpr (QE > 0) rc[0][j] = out;
#pragma unroll
                for (int i = QD - 1; i > 0; --i) rq[i][k][j] = rq[i - 1][k][j];
            }
        }
        if (t < nstepsA) stepA(K, t);
        else {
            OFX_COLD_PATH();
            if (t == nstepsA) ring_warped(yeA - 1);
            no_rcp(rq[0][k]);
            landed(pfb_i, pfb_o); // (on this path B's rows are not behind a wait of A's yet)
        }
        if (t >= kLagSteps) {
            // (what A has just put into the rings is read by other lanes: LDS operations of a wave execute in order)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if constexpr (kb == 0) {
                if (t == kLagSteps) primeB();
            }
            stepB(std::integral_constant<int, kb>{}, t - kLagSteps, rcpB);
        } else OFX_COLD_PATH();
    };
    int s = 0;
    while (true) {
        body(std::integral_constant<int, 0>{}, s);
        if (++s >= nsteps) break;
        body(std::integral_constant<int, 1>{}, s);
        if (++s >= nsteps) break;
        body(std::integral_constant<int, 2>{}, s);
        if (++s >= nsteps) break;
        OFX_LK_PRIO_STEP();
    }
    if constexpr (WOUT) { // the warped row of B's last step
        const uint32_t wn = warp_row_finish(WB);
        __builtin_amdgcn_raw_buffer_store_b32(wn, rs_wout, wvo, (yeB - 1) * A.pitch, 0);
    }
}

} // namespace ofx_dev
