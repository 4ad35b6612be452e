// The plan of a fused two-iteration launch (lk_body_pair.h): which rows of which tile column every wave
// marches.  Plain host code without HIP in it, so that tests/test_pair_plan.py compiles it into a stand-alone program.
//
// A launch runs in ONE residency round of `capacity` waves and lasts as long as its longest wave, so the plan equalises the waves'
// STEPS, not their rows.  A wave carries up to kPairMaxSegs segments; a segment is rows [y0, y1) of one tile column of one item
// -- what a strip is to plan_table_g -- and costs (y1 - y0) + overhead steps (overhead = 3R + 4: the priming of both marches and the
// lag between them, paid by every segment).  The tile columns of all items, in order, are laid end to end and cut into waves of at
// most S steps; S is the smallest budget with which `capacity` waves are enough.
#pragma once

#include <vector>

namespace ofx_plan {

constexpr int kPairMaxSegs = 2; // segments a wave carries at most

struct PairSeg { // rows [y0, y1) of tile column `tile` of item `item`; y1 <= y0: none (16 bytes: the kernel reads it as one int4)
    int item, tile, y0, y1;
};
struct PairItem { // a (pair, level) item: its level's size
    int w, h;
};
struct PairPlan {
    int waves = 0, segments = 0;
    int S = 0;                 // steps of the longest wave
    std::vector<PairSeg> segs; // waves x kPairMaxSegs
};

// The greedy fill for one step budget S.  A cut leaves no piece shorter than min_h on either side of it (a column shorter than that
// stays whole): where the rest of a wave's budget holds less, the wave closes early.  false: S is too small for some column, or
// more than `capacity` waves are needed.
inline bool pair_plan_fill(const PairItem *items, int n, int out_w, int overhead, int min_h, int S, int capacity, PairPlan *out)
{
    PairPlan p;
    int used = 0, nseg = 0; // of the open wave
    bool open = false;
    for (int i = 0; i < n; ++i) {
        const int tiles = (items[i].w + out_w - 1) / out_w, h = items[i].h;
        for (int t = 0; t < tiles; ++t) {
            int y = 0;
            while (y < h) {
                if (!open) {
                    if (p.waves == capacity) return false;
                    ++p.waves;
                    p.segs.resize((size_t)p.waves * kPairMaxSegs, PairSeg{0, 0, 0, 0});
                    used = 0, nseg = 0, open = true;
                }
                const int rem = h - y, avail = S - used - overhead;
                int r = rem <= avail ? rem : avail;
                if (r < rem && rem - r < min_h) r = rem - min_h; // (no sliver below the cut either)
                if (r < rem && r < min_h) {
                    if (nseg == 0) return false; // a whole wave cannot take a legal piece of this column
                    open = false;
                    continue;
                }
                p.segs[(size_t)(p.waves - 1) * kPairMaxSegs + nseg] = PairSeg{i, t, y, y + r};
                ++p.segments;
                used += r + overhead, ++nseg, y += r;
                if (used > p.S) p.S = used;
                if (nseg == kPairMaxSegs || S - used <= overhead) open = false;
            }
        }
    }
    *out = p;
    return true;
}

// The plan with the smallest step budget that fits `capacity` waves.  The budgets are tried in order from the bound that the total
// cost sets (the wave count of the greedy fill need not fall monotonically with S, so this is a scan, not a bisection; a fill is a
// few thousand operations and the result is cached per launch shape).  false: no budget fits -- more tile columns than
// kPairMaxSegs x capacity -- and the caller keeps the one-strip-per-wave plan.
inline bool pair_plan_make(const PairItem *items, int n, int out_w, int overhead, int min_h, int capacity, PairPlan *out)
{
    if (n <= 0 || capacity <= 0 || out_w <= 0 || min_h < 1) return false;
    long total = 0;
    int max_h = 0;
    for (int i = 0; i < n; ++i) {
        if (items[i].w <= 0 || items[i].h <= 0) return false;
        total += (long)((items[i].w + out_w - 1) / out_w) * (items[i].h + overhead);
        max_h = items[i].h > max_h ? items[i].h : max_h;
    }
    int S = (int)((total + capacity - 1) / capacity);
    if (S < overhead + 1) S = overhead + 1;
    const int S_max = kPairMaxSegs * (max_h + overhead);
    for (; S <= S_max; ++S)
        if (pair_plan_fill(items, n, out_w, overhead, min_h, S, capacity, out)) return true;
    return false;
}

} // namespace ofx_plan
