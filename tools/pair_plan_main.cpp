// The planner of the fused two-iteration launch (csrc/pair_plan.h) as a stand-alone host program: prints the plan for the items
// given on the command line.  tests/test_pair_plan.py builds and checks it; it is also how the figures in DESIGN.md section 4.5
// were taken.
//
//   pair_plan_main OUT_W OVERHEAD MIN_H CAPACITY  W H [W H ...]
//
// Output: "plan WAVES SEGMENTS S" and one line "WAVE ITEM TILE Y0 Y1" per segment, or "none" when no budget fits.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pair_plan.h"

int main(int argc, char **argv)
{
    if (argc < 7 || ((argc - 5) & 1)) {
        fprintf(stderr, "usage: %s OUT_W OVERHEAD MIN_H CAPACITY W H [W H ...]\n", argv[0]);
        return 2;
    }
    const int out_w = atoi(argv[1]), overhead = atoi(argv[2]), min_h = atoi(argv[3]), capacity = atoi(argv[4]);
    std::vector<ofx_plan::PairItem> items;
    for (int i = 5; i + 1 < argc; i += 2) items.push_back(ofx_plan::PairItem{atoi(argv[i]), atoi(argv[i + 1])});
    ofx_plan::PairPlan p;
    if (!ofx_plan::pair_plan_make(items.data(), (int)items.size(), out_w, overhead, min_h, capacity, &p)) {
        printf("none\n");
        return 0;
    }
    printf("plan %d %d %d\n", p.waves, p.segments, p.S);
    for (int w = 0; w < p.waves; ++w)
        for (int k = 0; k < ofx_plan::kPairMaxSegs; ++k) {
            const ofx_plan::PairSeg &g = p.segs[(size_t)w * ofx_plan::kPairMaxSegs + k];
            if (g.y1 > g.y0) printf("%d %d %d %d %d\n", w, g.item, g.tile, g.y0, g.y1);
        }
    return 0;
}
