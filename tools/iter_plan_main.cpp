// The schedule of the refinement iterations (csrc/iter_plan.h) as a stand-alone host program: prints the plan for the session
// described on the command line.  tests/test_iter_plan.py builds and checks it.
//
//   iter_plan_main ITERS FUSED PAIRS
//
// Output: "plan PASSES" and one line "IT COUNT SHIFT WARP WOUT WIN WO FIN FOUT" per pass.
#include <stdio.h>
#include <stdlib.h>

#include "iter_plan.h"

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: %s ITERS FUSED PAIRS\n", argv[0]);
        return 2;
    }
    const int iters = atoi(argv[1]);
    const bool fused = atoi(argv[2]) != 0, pairs = atoi(argv[3]) != 0;
    if (iters < 0 || iters > ofx_plan::kMaxIterPasses + 1 || (pairs && !fused)) {
        fprintf(stderr, "%s: ITERS 0 .. %d, and PAIRS needs FUSED\n", argv[0], ofx_plan::kMaxIterPasses + 1);
        return 2;
    }
    ofx_plan::IterPass plan[ofx_plan::kMaxIterPasses];
    const int n = ofx_plan::iter_plan_make(iters, fused, pairs, plan);
    printf("plan %d\n", n);
    for (int i = 0; i < n; ++i) {
        const ofx_plan::IterPass &q = plan[i];
        printf("%d %d %d %d %d %d %d %d %d\n", q.it, q.count, (int)q.shift, (int)q.warp, (int)q.wout, q.win, q.wo, q.fin, q.fout);
    }
    return 0;
}
