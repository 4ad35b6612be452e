// The schedule of a pair's refinement iterations 2 .. iters: which accumulating launches follow iteration 1,
// how many iterations each carries, and which flow set and which warped plane each reads and writes.  Plain host code without HIP in
// it, so that tests/test_iter_plan.py compiles it into a stand-alone program.  A session makes its plans once (ofx_session_create);
// the stream tick and the pair-at-a-time path only walk them.
#pragma once

#include <assert.h>

namespace ofx_plan {

constexpr int kMaxIterPasses = 63; // ofx_session_create takes iters <= 64, and iteration 1 is not a pass

struct IterPass {
    int it;        // iterations done before this launch (1 ..)
    int count;     // 1, or 2: a two-iteration launch (lk_body_pair.h)
    bool shift;    // a shift launch precedes it (unfused sessions: once, before iteration 2)
    bool warp;     // a warp launch precedes it (unfused sessions: always)
    bool wout;     // the launch also writes the warped image of the launch after it (lk_body_warp.h)
    int win, wo;   // 0 / 1: the warped plane it reads, and (wout) the one it writes
    int fin, fout; // 0 / 1: the flow set it reads / writes (0 = flowset, 1 = flowset2); fin == fout unless count == 2
};

// fused: the launches write the next launch's warped image themselves, into the other of two planes (iteration 1 wrote plane 0) --
// otherwise a warp launch writes plane 0 before every pass, and a shift launch makes its source before the first.  pairs: iterations
// two per launch, paired from the front; a left-over one runs last, alone and in place.  A two-iteration launch moves the flow to the
// other set, and the last launch writes set 0: the set iteration 1 has to write is out[0].fin.  Returns the number of passes.
inline int iter_plan_make(int iters, bool fused, bool pairs, IterPass *out)
{
    assert(iters <= kMaxIterPasses + 1 && (!pairs || fused));
    int n = 0;
    for (int it = 1, win = 0; it < iters; ++n) {
        const int count = pairs && it + 2 <= iters ? 2 : 1;
        out[n] = IterPass{it, count, !fused && it == 1, !fused, fused && it + count < iters, win, 1 - win, 0, 0};
        if (fused) win = 1 - win;
        it += count;
    }
    for (int i = n - 1, set = 0; i >= 0; --i) { // backwards from the result
        out[i].fout = set;
        if (out[i].count == 2) set = 1 - set;
        out[i].fin = set;
    }
    return n;
}

} // namespace ofx_plan
