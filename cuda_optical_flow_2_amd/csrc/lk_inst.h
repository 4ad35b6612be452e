// The launch families declared in lk_launch.h, defined: included by the lk_inst_*.hip translation units only, each of which
// instantiates one of them explicitly (and with it the family's kernels, radii 1..11 or 12).
#pragma once

#include "lk_launch.h"

namespace ofx_launch {

template <int MODE, bool FAST>
int levels(int radius, const LkLevelIn *lv, int n, bool sums, hipStream_t st)
{
    int rc = OFX_E_UNSUPPORTED;
    const bool known = dispatch_radius<lk_max_radius(MODE)>(radius, [&](auto R) {
        if constexpr (!FAST) {
            if (sums) {
                rc = launch_r<decltype(R)::value, MODE, true, false>(lv, n, st);
                return;
            }
        }
        rc = launch_r<decltype(R)::value, MODE, false, FAST>(lv, n, st);
    });
    if (!known) ofx_set_error("ofx_lk_level: window %d not supported in mode %d", 2 * radius + 1, MODE);
    return rc;
}

template <int MODE, bool FAST, int ITER>
int iter(int radius, const LkLevelIn *lv, int n, bool deep, hipStream_t st)
{
    int rc = OFX_E_UNSUPPORTED;
    const bool known = dispatch_radius<lk_max_radius(MODE)>(radius, [&](auto R) {
        rc = deep ? launch_iter_r<decltype(R)::value, MODE, FAST, ITER, true>(lv, n, st) : launch_iter_r<decltype(R)::value, MODE, FAST, ITER, false>(lv, n, st);
    });
    if (!known) ofx_set_error("ofx_lk_level: window %d not supported in mode %d", 2 * radius + 1, MODE);
    return rc;
}

template <bool FAST, bool WOUT>
int iter_pair(int radius, const LkLevelIn *lv, int n, const ofx_pair_opts *opts, hipStream_t st)
{
    int rc = OFX_E_UNSUPPORTED;
    const bool known = dispatch_radius<kLkPairMaxR>(radius, [&](auto R) { rc = launch_pair_r<decltype(R)::value, FAST, WOUT>(lv, n, opts, st); });
    if (!known) ofx_set_error("ofx_lk_levels_pair: window %d not supported", 2 * radius + 1);
    return rc;
}

template <int MODE, bool FAST, int WOUT>
int stream(int radius, const LkLevelIn *lv, int n, bool deep, bool many, StreamArgs &S, const int *stage_blocks, size_t lds, hipStream_t st)
{
    int rc = OFX_E_UNSUPPORTED;
    const bool known = dispatch_radius<lk_max_radius(MODE)>(radius, [&](auto R) {
        if constexpr (WOUT == ofx_plan::kIterSet) { // (the ticks that write warped images have no deep-fetch kernels)
            if (deep) {
                rc = launch_stream_r<decltype(R)::value, MODE, FAST, true, WOUT>(lv, n, many, S, stage_blocks, lds, st);
                return;
            }
        }
        rc = launch_stream_r<decltype(R)::value, MODE, FAST, false, WOUT>(lv, n, many, S, stage_blocks, lds, st);
    });
    if (!known) ofx_set_error("ofx_stream_launch: window %d not supported in mode %d", 2 * radius + 1, MODE);
    return rc;
}

} // namespace ofx_launch
