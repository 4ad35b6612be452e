// One family of instantiations of the templates in lk_launch.h (see there): two refinement iterations per launch (lk_body_pair.h),
// the reference solve; the second iteration with and without the warped image of the one after it.
#include "lk_inst.h"

template int ofx_launch::iter_pair<false, false>(int, const LkLevelIn *, int, const ofx_pair_opts *, hipStream_t);
template int ofx_launch::iter_pair<false, true>(int, const LkLevelIn *, int, const ofx_pair_opts *, hipStream_t);
