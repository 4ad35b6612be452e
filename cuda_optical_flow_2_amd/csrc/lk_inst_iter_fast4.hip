// One family of instantiations of the templates in lk_launch.h (see there): refinement iterations on the buffer march, ITER = 4
// (an accumulating launch that also writes the next warped image, on the row windows of a shard).
#include "lk_inst.h"

template int ofx_launch::iter<OFX_MODE_LK_FLOAT, true, 4>(int, const LkLevelIn *, int, bool, hipStream_t);
