// One family of instantiations of the templates in lk_launch.h (see there): refinement iterations on the buffer march, ITER = 1.
#include "lk_inst.h"

template int ofx_launch::iter<OFX_MODE_LK_FLOAT, true, 1>(int, const LkLevelIn *, int, bool, hipStream_t);
