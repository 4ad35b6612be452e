// One family of instantiations of the templates in lk_launch.h (see there).
#include "lk_inst.h"

template int ofx_launch::levels<OFX_MODE_LK_FLOAT, false>(int, const LkLevelIn *, int, bool, hipStream_t);
