// One family of instantiations of the templates in lk_launch.h (see there).
#include "lk_inst.h"

template int ofx_launch::stream<OFX_MODE_LK_FLOAT, true>(int, const LkLevelIn *, int, bool, bool, StreamArgs &, const int *, size_t, hipStream_t);
