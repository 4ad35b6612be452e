// One family of instantiations of the templates in lk_launch.h (see there): the stream tick whose LK stage also writes the
// warped images of its pairs' second refinement iteration (lk_wave_buf's ITER = 3).
#include "lk_inst.h"

template int ofx_launch::stream<OFX_MODE_LK_FLOAT, false, 3>(int, const LkLevelIn *, int, bool, bool, StreamArgs &, const int *, size_t, hipStream_t);
