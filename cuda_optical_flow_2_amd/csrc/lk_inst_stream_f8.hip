// One family of instantiations of the templates in lk_launch.h (see there): the stream tick with eight columns per lane.
#include "lk_inst.h"

template int ofx_launch::stream<OFX_MODE_LK_FLOAT, false, 0, 8>(int, const LkLevelIn *, int, StreamArgs &, const int *, size_t, hipStream_t);
template int ofx_launch::iter<OFX_MODE_LK_FLOAT, false, 0, 8>(int, const LkLevelIn *, int, hipStream_t); // all levels of one pair (the pair-at-a-time path)
