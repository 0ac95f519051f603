// odu.hip's fused OverlapDetection res block with two strips per workgroup on one weight stream.
// See odw.hip.  Same arguments, same bits.
#pragma once
#include "odu.h"

// block geometry (h, w, cin, c, pool) that odw_launch runs: the blocks measured faster than on odu
bool odw_supported(int h, int w, int cin, int c, bool pool);
hipError_t odw_launch(const OduArgs& a, int h, int w, int cin, int c, bool pool, hipStream_t stream);
