// raster_common.h -- the ONE copy of stage P (pose -> float32 screen vertex) and of stage R's coverage predicate (include/pvnet_raster.h,
// THE DEFINITION), compiled by raster.hip (libpvnet_raster.so) and depth.hip (libpvnet_depth.so): a depth image is non-zero exactly
// where the silhouette is set because both evaluate these functions.
//
// Nothing here may be contracted into a fused multiply-add (tests/test_raster_cpu.py looks for fused float32 instructions in the
// assembly); float32 denormals are kept (the compiler's default for gfx950).
#ifndef PVNET_RASTER_COMMON_H_
#define PVNET_RASTER_COMMON_H_

#include "mesh_stages.h"   // the bodies: project, Edge, make_edge, same_side, inside (libpvnet_shade.so compiles them from there)

#endif  // PVNET_RASTER_COMMON_H_
