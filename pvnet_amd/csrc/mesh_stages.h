// mesh_stages.h -- stage P (pose -> float32 screen vertex) and stage R's coverage predicate (include/pvnet_raster.h, THE DEFINITION) as
// raster.hip and depth.hip reach them through raster_common.h and shade.hip (libpvnet_shade.so) by this name: a colour image is covered
// exactly where the silhouette is set and the depth image non-zero because all three evaluate these functions.
//
// The bodies live in mesh_core.h, which libpvnet_texture.so compiles from there; this header only includes it.
#ifndef PVNET_MESH_STAGES_H_
#define PVNET_MESH_STAGES_H_

#include "mesh_core.h"   // the bodies: project, Edge, make_edge, same_side, inside

#endif  // PVNET_MESH_STAGES_H_
