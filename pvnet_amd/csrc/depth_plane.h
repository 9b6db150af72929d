// depth_plane.h -- the depth of a covered pixel under one triangle (include/pvnet_depth.h, THE DEFINITION) as depth.hip
// (libpvnet_depth.so) and shade.hip (libpvnet_shade.so) reach it: the depth a colour render writes is the depth render's because both
// evaluate these functions.
//
// The bodies live in depth_core.h, which libpvnet_texture.so compiles from there; this header only includes it.
#ifndef PVNET_DEPTH_PLANE_H_
#define PVNET_DEPTH_PLANE_H_

#include "depth_core.h"   // the bodies: camera_z, Plane, make_plane, pixel_depth

#endif  // PVNET_DEPTH_PLANE_H_
