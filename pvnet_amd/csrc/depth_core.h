// depth_core.h -- the ONE copy of the depth of a covered pixel under one triangle (include/pvnet_depth.h, THE DEFINITION): the plane of
// inverse depth in float64, clamped to the triangle's z range.  Compiled by depth.hip (libpvnet_depth.so), shade.hip
// (libpvnet_shade.so) and texture.hip (libpvnet_texture.so) with the triangle walk of zbuffer_core.h: the depth a colour or textured
// render writes is the depth render's because all three evaluate these functions.
//
// Nothing here may be contracted into a fused multiply-add; float64 denormals are kept (the compiler's default for gfx950).
#ifndef PVNET_DEPTH_CORE_H_
#define PVNET_DEPTH_CORE_H_

#include <hip/hip_runtime.h>

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

// camera z of one vertex: the c_2 of stage P (the same expression as in project(): the same bits)
__device__ __forceinline__ double camera_z(const double* pose, const double* X) {
    return ((pose[8] * X[0] + pose[9] * X[1]) + pose[10] * X[2]) + pose[11];
}

// the plane of inverse depth of one triangle: what does not depend on the pixel
struct Plane {
    double x0, y0, i0, b, c, zmin, zmax;
    int flat;   // area == 0
};

__device__ __forceinline__ Plane make_plane(float fx0, float fy0, float fx1, float fy1, float fx2, float fy2, double z0, double z1,
                                            double z2) {
    Plane p;
    const double x0 = (double)fx0, y0 = (double)fy0, x1 = (double)fx1, y1 = (double)fy1, x2 = (double)fx2, y2 = (double)fy2;
    const double i0 = 1.0 / z0, i1 = 1.0 / z1, i2 = 1.0 / z2;
    p.zmin = fmin(fmin(z0, z1), z2);
    p.zmax = fmax(fmax(z0, z1), z2);
    const double dx1 = x1 - x0, dy1 = y1 - y0, dx2 = x2 - x0, dy2 = y2 - y0, di1 = i1 - i0, di2 = i2 - i0;
    const double a0 = dx1 * dy2, a1 = dx2 * dy1;
    const double area = a0 - a1;
    const double b0 = di1 * dy2, b1 = di2 * dy1;
    const double c0 = di2 * dx1, c1 = di1 * dx2;
    p.b = (b0 - b1) / area;
    p.c = (c0 - c1) / area;
    p.x0 = x0;
    p.y0 = y0;
    p.i0 = i0;
    p.flat = area == 0.0 ? 1 : 0;
    return p;
}

__device__ __forceinline__ float pixel_depth(const Plane& p, float px, float py) {
    const double ex = (double)px - p.x0, ey = (double)py - p.y0;
    const double tb = p.b * ex, tc = p.c * ey;
    const double s = p.i0 + tb;
    const double inv = s + tc;
    double d = 1.0 / inv;
    if (p.flat) d = p.zmin;
    if (!(d >= p.zmin)) d = p.zmin;
    if (d > p.zmax) d = p.zmax;
    return (float)d;
}

}  // namespace
}  // namespace pvd
#endif  // PVNET_DEPTH_CORE_H_
