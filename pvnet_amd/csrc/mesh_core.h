// mesh_core.h -- the ONE copy of stage P (pose -> float32 screen vertex) and of stage R's coverage predicate (include/pvnet_raster.h,
// THE DEFINITION).  raster.hip (libpvnet_raster.so) includes it itself; depth.hip, shade.hip and texture.hip compile it with the
// z-buffer of zbuffer_core.h: a colour or textured image is covered exactly where the silhouette is set and the depth image non-zero
// because all four libraries evaluate these functions.
//
// Nothing here may be contracted into a fused multiply-add (tests/test_raster_cpu.py looks for fused float32 instructions in the
// assembly); float32 denormals are kept (the compiler's default for gfx950).
#ifndef PVNET_MESH_CORE_H_
#define PVNET_MESH_CORE_H_

#include <hip/hip_runtime.h>

#pragma STDC FP_CONTRACT OFF

namespace pvd {
namespace {

// stage P for one vertex
__device__ __forceinline__ void project(const double* pose, const double* K, const double* X, float& u, float& v) {
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    const double c0 = ((pose[0] * X0 + pose[1] * X1) + pose[2] * X2) + pose[3];
    const double c1 = ((pose[4] * X0 + pose[5] * X1) + pose[6] * X2) + pose[7];
    const double c2 = ((pose[8] * X0 + pose[9] * X1) + pose[10] * X2) + pose[11];
    const double p0 = (K[0] * c0 + K[1] * c1) + K[2] * c2;
    const double p1 = (K[3] * c0 + K[4] * c1) + K[5] * c2;
    const double p2 = (K[6] * c0 + K[7] * c1) + K[8] * c2;
    u = (float)(p0 / p2);
    v = (float)(p1 / p2);
}

// one edge of same_side: what does not depend on the pixel
struct Edge {
    float xa, ya, nx, ny, val0;
};

__device__ __forceinline__ Edge make_edge(float xa, float ya, float xb, float yb, float tx, float ty) {
    Edge e;
    const float dx = xb - xa, dy = yb - ya;
    e.xa = xa;
    e.ya = ya;
    e.nx = -dy;
    e.ny = dx;
    const float dx0 = tx - xa, dy0 = ty - ya;
    const float a = dx0 * e.nx, b = dy0 * e.ny;
    e.val0 = a + b;
    return e;
}

__device__ __forceinline__ bool same_side(const Edge& e, float px, float py) {
    const float dx1 = px - e.xa, dy1 = py - e.ya;
    const float a = dx1 * e.nx, b = dy1 * e.ny;
    const float val1 = a + b;
    const float prod = e.val0 * val1;
    return prod >= 0.f;
}

__device__ __forceinline__ bool inside(const Edge& e0, const Edge& e1, const Edge& e2, float px, float py) {
    return same_side(e0, px, py) && same_side(e1, px, py) && same_side(e2, px, py);
}

}  // namespace
}  // namespace pvd
#endif  // PVNET_MESH_CORE_H_
