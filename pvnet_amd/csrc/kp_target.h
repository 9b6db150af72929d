// kp_target.h -- THE definition of a vector-field target, written once for the two translation units that make targets from key-points:
// head_targets.hip (libpvnet_targets.so: one set of key-points per image) and class_targets.hip (libpvnet_class_targets.so: one set
// per class, picked by the pixel's label).  Nothing else in the project makes a target.  Both functions are inlined into the kernel
// that calls them: the two libraries share source, not symbols.  namespace pvh.
#pragma once
#include <hip/hip_runtime.h>

// no contraction: vx vx + vy vy and hx - x hz round as the reference's separate numpy operations do
#pragma clang fp contract(off)

namespace pvh {

// ---- THE definition (linemod_dataset.py:72-77): the target of the pixel (x, y) with mask == 1 for the key-point (hx, hy, hz).  Every
//      operation is one IEEE float64 operation, in the reference's order; the result is rounded once to float32 ----------------------
__device__ __forceinline__ void kp_target(double hx, double hy, double hz, int x, int y, bool motion, float& tx, float& ty) {
    double vx = hx - (double)x * hz, vy = hy - (double)y * hz;
    if (!motion) {
        double n = sqrt(vx * vx + vy * vy);
        if (n < 1e-3) n = n + 1e-3;
        vx = vx / n;
        vy = vy / n;
    }
    tx = (float)vx;
    ty = (float)vy;
}

// the weight of a pixel of the single-class targets: the mask's value as float32 (mask.float()) times the image's scale
__device__ __forceinline__ float kp_weight(long long m, float scale) { return (float)m * scale; }

}  // namespace pvh
