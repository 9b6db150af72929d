// pose_solve.hip -- the pose solve after voting, on the device: pvnet_pnp_solve (pvnet_amd/csrc/pvnet_pnp.cpp) restated for
// gfx950, one image per wavefront, float64 throughout.  C ABI: pvnet_pose_solve in include/pvnet_vote.h.
//
// Replaces the host round trip of every batch (synchronise, copy the key-points out, pvnet_pnp_solve_batch on a thread pool, copy
// the poses back): key-points in, poses out, on the voting stream, so voting and pose can be captured in one graph.
//
// The solver itself -- the linear start, the refinement, the covariance weights and the per-item body this kernel runs -- is
// pose_core.h, shared with pose_classes.hip (libpvnet_poses.so).  That header also sets `#pragma clang fp contract(off)` for the
// rest of this file: the host library is compiled without FMA, and the device must round every product and sum as it does.
// What is here: the arguments, the kernel (an image is an item; one point set for all) and the entry point with its checks.
#include "pose_core.h"

namespace {

#define PVNET_POSE_SPARE_VGPR 195  // the kernel names v0..v186

struct PoseArgs {
    const void* pts2d;
    int64_t s0, s1, s2;   // element strides of pts2d [n,pn,2]
    int f64;              // pts2d is float64 (else float32)
    const double* pts3d;  // [pn,3]
    const void* weights;  // PVNET_POSE_W_*
    int weight_kind;
    const double* K;      // [3,3] or [n,3,3]
    int k_per_image;
    int n, pn, max_iterations;
    double* rt;           // [n,6] or null
    double* poses;        // [n,3,4] or null
    int32_t* status;      // [n] or null
    // where item `img` is (pose_core.h: pose_item)
    __device__ __forceinline__ const double* camera(int img) const { return K + (k_per_image ? (size_t)img * 9 : 0); }
    __device__ __forceinline__ int64_t point_offset(int img) const { return img * s0; }
    __device__ __forceinline__ const double* points(int) const { return pts3d; }
};

PVNET_POSE_KERNEL(pose_solve_kernel, PoseArgs, PVNET_POSE_SPARE_VGPR, (void)0)

}  // namespace

extern "C" int pvnet_pose_solve(const void* pts2d, int pts2d_f64, const int64_t pts2d_strides[3], const double* pts3d,
                                const void* weights, int weight_kind, const double* K, int k_per_image, int n, int pn,
                                int max_iterations, double* rt, double* poses, int32_t* status, void* stream) {
    if (!pts2d || !pts2d_strides || !pts3d || !K || (!rt && !poses) || n < 0 || max_iterations <= 0) return PVNET_E_BADARG;
    if (weight_kind != PVNET_POSE_W_NONE && weight_kind != PVNET_POSE_W_EXPLICIT && weight_kind != PVNET_POSE_W_COV_F32)
        return PVNET_E_BADARG;
    if (weight_kind != PVNET_POSE_W_NONE && !weights) return PVNET_E_BADARG;
    if (pn < 6 || pn > PVNET_POSE_MAX_PN) return PVNET_E_UNSUPPORTED;   // the linear start needs 6 points; a lane per point
    if (n > 2147483647 / 12) return PVNET_E_UNSUPPORTED;
    if (n == 0) return 0;
    PoseArgs A;
    A.pts2d = pts2d;
    A.s0 = pts2d_strides[0];
    A.s1 = pts2d_strides[1];
    A.s2 = pts2d_strides[2];
    A.f64 = pts2d_f64 ? 1 : 0;
    A.pts3d = pts3d;
    A.weights = weights;
    A.weight_kind = weight_kind;
    A.K = K;
    A.k_per_image = k_per_image ? 1 : 0;
    A.n = n;
    A.pn = pn;
    A.max_iterations = max_iterations;
    A.rt = rt;
    A.poses = poses;
    A.status = status;
    hipLaunchKernelGGL(pose_solve_kernel, dim3((unsigned)n), dim3(PS_LANES), 0, static_cast<hipStream_t>(stream), A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
