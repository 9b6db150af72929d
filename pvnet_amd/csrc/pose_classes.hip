// pose_classes.hip -- the pose solve behind the per-class vote: one pose per (image, class) in one launch, one wavefront per item.
// C ABI: pvnet_pose_solve_classes in include/pvnet_poses.h (libpvnet_poses.so).
//
// The solver is pose_core.h, the one copy that pose_solve.hip (libpvnet_vote.so) compiles too; that header also sets
// `#pragma clang fp contract(off)` for the rest of this file.  What is here is what differs from pvnet_pose_solve: where an item's
// inputs are -- item = image * nk + class: the image's camera, the class's object points, four strides into the key-points -- and
// the gate in front of the solve: an item whose vote was skipped reads nothing, writes zeros and PVNET_POSES_ABSENT, and leaves.
#include "pose_core.h"

#include "pvnet_poses.h"

static_assert(PVNET_POSES_W_NONE == PVNET_POSE_W_NONE && PVNET_POSES_W_EXPLICIT == PVNET_POSE_W_EXPLICIT &&
              PVNET_POSES_W_COV_F32 == PVNET_POSE_W_COV_F32 && PVNET_POSES_MAX_PN == PVNET_POSE_MAX_PN,
              "pvnet_poses.h mirrors the weight kinds and the point limit of pvnet_pose_solve");
static_assert(PVNET_POSES_MAX_ITEMS == 2147483647 / 12, "12 entries of a pose per item, indexed in 31 bits");

namespace {

#define PVNET_POSE_CLASSES_SPARE_VGPR 195  // the kernel names v0..v186, as pose_solve_kernel does

struct ClassPoseArgs {
    const void* pts2d;
    int64_t s0, sk, s1, s2;      // element strides of pts2d [b,nk,pn,2]
    int f64;                     // pts2d is float64 (else float32)
    const double* pts3d;         // [nk,pn,3]
    const void* weights;         // PVNET_POSES_W_*, [b,nk,pn,..]
    int weight_kind;
    const double* K;             // [3,3] or [b,3,3]
    int k_per_image;
    const int32_t* vote_status;  // [b,nk,pn] or null
    int nk, pn, max_iterations;
    double* rt;                  // [b,nk,6] or null
    double* poses;               // [b,nk,3,4] or null
    int32_t* status;             // [b,nk] or null
    // where item `it` = image * nk + class is (pose_core.h: PVNET_POSE_KERNEL)
    __device__ const double* camera(int it) const { return K + (k_per_image ? (size_t)(it / nk) * 9 : 0); }
    __device__ int64_t point_offset(int it) const { return (it / nk) * s0 + (it % nk) * sk; }
    __device__ const double* points(int it) const { return pts3d + (size_t)(it % nk) * pn * 3; }
};

// the gate: true (wave-uniform) when a status word of the item has PVNET_S_SKIPPED; its rows are written here then
__device__ inline bool absent(const ClassPoseArgs& A, int it, int lane) {
    if (!A.vote_status) return false;
    const bool skipped = lane < A.pn && (A.vote_status[(size_t)it * A.pn + lane] & PVNET_S_SKIPPED);
    if (!__any(skipped)) return false;
    if (A.rt && lane < 6) A.rt[(size_t)it * 6 + lane] = 0.0;
    if (A.poses && lane < 12) A.poses[(size_t)it * 12 + lane] = 0.0;
    if (A.status && lane == 0) A.status[it] = PVNET_POSES_ABSENT;
    return true;
}

PVNET_POSE_KERNEL(pose_classes_kernel, ClassPoseArgs, PVNET_POSE_CLASSES_SPARE_VGPR, if (absent(A, img, lane)) return)

}  // namespace

extern "C" int pvnet_poses_abi_version(void) { return PVNET_POSES_ABI_VERSION; }

extern "C" int pvnet_pose_solve_classes(const void* pts2d, int pts2d_f64, const int64_t pts2d_strides[4], const double* pts3d,
                                        const void* weights, int weight_kind, const double* K, int k_per_image,
                                        const int32_t* vote_status, int b, int nk, int pn, int max_iterations, double* rt,
                                        double* poses, int32_t* status, void* stream) {
    if (!pts2d || !pts2d_strides || !pts3d || !K || (!rt && !poses) || b < 0 || nk < 1 || max_iterations <= 0) return PVNET_E_BADARG;
    if (weight_kind != PVNET_POSES_W_NONE && weight_kind != PVNET_POSES_W_EXPLICIT && weight_kind != PVNET_POSES_W_COV_F32)
        return PVNET_E_BADARG;
    if (weight_kind != PVNET_POSES_W_NONE && !weights) return PVNET_E_BADARG;
    if (pn < 6 || pn > PVNET_POSES_MAX_PN) return PVNET_E_UNSUPPORTED;   // the linear start needs 6 points; a lane per point
    if (nk > PVNET_POSES_MAX_CLASSES) return PVNET_E_UNSUPPORTED;
    if ((int64_t)b * nk > PVNET_POSES_MAX_ITEMS) return PVNET_E_UNSUPPORTED;
    if (b == 0) return 0;
    ClassPoseArgs A;
    A.pts2d = pts2d;
    A.s0 = pts2d_strides[0];
    A.sk = pts2d_strides[1];
    A.s1 = pts2d_strides[2];
    A.s2 = pts2d_strides[3];
    A.f64 = pts2d_f64 ? 1 : 0;
    A.pts3d = pts3d;
    A.weights = weights;
    A.weight_kind = weight_kind;
    A.K = K;
    A.k_per_image = k_per_image ? 1 : 0;
    A.vote_status = vote_status;
    A.nk = nk;
    A.pn = pn;
    A.max_iterations = max_iterations;
    A.rt = rt;
    A.poses = poses;
    A.status = status;
    hipLaunchKernelGGL(pose_classes_kernel, dim3((unsigned)(b * nk)), dim3(PS_LANES), 0, static_cast<hipStream_t>(stream), A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
