/* pvnet_poses.h -- C ABI of libpvnet_poses.so: the pose solve behind the PER-CLASS vote, one pose per (image, class) in one launch.
 *
 * The per-class vote (include/pvnet_classes.h, then pvnet_vote_v3_prepared of include/pvnet_vote.h: the reference's
 * ransac_voting_layer_v2, lib/ransac_voting_gpu_layer/ransac_voting_gpu.py:99-215) returns key-points [b, nk, pn, 2] with
 * nk = class_num - 1 and pn = vn, and a status word per key-point.  Every class has object points of its own, and a class that is not
 * in an image has all-zero key-points.  pvnet_pose_solve (include/pvnet_vote.h) takes ONE point set for all its images, so a caller
 * would slice per class, launch nk times and still solve garbage for the absent classes.  pvnet_pose_solve_classes is that solve for
 * all b * nk items at once:
 *
 *   item (i, k)  image i, class k + 1 -- row i * nk + k of every output, the order of the vote's output
 *
 *   pts2d        [b,nk,pn,2] key-points, float32 (what the vote writes) or float64 (pts2d_f64 != 0), element strides
 *                pts2d_strides[4] (host array), read in place; widened to float64 on read
 *   pts3d        [nk,pn,3] float64 object points, one set per class (every class has pn points: the field has one set of vn
 *                channels)
 *   weights      the three kinds of pvnet_pose_solve, a row per item.  PVNET_POSES_W_NONE: ignored; PVNET_POSES_W_EXPLICIT: float64
 *                [b,nk,pn,3] (wxx, wxy, wyy), residual = W d; PVNET_POSES_W_COV_F32: float32 [b,nk,pn,2,2] covariances, turned into
 *                weights as there: zero when cov[0,0] < 1e-6 or an entry is NaN, else the inverse matrix square root with every
 *                eigenvalue clamped to >= 1e-30.  Contiguous.
 *   K            float64 [3,3], or [b,3,3] with k_per_image != 0: the classes of an image share its camera
 *   vote_status  NULL, or int32 [b,nk,pn] contiguous: the status words of the per-class vote (PVNET_S_* of include/pvnet_vote.h).
 *                An item is ABSENT when any of its pn words has PVNET_S_SKIPPED (the vote sets it for every key-point of a class
 *                with too few pixels).  Other bits do not gate.  Without vote_status every item is solved.
 *   pn           6 .. PVNET_POSES_MAX_PN;  nk  1 .. PVNET_POSES_MAX_CLASSES;  b >= 0 (b == 0 returns 0)
 *   max_iterations  LM iterations per refinement (> 0; the host solver uses 200)
 *   rt           NULL or float64 [b,nk,6] angle-axis | translation;  poses  NULL or float64 [b,nk,3,4] (R | t) -- at least one of
 *                the two
 *   status       NULL or int32 [b,nk]
 *
 * A SOLVED item is pvnet_pose_solve's item: the same linear start, the same refinements (unweighted, then, with weights, weighted
 * from the unweighted optimum), the same status -- the LM iterations (>= 0), or -2 with zeros in rt and poses when the linear start
 * failed.  Both kernels are built on the one copy of the solver (pvnet_amd/csrc/pose_core.h), compiled without contraction: an item
 * has the bits pvnet_pose_solve gives for its key-points, its class's points and its image's camera, whatever its neighbours are.
 *
 * An ABSENT item reads none of its key-points or weights, gets exact zeros in its rows of rt and poses and PVNET_POSES_ABSENT in
 * status, and its wave leaves at once.
 *
 * Kernel shape: ONE launch of b * nk workgroups of one wavefront, a lane per key-point, float64 throughout, 15 KB of LDS; no
 * workspace, no atomics, no allocation, no synchronisation -- capturable in a graph behind the vote, bitwise reproducible.  The
 * solver is latency-bound (a wave's dependent chain), so the launch costs about what one pvnet_pose_solve launch costs while its
 * waves fit the machine at once.
 *
 * Arguments are checked before any HIP call.  Return value: 0, a positive hipError_t, or
 *   PVNET_E_BADARG (-1)       pts2d, pts2d_strides, pts3d or K null; rt and poses both null; b < 0; nk < 1; max_iterations <= 0; an
 *                             unknown weight kind; a kind other than NONE without weights
 *   PVNET_E_UNSUPPORTED (-3)  pn outside 6 .. PVNET_POSES_MAX_PN; nk > PVNET_POSES_MAX_CLASSES; b * nk > PVNET_POSES_MAX_ITEMS
 */
#ifndef PVNET_POSES_H_
#define PVNET_POSES_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVNET_POSES_ABI_VERSION 1
/* weight kinds: the values of PVNET_POSE_W_* (include/pvnet_vote.h) */
#define PVNET_POSES_W_NONE     0
#define PVNET_POSES_W_EXPLICIT 1
#define PVNET_POSES_W_COV_F32  2
#define PVNET_POSES_MAX_PN      64          /* a lane per key-point: PVNET_POSE_MAX_PN */
#define PVNET_POSES_MAX_CLASSES 63          /* classes without the background: PVNET_CLASSES_MAX - 1 */
#define PVNET_POSES_MAX_ITEMS   178956970   /* b * nk at most: 12 entries of a pose per item, indexed in 31 bits (pvnet_pose_solve's n) */
/* status of an absent item; a solved one has pvnet_pose_solve's values (>= 0, or -2) */
#define PVNET_POSES_ABSENT (-3)

int pvnet_poses_abi_version(void);

int pvnet_pose_solve_classes(const void* pts2d, int pts2d_f64, const int64_t pts2d_strides[4],
                             const double* pts3d, const void* weights, int weight_kind,
                             const double* K, int k_per_image, const int32_t* vote_status,
                             int b, int nk, int pn, int max_iterations,
                             double* rt, double* poses, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_POSES_H_ */
