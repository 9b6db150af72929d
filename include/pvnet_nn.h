/* pvnet_nn.h -- C ABI of the brute-force nearest-neighbour search behind the reference's symmetric-object metrics
 * (ADD-S, symmetric 2-D projection error): lib/utils/extend_utils/src/nearest_neighborhood.cu:48-117, bound through
 * cffi as `lib.findNearestPointIdxLauncher` (lib/utils/extend_utils/extend_utils.py:39-60) and consumed by
 * `find_nearest_point_distance` / `Evaluator.add_metric_sym` / `projection_2d_sym`
 * (lib/utils/evaluation_utils.py:54-62,84-91,111-122).  Part of libpvnet_vote.so (pvnet_amd/csrc/pvnet_nn.hip).
 *
 * For every query point the index of the nearest reference point, squared Euclidean distance in float32 in the
 * reference's operation order ((x1-x2)^2 + (y1-y2)^2 [+ (z1-z2)^2], one rounding per operation), FIRST index on ties
 * (the reference's strict `dist < min_dist` scan).  dim is 2 or 3.  exclude_self: reference point i is skipped for
 * query i (nearest OTHER point of one cloud).
 */
#ifndef PVNET_NN_H_
#define PVNET_NN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers; only enqueues on `stream` (no allocation, no synchronisation).
 *   ref_pts [b,pn1,dim] f32, que_pts [b,pn2,dim] f32, idxs [b,pn2] i32 (output),
 *   workspace: pvnet_nearest_workspace_bytes(b, pn2) bytes, 256-byte aligned (one packed (distance, index) word per
 *   query, the running minimum over the reference tiles); read only when the reference cloud is split into more than
 *   one slice, otherwise it may be null.
 * pn1 may be 0 (an empty reference cloud): ref_pts is then not read and may be null, and every query answers index 0,
 * as the reference's scan from `min_idx = 0` does.  pn2 must be at least 1.
 * Returns 0, a positive hipError_t, or a negative PVNET_E_* code (include/pvnet_vote.h). */
size_t pvnet_nearest_workspace_bytes(int b, int pn2);
int pvnet_nearest_point_idx(const float* ref_pts, const float* que_pts, int32_t* idxs, int b, int pn1, int pn2, int dim,
                            int exclude_self, void* workspace, size_t workspace_bytes, void* stream);

/* The reference's own launcher symbol and signature (nearest_neighborhood.cu:120-160): HOST pointers in and out; it
 * allocates device buffers, copies, runs the search on the current device's null stream and copies back, exactly like
 * the original -- so the reference's cffi call `lib.findNearestPointIdxLauncher(...)` binds to it unchanged. */
void findNearestPointIdxLauncher(float* ref_pts, float* que_pts, int* idxs, int b, int pn1, int pn2, int dim,
                                 int exclude_self);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_NN_H_ */
