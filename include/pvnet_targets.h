/* pvnet_targets.h -- C ABI of libpvnet_targets.so: the training targets of the vector field made on the device from the key-points,
 * and the network head's forward and backward fused with them.
 *
 * The reference makes the target field `vertex [2vn,h,w]` and its weights `vertex_weights [1,h,w]` on the host, per sample
 * (compute_vertex_hcoords, lib/datasets/linemod_dataset.py:68-81, called at :224-227), and ships them to the device: 76 bytes per
 * pixel at vn = 9.  Both are a pure function of the mask and of the image's homogeneous 2-D key-points `hcoords [vn,3]`, 27 numbers.
 * pvnet_vertex_targets is that function for a batch, bit for bit; pvnet_head_metrics_kp and pvnet_head_grad_kp are
 * pvnet_head_metrics (include/pvnet_head.h) and pvnet_head_grad (include/pvnet_train.h) with the target and the weight of a pixel
 * computed in registers by the same device function, so the field is never written or read.
 *
 * The target, for a pixel with mask == 1 at column x, row y and key-point (hx, hy, hz), in float64 without contraction:
 *
 *   v = (hx - x hz, hy - y hz);  n = sqrt(vx vx + vy vy);  if n < 1e-3 then n = n + 1e-3;  t = (vx / n, vy / n)
 *
 * each component rounded once to float32; with PVNET_TARGETS_F_MOTION (the reference's use_motion) t = v, rounded once.  Every
 * other pixel gets 0: the target's foreground is mask == 1, NOT the head's mask != 0.  A NaN key-point gives NaN targets on its
 * image's mask == 1 pixels only.  The weight of a pixel is (float)mask * weight_scale[image]: the mask's VALUE, as the reference's
 * mask.float() gives it (a mask value 2 is no target pixel but weighs 2).
 *
 * A library of its own beside libpvnet_head.so, libpvnet_train.so and libpvnet_vote.so, whose ABIs it leaves alone.  It shares their
 * error codes (PVNET_E_*), mask codes (PVNET_MASK_U8 / _I32 / _I64), the flags PVNET_HEAD_F_* and the status bit
 * PVNET_HEAD_S_BAD_LABEL by value and defines only what is new.  No atomics, fixed summation orders: two calls agree bit for bit.
 */
#ifndef PVNET_TARGETS_H
#define PVNET_TARGETS_H

#include <stddef.h>
#include <stdint.h>

#include "pvnet_head.h"

#define PVNET_TARGETS_ABI_VERSION 1

/* a flag of all three calls, beside the PVNET_HEAD_F_* of the two fused ones: targets are the unnormalised v (use_motion=True) */
#define PVNET_TARGETS_F_MOTION 64

#ifdef __cplusplus
extern "C" {
#endif

int pvnet_targets_abi_version(void);

/* Enqueues the targets of b images on `stream`; allocates nothing, synchronises nothing, needs no workspace.  Arguments are checked
 * before any HIP call.  All pointers but `stream` and the stride arrays are device pointers; strides are in elements.
 *
 *   mask            [b,h,w], mask_dtype PVNET_MASK_U8 / _I32 / _I64, strides mask_strides
 *   hcoords         [b,vn,3] float64, contiguous
 *   weight_scale    NULL (1) or [b] float32: the reference's `ver_weight *= 0.0` of its "fuse" images
 *   flags           0 or PVNET_TARGETS_F_MOTION
 *   vertex          NULL or [b,2vn,h,w] float32, strides v_strides: plane 2k is x, plane 2k+1 is y of key-point k
 *   vertex_weights  NULL or [b,1,h,w] float32, strides w_strides (b, h, w)
 *
 * Both outputs NULL is an error; the stride array of a NULL output may be NULL.  Every element of an output that is asked for is
 * written.  Eight pixels per lane and 16 bytes per store where the planes of the outputs and of the mask are contiguous in the
 * pixels and 16-byte aligned and h * w is a multiple of 8; element by element otherwise.  One launch.
 *
 * Returns 0, PVNET_E_BADARG, PVNET_E_UNSUPPORTED (b > 65535, h*w > 2^30, other mask types) or a hipError_t.  b == 0 returns 0 and
 * enqueues nothing. */
int pvnet_vertex_targets(const void* mask, int mask_dtype, const int64_t mask_strides[3], const double* hcoords,
                         const float* weight_scale, int b, int h, int w, int vn, uint32_t flags, float* vertex,
                         const int64_t v_strides[4], float* vertex_weights, const int64_t w_strides[3], void* stream);

/* bytes of workspace a call with these sizes needs (0 for sizes the call rejects); the workspace may hold anything on entry */
size_t pvnet_head_metrics_kp_workspace_bytes(int b, int h, int w);

/* pvnet_head_metrics (include/pvnet_head.h) with `vertex_target` + strides and `vertex_weights` + strides replaced by `hcoords`
 * and `weight_scale` as above, and PVNET_TARGETS_F_MOTION accepted in `flags`.  Same outputs, launches, grid, segment size and
 * summation order: the results equal pvnet_head_metrics on the output of pvnet_vertex_targets bit for bit.  The predictions are
 * read at every pixel, background included: a NaN there reaches loss_vertex as 0 * NaN does. */
int pvnet_head_metrics_kp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                          const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                          int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                          double* losses, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

size_t pvnet_head_grad_kp_workspace_bytes(int b, int h, int w);

/* pvnet_head_grad (include/pvnet_train.h) with the same replacement: the gradients equal pvnet_head_grad on the output of
 * pvnet_vertex_targets bit for bit.  A NULL gradient pointer skips that half (its stride array may be NULL then); the mask is read
 * by either half. */
int pvnet_head_grad_kp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                       const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                       int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                       const double* upstream, void* grad_seg, const int64_t gs_strides[4], void* grad_vertex,
                       const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PVNET_TARGETS_H */
