/* pvnet_class_targets.h -- C ABI of libpvnet_class_targets.so: the training targets of the vector field for images that hold several
 * objects, made on the device from a LABEL image and one set of key-points per class, and the network head's forward and backward
 * fused with them.
 *
 * pvnet_vertex_targets (include/pvnet_targets.h) takes one set of key-points per image; its foreground is mask == 1 and a pixel's
 * weight is the mask's value.  Here the pixel's label picks the key-points.  Inputs:
 *
 *   labels        [b,h,w], PVNET_MASK_U8 / _I32 / _I64, any strides
 *   class_num     nk + 1: the classes, the background (label 0) counted
 *   hcoords       [b,nk,vn,3] float64, contiguous: row k holds the homogeneous 2-D key-points of class k + 1
 *   weight_scale  NULL (all 1) or [b,nk] float32
 *
 * For the pixel at column x, row y of image i with label l:
 *
 *   1 <= l <= nk      the target of key-point j is the target pvnet_targets.h defines for the key-point hcoords[i, l-1, j] at (x, y) --
 *                     the same device function, operation for operation: float64 without contraction, each component rounded once to
 *                     float32, unnormalised with PVNET_TARGETS_F_MOTION.  The weight is weight_scale[i, l-1], or 1.0f without a scale.
 *   every other l     (0, negative, >= class_num): every target is +0.0f and the weight is 0.0f.
 *
 * What follows from that:
 *
 *   Selection, not a sum.  On the pixels of label k + 1 the outputs equal, bit for bit and the sign of a zero included, what
 *       pvnet_vertex_targets gives for the binary mask labels == k + 1 and hcoords[:, k].
 *   nk = 1 on a 0/1 mask.  The result equals pvnet_vertex_targets bit for bit.  On a mask value of 2 it does not: the weight is 0
 *       here and 2 there.  This is the one deliberate difference.  (Bit for bit with no scale or a scale that is finite and not
 *       negative.  The background weighs 0 * scale there and 0.0f here: under a negative scale that is -0.0 against +0.0, equal as
 *       numbers and in every loss and gradient made of them; under a NaN or infinite scale it is NaN there and 0 here.)
 *   NaN key-points.  A NaN key-point gives NaN targets on its class's pixels only, whatever that class's weight.
 *   Predictions are read at every pixel by the fused forms, background included, as by the single-class ones: a NaN there reaches
 *       loss_vertex and the gradient as 0 * NaN does.
 *
 * A library of its own beside libpvnet_targets.so, whose ABI it leaves alone.  It shares the error codes (PVNET_E_*), the mask codes,
 * the flags PVNET_HEAD_F_* and PVNET_TARGETS_F_MOTION and the status bit PVNET_HEAD_S_BAD_LABEL by value, and the limit of the class
 * count with PVNET_CLASSES_MAX of include/pvnet_classes.h by value.  No atomics, fixed summation orders: two calls agree bit for bit.
 */
#ifndef PVNET_CLASS_TARGETS_H
#define PVNET_CLASS_TARGETS_H

#include <stddef.h>
#include <stdint.h>

#include "pvnet_targets.h"

#define PVNET_CLASS_TARGETS_ABI_VERSION 1

/* class_num lies in 2 .. PVNET_CLASS_TARGETS_MAX_CLASSES (PVNET_E_BADARG otherwise), and an image's table of key-points, held in
 * the workgroup's local memory, has at most PVNET_CLASS_TARGETS_MAX_TABLE of them: (class_num - 1) * vn beyond that is
 * PVNET_E_UNSUPPORTED.  63 classes of 16 key-points and 13 of 78 fit. */
#define PVNET_CLASS_TARGETS_MAX_CLASSES 64
#define PVNET_CLASS_TARGETS_MAX_TABLE 1024

#ifdef __cplusplus
extern "C" {
#endif

int pvnet_class_targets_abi_version(void);

/* pvnet_vertex_targets with `mask` a label image, `class_num` behind `weight_scale`, and `hcoords` / `weight_scale` per class as
 * above.  The same output rules: `vertex` NULL or [b,2vn,h,w] float32, `vertex_weights` NULL or [b,1,h,w] float32, both NULL is an
 * error, the stride array of a NULL output may be NULL, every element of an output that is asked for is written.  Eight pixels per
 * lane and 16 bytes per store where the planes of the outputs and of the labels are contiguous in the pixels and 16-byte aligned and
 * h * w is a multiple of 8; element by element otherwise.  One launch; arguments are checked before any HIP call.
 *
 * Returns 0, PVNET_E_BADARG, PVNET_E_UNSUPPORTED (b > 65535, h*w > 2^30, other label types, a table beyond
 * PVNET_CLASS_TARGETS_MAX_TABLE) or a hipError_t.  b == 0 returns 0 and enqueues nothing. */
int pvnet_vertex_targets_classes(const void* mask, int mask_dtype, const int64_t mask_strides[3], const double* hcoords,
                                 const float* weight_scale, int class_num, int b, int h, int w, int vn, uint32_t flags, float* vertex,
                                 const int64_t v_strides[4], float* vertex_weights, const int64_t w_strides[3], void* stream);

/* bytes of workspace a call with these sizes needs (0 for sizes the call rejects): those of pvnet_head_metrics_kp_workspace_bytes */
size_t pvnet_head_metrics_ckp_workspace_bytes(int b, int h, int w);

/* pvnet_head_metrics_kp (include/pvnet_targets.h) with hcoords [b,num_classes-1,vn,3] and weight_scale NULL or [b,num_classes-1]:
 * nk is num_classes - 1, there is no second class count.  Same outputs, error codes, flags, workspace, records, launches, grid,
 * segment size and summation order: the results equal pvnet_head_metrics on the output of pvnet_vertex_targets_classes bit for bit.
 * num_classes beyond PVNET_CLASS_TARGETS_MAX_CLASSES is PVNET_E_BADARG, a table beyond PVNET_CLASS_TARGETS_MAX_TABLE
 * PVNET_E_UNSUPPORTED. */
int pvnet_head_metrics_ckp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                           const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                           int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                           double* losses, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

size_t pvnet_head_grad_ckp_workspace_bytes(int b, int h, int w);

/* pvnet_head_grad_kp with the same replacement: the gradients equal pvnet_head_grad on the output of pvnet_vertex_targets_classes
 * bit for bit.  A NULL gradient pointer skips that half (its stride array may be NULL then); the labels are read by either half. */
int pvnet_head_grad_ckp(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                        const int64_t vp_strides[4], const double* hcoords, const float* weight_scale, const void* mask,
                        int mask_dtype, const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags,
                        const double* upstream, void* grad_seg, const int64_t gs_strides[4], void* grad_vertex,
                        const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PVNET_CLASS_TARGETS_H */
