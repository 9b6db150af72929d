/* pvnet_head.h -- C ABI of libpvnet_head.so: the network-head metrics of a validation step on the device.
 *
 * What the reference's NetWrapper.forward computes after the backbone (tools/train_linemod.py:85-91), for a batch in one call:
 * the per-image cross-entropy of seg_pred against the mask, the weighted smooth-L1 loss of vertex_pred against the target field
 * (lib/utils/net_utils.py:54-79) and the segmentation precision and recall (net_utils.py:329-348).  Two launches, no atomics; every
 * input byte is read once, all arithmetic after the load is float64, and the outputs are bitwise reproducible.
 *
 * A library of its own beside libpvnet_vote.so (whose ABI, include/pvnet_vote.h, it leaves alone).  It shares that header's error
 * codes (PVNET_E_BADARG, PVNET_E_WORKSPACE, PVNET_E_UNSUPPORTED) and mask codes (PVNET_MASK_U8, PVNET_MASK_I32, PVNET_MASK_I64).
 */
#ifndef PVNET_HEAD_H
#define PVNET_HEAD_H

#include <stddef.h>
#include <stdint.h>

#include "pvnet_vote.h"

#define PVNET_HEAD_ABI_VERSION 1

/* flags: the element type of the two predictions (float32 without a flag; read in place and widened on read) */
#define PVNET_HEAD_F_VERTEX_F16 1
#define PVNET_HEAD_F_VERTEX_BF16 2
#define PVNET_HEAD_F_LOGITS_F16 4
#define PVNET_HEAD_F_LOGITS_BF16 8
/* measurement aids (tools/head_metrics_probe.py): by default the targets, the weights and the mask -- read once, never again -- are
 * loaded non-temporally and the predictions, which the vote reads next, plainly.  NT_NONE loads everything plainly, NT_ALL
 * everything non-temporally.  The results do not depend on them. */
#define PVNET_HEAD_F_NT_NONE 16
#define PVNET_HEAD_F_NT_ALL 32

/* status bits (per image) */
#define PVNET_HEAD_S_BAD_LABEL 1 /* a mask value outside 0 .. num_classes-1: loss_seg of the image is NaN */

#ifdef __cplusplus
extern "C" {
#endif

int pvnet_head_abi_version(void);

/* bytes of workspace a call with these sizes needs (0 for sizes the call rejects); the workspace may hold anything on entry */
size_t pvnet_head_metrics_workspace_bytes(int b, int h, int w);

/* Enqueues the head metrics of b images on `stream`; allocates nothing, synchronises nothing.  Arguments are checked before any HIP
 * call.  All pointers but `stream` are device pointers; strides are in elements.
 *
 *   seg_pred       [b,C,h,w] class logits, C = num_classes >= 2, strides seg_strides (b, C, h, w)
 *   vertex_pred    [b,2vn,h,w] predicted field, strides vp_strides
 *   vertex_target  [b,2vn,h,w] float32 target field, strides vt_strides
 *   vertex_weights [b,1,h,w] float32, broadcast over the planes, strides w_strides (b, h, w)
 *   mask           [b,h,w] labels, mask_dtype PVNET_MASK_U8 / _I32 / _I64, strides mask_strides
 *   sigma          the smooth-L1 knee (the reference's default is 1): finite and > 0
 *   losses         [b,4] float64: loss_seg, loss_vertex, precision, recall
 *   counts         [b,3] int64: tp, fp, fn of (argmax_c seg_pred != 0) against (mask != 0)
 *   status         NULL or [b] int32: 0 or PVNET_HEAD_S_* bits
 *
 * loss_seg = mean over pixels of logsumexp_c(s) - s[mask] (the maximum subtracted first); loss_vertex = sum L(w (p - t)) /
 * (2vn sum w + 1e-3) with L(d) = d^2 sigma^2 / 2 where |d| < 1 / sigma^2, else |d| - 0.5 / sigma^2 (a NaN takes the second branch);
 * argmax as torch: the first maximum wins, a NaN counts as the maximum; precision = (tp+1)/(tp+fp+1), recall = (tp+1)/(tp+fn+1).
 * A pixel with a bad label counts as foreground.
 *
 * Returns 0, PVNET_E_BADARG, PVNET_E_WORKSPACE, PVNET_E_UNSUPPORTED (b > 65535, h*w > 2^30, other mask types) or a hipError_t.
 * b == 0 returns 0 and enqueues nothing. */
int pvnet_head_metrics(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                       const int64_t vp_strides[4], const float* vertex_target, const int64_t vt_strides[4],
                       const float* vertex_weights, const int64_t w_strides[3], const void* mask, int mask_dtype,
                       const int64_t mask_strides[3], int b, int h, int w, int vn, double sigma, uint32_t flags, double* losses,
                       int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PVNET_HEAD_H */
