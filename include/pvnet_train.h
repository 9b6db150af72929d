/* pvnet_train.h -- C ABI of libpvnet_train.so: the backward of the network-head losses of a training step on the device.
 *
 * The loss is the reference's (tools/train_linemod.py:85-91, lib/utils/net_utils.py:54-79), the one pvnet_head_metrics
 * (include/pvnet_head.h) computes forward: per image the cross-entropy of seg_pred against the mask and the weighted smooth-L1 loss
 * of vertex_pred against the target field.  pvnet_head_grad writes their gradients with respect to the two predictions from the
 * forward's own inputs -- the gradient has a closed form per element, nothing of the forward is kept.
 *
 * A library of its own beside libpvnet_head.so and libpvnet_vote.so, whose ABIs it leaves alone.  It shares their error codes
 * (PVNET_E_BADARG, PVNET_E_WORKSPACE, PVNET_E_UNSUPPORTED), mask codes (PVNET_MASK_U8, PVNET_MASK_I32, PVNET_MASK_I64), the flags
 * PVNET_HEAD_F_* (element types of the predictions, which loads are non-temporal) and the status bit PVNET_HEAD_S_BAD_LABEL, by
 * value: no second family is defined here.
 *
 * The gradient, for image i with upstream gradients u_s = dL/dloss_seg[i] and u_v = dL/dloss_vertex[i], logits s, label m,
 * prediction p, target t, weight w:
 *
 *   logits   e_c = exp(s_c - max_c s), S = sum_c e_c (class order);
 *            d/ds_c = u_s / (h w) * (e_c / S)                    for c != m
 *            d/ds_m = -(u_s / (h w) * (sum_{j != m} e_j / S))    for the label's class: the others' share, NOT e_m / S - 1, which
 *            cancels once the label's logit leads by a margin of ~20.  A NaN logit makes the pixel's C gradients NaN (a NaN counts as
 *            the maximum, as in the forward).  A label outside 0 .. C-1 makes the pixel's C gradients NaN and sets
 *            PVNET_HEAD_S_BAD_LABEL in the image's status (the forward's loss_seg is NaN there).
 *   field    d = w (p - t), D_i = 2vn sum_pixels w + 1e-3 (the forward's denominator: weights only);
 *            d/dp = w (d sigma^2) * (u_v / D_i)   where |d| < 1 / sigma^2
 *            d/dp = w sign(d) * (u_v / D_i)       otherwise.
 *            IEEE semantics as written: w = 0 gives an exact zero, a NaN in d fails the comparison and gives a NaN.
 *
 * All arithmetic after the load is float64; each output element is rounded ONCE to the element type of the prediction it belongs to
 * (float32, float16 or bfloat16).  No atomics: two calls on the same inputs agree bit for bit.  Once-differentiable: there is no
 * gradient with respect to the targets, the weights or the mask, and no double backward.
 */
#ifndef PVNET_TRAIN_H
#define PVNET_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "pvnet_head.h"

#define PVNET_TRAIN_ABI_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

int pvnet_train_abi_version(void);

/* bytes of workspace a call with these sizes needs (0 for sizes the call rejects); the workspace may hold anything on entry */
size_t pvnet_head_grad_workspace_bytes(int b, int h, int w);

/* Enqueues the head gradients of b images on `stream`; allocates nothing, synchronises nothing.  Arguments are checked before any
 * HIP call.  All pointers but `stream` and the stride arrays are device pointers; strides are in elements.
 *
 *   seg_pred ... sigma   the forward's inputs, exactly as pvnet_head_metrics takes them (include/pvnet_head.h): read in place, any
 *                        strides, any base alignment
 *   flags                PVNET_HEAD_F_VERTEX_F16 / _BF16, PVNET_HEAD_F_LOGITS_F16 / _BF16: the element type of a prediction AND of
 *                        its gradient.  Measurement aids (tools/head_grad_probe.py): by default the targets, the weights and the
 *                        mask are loaded non-temporally, the predictions plainly and the gradients are stored plainly (the
 *                        backbone's backward reads them next); PVNET_HEAD_F_NT_NONE makes every access plain, PVNET_HEAD_F_NT_ALL
 *                        every load and every gradient store non-temporal.  The results do not depend on them.
 *   upstream             [b,2] float64, contiguous: u_s, u_v per image
 *   grad_seg             NULL or [b,C,h,w], the element type of seg_pred, strides gs_strides (its own: channels-last, or a channel
 *                        slice of a wider tensor)
 *   grad_vertex          NULL or [b,2vn,h,w], the element type of vertex_pred, strides gv_strides
 *   status               NULL or [b] int32: 0 or PVNET_HEAD_S_BAD_LABEL
 *
 * A NULL gradient pointer skips that half, its loads included (its stride array may be NULL then): without grad_seg the logits and
 * the mask are not read and status is 0; without grad_vertex the field, the targets and the weights are not read.  Both NULL is an
 * error.  Every element of a gradient tensor that is asked for is written.  Eight pixels per lane and 16 bytes per access where the
 * planes of every tensor of the half are contiguous in the pixels and 16-byte aligned and h * w is a multiple of 8; element by
 * element otherwise.  Up to four launches: the weights' sum per pixel segment (only with grad_vertex), the image's two coefficients,
 * the gradients, the status (only with status).
 *
 * Returns 0, PVNET_E_BADARG, PVNET_E_WORKSPACE, PVNET_E_UNSUPPORTED (b > 65535, h*w > 2^30, other mask types) or a hipError_t.
 * b == 0 returns 0 and enqueues nothing. */
int pvnet_head_grad(const void* seg_pred, const int64_t seg_strides[4], int num_classes, const void* vertex_pred,
                    const int64_t vp_strides[4], const float* vertex_target, const int64_t vt_strides[4], const float* vertex_weights,
                    const int64_t w_strides[3], const void* mask, int mask_dtype, const int64_t mask_strides[3], int b, int h, int w,
                    int vn, double sigma, uint32_t flags, const double* upstream, void* grad_seg, const int64_t gs_strides[4],
                    void* grad_vertex, const int64_t gv_strides[4], int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PVNET_TRAIN_H */
