"""The validation step behind the backbone, on the device (reference: tools/train_linemod.py:177-253).

* ``head_metrics_device`` / ``HeadMetrics`` -- what the reference's ``NetWrapper.forward`` computes after the two predictions
  (train_linemod.py:85-91): the per-image cross-entropy of ``seg_pred`` against the mask, the weighted smooth-L1 loss of
  ``vertex_pred`` (lib/utils/net_utils.py:54-79) and the segmentation precision and recall (net_utils.py:329-348), in ONE fused
  pass over the inputs (``pvnet_head_metrics``, pvnet_amd/csrc/head_metrics.hip, libpvnet_head.so; C ABI include/pvnet_head.h):
  every input byte is read once, in place, whatever its strides; float64 arithmetic; bitwise reproducible.
* ``head_grad_device`` / ``HeadLoss`` -- the same four lines as the loss of the reference's TRAINING loop (train_linemod.py:146-153):
  ``HeadLoss`` is ``HeadMetrics`` with a backward, ONE fused pass that reads the forward's inputs again and writes both gradients
  (``pvnet_head_grad``, pvnet_amd/csrc/head_grad.hip, libpvnet_train.so; C ABI and the formulas: include/pvnet_train.h).
* ``vertex_targets_device`` and the ``*_from_keypoints`` forms of all of the above -- the target field and its weights made on the
  device from the mask and the loader's ``hcoords`` (the reference's ``compute_vertex_hcoords``, lib/datasets/linemod_dataset.py:68-81,
  bit for bit), either written out or computed in registers inside the head's forward and backward, which then never read a target
  (pvnet_amd/csrc/head_targets.hip, libpvnet_targets.so; C ABI and the definition: include/pvnet_targets.h).
* ``vertex_targets_classes_device`` and the ``*_from_class_keypoints`` forms -- the same for images of several objects: the key-points
  of a pixel are picked by its label (pvnet_amd/csrc/class_targets.hip, libpvnet_class_targets.so; the definition:
  include/pvnet_class_targets.h).
* ``ValStep`` -- the whole step on the current stream: head metrics, then ``voting.PoseEvalWrapper`` (fused arg-max voting and the
  pose solve), then the pose metrics ``Evaluator.evaluate_batch`` records (``evaluation.pose_metrics_device``); one host copy at the
  end.  ``enqueue`` is the part a graph captures.

PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import torch

from ._abi import (HEAD_F_LOGITS_BF16, HEAD_F_LOGITS_F16, HEAD_F_NT_ALL, HEAD_F_NT_NONE, HEAD_F_VERTEX_BF16,  # noqa: F401
                   HEAD_F_VERTEX_F16, HEAD_S_BAD_LABEL, MASK_I32, MASK_I64, MASK_U8, TARGETS_F_MOTION, CLASS_TARGETS_MAX_CLASSES,
                   CLASS_TARGETS_MAX_TABLE, _check, load_class_targets_library, load_head_library, load_targets_library,
                   load_train_library)
from ._marshal import nbytes as _nbytes, opt_strides as _opt_strides, ptr as _ptr, stream as _stream, strides as _strides, \
    workspace as _workspace

_VERTEX_FLAGS = {torch.float32: 0, torch.float16: HEAD_F_VERTEX_F16, torch.bfloat16: HEAD_F_VERTEX_BF16}
_LOGITS_FLAGS = {torch.float32: 0, torch.float16: HEAD_F_LOGITS_F16, torch.bfloat16: HEAD_F_LOGITS_BF16}
_MASK_CODES = {torch.uint8: MASK_U8, torch.bool: MASK_U8, torch.int32: MASK_I32, torch.int64: MASK_I64}


def _head_inputs(seg_pred, vertex_pred, mask, vertex, vertex_weights, flags):
    """the checks ``head_metrics_device`` and ``head_grad_device`` share -> (device, b, C, h, w, 2vn, flags with the element types)"""
    tensors = (("seg_pred", seg_pred), ("vertex_pred", vertex_pred), ("mask", mask), ("vertex", vertex),
               ("vertex_weights", vertex_weights))
    for name, t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name} must be a CUDA tensor (there is no CPU fallback)")
    dev = seg_pred.device
    if any(t.device != dev for _, t in tensors):
        raise RuntimeError("seg_pred, vertex_pred, mask, vertex and vertex_weights must live on the same device")
    if seg_pred.dim() != 4 or seg_pred.shape[1] < 2:
        raise RuntimeError(f"seg_pred must be [b,C,h,w] with C >= 2, got {tuple(seg_pred.shape)}")
    b, nc, h, w = (int(x) for x in seg_pred.shape)
    if vertex_pred.dim() != 4 or vertex_pred.shape[1] % 2 or vertex_pred.shape[1] == 0 or \
            (vertex_pred.shape[0], vertex_pred.shape[2], vertex_pred.shape[3]) != (b, h, w):
        raise RuntimeError(f"vertex_pred must be [b,2vn,h,w] with (b,h,w)={(b, h, w)}, got {tuple(vertex_pred.shape)}")
    planes = int(vertex_pred.shape[1])
    if tuple(vertex.shape) != (b, planes, h, w):
        raise RuntimeError(f"vertex must be [b,2vn,h,w]={(b, planes, h, w)}, got {tuple(vertex.shape)}")
    if tuple(vertex_weights.shape) != (b, 1, h, w):
        raise RuntimeError(f"vertex_weights must be [b,1,h,w]={(b, 1, h, w)}, got {tuple(vertex_weights.shape)}")
    if tuple(mask.shape) != (b, h, w):
        raise RuntimeError(f"mask must be [b,h,w]={(b, h, w)}, got {tuple(mask.shape)}")
    if seg_pred.dtype not in _LOGITS_FLAGS or vertex_pred.dtype not in _VERTEX_FLAGS:
        raise RuntimeError("seg_pred and vertex_pred must be float32, float16 or bfloat16")
    if vertex.dtype != torch.float32 or vertex_weights.dtype != torch.float32:
        raise RuntimeError("vertex and vertex_weights must be float32")
    if mask.dtype not in _MASK_CODES:
        raise RuntimeError("mask must be uint8, bool, int32 or int64")
    flags = int(flags) | _LOGITS_FLAGS[seg_pred.dtype] | _VERTEX_FLAGS[vertex_pred.dtype]
    return dev, b, nc, h, w, planes, flags


def _metric_outputs(out, b, dev):
    """``(losses [b,4] float64, counts [b,3] int64, status [b] int32)``: new, or the caller's ``out`` checked"""
    if out is None:
        return (torch.empty((b, 4), dtype=torch.float64, device=dev), torch.empty((b, 3), dtype=torch.int64, device=dev),
                torch.empty((b,), dtype=torch.int32, device=dev))
    losses, counts, status = out
    for t, dt, shape, name in ((losses, torch.float64, (b, 4), "out[0]"), (counts, torch.int64, (b, 3), "out[1]"),
                               (status, torch.int32, (b,), "out[2]")):
        if not (t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError(f"{name} must be a contiguous {dt} CUDA tensor of shape {shape} on {dev}")
    return losses, counts, status


def _grad_outputs(seg_pred, vertex_pred, upstream, need, out, b, dev):
    """the checks of ``upstream``, ``need`` and ``out`` -> (grad_seg, grad_vertex, status): new tensors or the caller's, None for a
    half that is not wanted"""
    need = (bool(need[0]), bool(need[1]))
    if not any(need):
        raise RuntimeError("need: at least one of the two gradients must be wanted")
    if not (isinstance(upstream, torch.Tensor) and upstream.is_cuda):
        raise RuntimeError("upstream must be a CUDA tensor (there is no CPU fallback)")
    if not (upstream.device == dev and upstream.dtype == torch.float64 and tuple(upstream.shape) == (b, 2) and upstream.is_contiguous()):
        raise RuntimeError(f"upstream must be a contiguous float64 CUDA tensor of shape {(b, 2)} on {dev}")
    grads = []
    for k, (pred, name) in enumerate(((seg_pred, "out[0]"), (vertex_pred, "out[1]"))):
        g = None if out is None else out[k]
        if not need[k]:
            g = None
        elif g is None:
            g = torch.empty_like(pred)
        elif not (isinstance(g, torch.Tensor) and g.is_cuda and g.device == dev and g.dtype == pred.dtype and g.shape == pred.shape):
            raise RuntimeError(f"{name} must be a {pred.dtype} CUDA tensor of shape {tuple(pred.shape)} on {dev}")
        grads.append(g)
    return grads[0], grads[1], torch.empty((b,), dtype=torch.int32, device=dev)


def head_metrics_workspace_bytes(b, h, w):
    """the workspace ``head_metrics_device`` needs for b images of h x w pixels (bytes)"""
    return int(load_head_library().pvnet_head_metrics_workspace_bytes(int(b), int(h), int(w)))


def head_metrics_device(seg_pred, vertex_pred, mask, vertex, vertex_weights, sigma=1.0, out=None, workspace=None, flags=0):
    """The head metrics of a batch, enqueued on the current stream -- no synchronisation, no host copy.

    :param seg_pred:       [b,C,h,w] class logits, float32 / float16 / bfloat16 CUDA tensor, any strides (read in place)
    :param vertex_pred:    [b,2vn,h,w] predicted field, float32 / float16 / bfloat16, any strides (read in place)
    :param mask:           [b,h,w] labels, uint8 / bool / int32 / int64, any strides
    :param vertex:         [b,2vn,h,w] float32 target field, any strides
    :param vertex_weights: [b,1,h,w] float32 weights, any strides
    :param sigma:          the smooth-L1 knee (``smooth_l1_loss``'s default 1)
    :param out:            None, or caller-owned contiguous ``(losses [b,4] float64, counts [b,3] int64, status [b] int32)``
    :param workspace:      None, or a caller-owned uint8 CUDA tensor of at least ``head_metrics_workspace_bytes`` bytes
    :param flags:          ``HEAD_F_NT_NONE`` / ``HEAD_F_NT_ALL`` (measurement aids; the results do not depend on them)
    :return: ``(losses, counts, status)`` on the device: losses = (loss_seg, loss_vertex, precision, recall) per image, counts =
             (tp, fp, fn), status 0 or ``HEAD_S_BAD_LABEL`` (a label outside 0..C-1: that image's loss_seg is NaN)."""
    lib = load_head_library()
    dev, b, nc, h, w, planes, flags = _head_inputs(seg_pred, vertex_pred, mask, vertex, vertex_weights, flags)
    with torch.cuda.device(dev):
        losses, counts, status = _metric_outputs(out, b, dev)
        if b == 0:
            return losses, counts, status
        ws = _workspace(workspace, lib.pvnet_head_metrics_workspace_bytes(b, h, w), dev)
        _check(lib.pvnet_head_metrics(
            _ptr(seg_pred), _strides(seg_pred, (0, 1, 2, 3)), nc,
            _ptr(vertex_pred), _strides(vertex_pred, (0, 1, 2, 3)),
            _ptr(vertex), _strides(vertex, (0, 1, 2, 3)),
            _ptr(vertex_weights), _strides(vertex_weights, (0, 2, 3)),
            _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)),
            b, h, w, planes // 2, float(sigma), flags,
            _ptr(losses), _ptr(counts), _ptr(status),
            _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_head_metrics")
    return losses, counts, status


class HeadMetrics(torch.nn.Module):
    """What the reference's ``NetWrapper.forward`` returns after the two predictions (tools/train_linemod.py:87-91):
    ``forward(seg_pred, vertex_pred, mask, vertex, vertex_weights) -> (loss_seg, loss_vertex, precision, recall)``, float32 [b]
    each -- the float64 results of ``head_metrics_device`` rounded once.  Validation only: nothing here is differentiable."""

    def __init__(self, sigma=1.0):
        super().__init__()
        self.sigma = float(sigma)

    def forward(self, seg_pred, vertex_pred, mask, vertex, vertex_weights):
        losses, _, _ = head_metrics_device(seg_pred, vertex_pred, mask, vertex, vertex_weights, sigma=self.sigma)
        return tuple(losses.to(torch.float32).unbind(1))

    def from_keypoints(self, seg_pred, vertex_pred, mask, hcoords, weight_scale=None, use_motion=False):
        """the same four values from the loader's ``hcoords`` instead of the target field (``head_metrics_from_keypoints``)"""
        losses, _, _ = head_metrics_from_keypoints(seg_pred, vertex_pred, mask, hcoords, weight_scale, sigma=self.sigma,
                                                   use_motion=use_motion)
        return tuple(losses.to(torch.float32).unbind(1))

    def from_class_keypoints(self, seg_pred, vertex_pred, labels, hcoords, weight_scale=None, use_motion=False):
        """the same four values from a label image and key-points per class (``head_metrics_from_class_keypoints``)"""
        losses, _, _ = head_metrics_from_class_keypoints(seg_pred, vertex_pred, labels, hcoords, weight_scale, sigma=self.sigma,
                                                         use_motion=use_motion)
        return tuple(losses.to(torch.float32).unbind(1))


def head_grad_workspace_bytes(b, h, w):
    """the workspace ``head_grad_device`` needs for b images of h x w pixels (bytes)"""
    return int(load_train_library().pvnet_head_grad_workspace_bytes(int(b), int(h), int(w)))


def head_grad_device(seg_pred, vertex_pred, mask, vertex, vertex_weights, upstream, sigma=1.0, need=(True, True), out=None,
                     workspace=None, flags=0):
    """The gradients of the two head losses with respect to the two predictions, enqueued on the current stream -- no
    synchronisation, no host copy, nothing saved from a forward (the formulas: include/pvnet_train.h).

    The first five arguments and ``sigma`` are those of ``head_metrics_device``, read in place.

    :param upstream:  [b,2] float64 contiguous CUDA tensor: dL/dloss_seg and dL/dloss_vertex per image
    :param need:      ``(grad_seg wanted, grad_vertex wanted)``; a half that is not wanted is skipped, its loads included
    :param out:       None, or caller-owned ``(grad_seg, grad_vertex)`` (``None`` for a half that is not wanted): the shape, dtype and
                      device of their prediction, ANY strides -- channels-last, or channel slices of one wider tensor
    :param workspace: None, or a caller-owned uint8 CUDA tensor of at least ``head_grad_workspace_bytes`` bytes
    :param flags:     ``HEAD_F_NT_NONE`` / ``HEAD_F_NT_ALL`` (measurement aids; the results do not depend on them)
    :return: ``(grad_seg, grad_vertex, status)``: each gradient in its prediction's dtype (``torch.empty_like`` unless ``out`` is
             given), None for a half that is not wanted; status [b] int32, 0 or ``HEAD_S_BAD_LABEL`` (a label outside 0..C-1: that
             pixel's C gradients are NaN; 0 when grad_seg is not wanted -- the mask is not read then)."""
    lib = load_train_library()
    dev, b, nc, h, w, planes, flags = _head_inputs(seg_pred, vertex_pred, mask, vertex, vertex_weights, flags)
    with torch.cuda.device(dev):
        grad_seg, grad_vertex, status = _grad_outputs(seg_pred, vertex_pred, upstream, need, out, b, dev)
        if b == 0:
            return grad_seg, grad_vertex, status
        ws = _workspace(workspace, lib.pvnet_head_grad_workspace_bytes(b, h, w), dev)
        _check(lib.pvnet_head_grad(
            _ptr(seg_pred), _strides(seg_pred, (0, 1, 2, 3)), nc,
            _ptr(vertex_pred), _strides(vertex_pred, (0, 1, 2, 3)),
            _ptr(vertex), _strides(vertex, (0, 1, 2, 3)),
            _ptr(vertex_weights), _strides(vertex_weights, (0, 2, 3)),
            _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)),
            b, h, w, planes // 2, float(sigma), flags, _ptr(upstream),
            _ptr(grad_seg), _opt_strides(grad_seg, (0, 1, 2, 3)), _ptr(grad_vertex), _opt_strides(grad_vertex, (0, 1, 2, 3)),
            _ptr(status), _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_head_grad")
    return grad_seg, grad_vertex, status


# ---- the targets from the key-points (libpvnet_targets.so) ---------------------------------------------------------------------------
def _keypoint_inputs(mask, hcoords, weight_scale):
    """the checks the key-point entries share -> (device, b, h, w, vn, hcoords [b,vn,3] float64 contiguous, weight_scale or None)"""
    for name, t in (("mask", mask), ("hcoords", hcoords)) + ((("weight_scale", weight_scale),) if weight_scale is not None else ()):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name} must be a CUDA tensor (there is no CPU fallback)")
    dev = mask.device
    if mask.dim() != 3 or mask.dtype not in _MASK_CODES:
        raise RuntimeError(f"mask must be [b,h,w], uint8, bool, int32 or int64, got {tuple(mask.shape)} {mask.dtype}")
    b, h, w = (int(x) for x in mask.shape)
    if hcoords.device != dev or hcoords.dim() != 3 or hcoords.shape[0] != b or hcoords.shape[1] < 1 or hcoords.shape[2] not in (2, 3) or \
            hcoords.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"hcoords must be [b,vn,3] (or [b,vn,2]: hz = 1) float32 or float64 on {dev} with b={b}, got "
                           f"{tuple(hcoords.shape)} {hcoords.dtype}")
    hc = hcoords.to(torch.float64)   # (float32 widens exactly: the reference's numpy computes in float64 whatever arrives)
    if hc.shape[2] == 2:
        hc = torch.cat([hc, torch.ones_like(hc[:, :, :1])], 2)
    hc = hc.contiguous()
    if weight_scale is not None:
        if weight_scale.device != dev or tuple(weight_scale.shape) != (b,) or not weight_scale.dtype.is_floating_point:
            raise RuntimeError(f"weight_scale must be a floating-point tensor of shape {(b,)} on {dev}")
        weight_scale = weight_scale.to(torch.float32).contiguous()
    return dev, b, h, w, int(hc.shape[1]), hc, weight_scale


def vertex_targets_device(mask, hcoords, weight_scale=None, use_motion=False, out=None):
    """The reference's ``compute_vertex_hcoords`` (lib/datasets/linemod_dataset.py:68-81) and ``mask.float()`` weights (:227) for a
    batch, enqueued on the current stream -- no synchronisation, no host copy.  Bit for bit what the reference's numpy computes.

    :param mask:         [b,h,w] uint8 / bool / int32 / int64 CUDA tensor, any strides.  Target pixels are ``mask == 1``
    :param hcoords:      [b,vn,3] homogeneous 2-D key-points as the loader returns them (float64, or float32 which widens exactly);
                         [b,vn,2] is taken as hz = 1 (tools/demo.py:58-71)
    :param weight_scale: None (1), or [b]: a factor on an image's weights (the reference's ``ver_weight *= 0.0`` of its "fuse" images)
    :param use_motion:   the reference's ``use_motion=True``: the targets are not normalised
    :param out:          None, or caller-owned float32 ``(vertex [b,2vn,h,w], vertex_weights [b,1,h,w])``, ANY strides; either may be
                         ``None`` to skip that output
    :return: ``(vertex, vertex_weights)``: plane 2k of ``vertex`` is x and plane 2k+1 is y of key-point k, zero off ``mask == 1``;
             the weight of a pixel is its mask VALUE times the image's scale."""
    lib = load_targets_library()
    dev, b, h, w, vn, hc, weight_scale = _keypoint_inputs(mask, hcoords, weight_scale)
    with torch.cuda.device(dev):
        if out is None:
            vertex = torch.empty((b, 2 * vn, h, w), dtype=torch.float32, device=dev)
            weights = torch.empty((b, 1, h, w), dtype=torch.float32, device=dev)
        else:
            vertex, weights = out
            for t, shape, name in ((vertex, (b, 2 * vn, h, w), "out[0]"), (weights, (b, 1, h, w), "out[1]")):
                if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and
                                          tuple(t.shape) == shape):
                    raise RuntimeError(f"{name} must be a float32 CUDA tensor of shape {shape} on {dev}")
            if vertex is None and weights is None:
                raise RuntimeError("out: at least one of the two outputs must be asked for")
        if b == 0:
            return vertex, weights
        _check(lib.pvnet_vertex_targets(
            _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)), _ptr(hc),
            _ptr(weight_scale), b, h, w, vn, TARGETS_F_MOTION if use_motion else 0,
            _ptr(vertex), _opt_strides(vertex, (0, 1, 2, 3)), _ptr(weights), _opt_strides(weights, (0, 2, 3)),
            _stream(dev)), "pvnet_vertex_targets")
    return vertex, weights


def _kp_head_inputs(seg_pred, vertex_pred, mask, hcoords, weight_scale, flags, use_motion):
    """the checks ``head_metrics_from_keypoints`` and ``head_grad_from_keypoints`` share"""
    for name, t in (("seg_pred", seg_pred), ("vertex_pred", vertex_pred)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name} must be a CUDA tensor (there is no CPU fallback)")
    dev, b, h, w, vn, hc, weight_scale = _keypoint_inputs(mask, hcoords, weight_scale)
    if seg_pred.device != dev or vertex_pred.device != dev:
        raise RuntimeError("seg_pred, vertex_pred, mask and hcoords must live on the same device")
    if seg_pred.dim() != 4 or seg_pred.shape[1] < 2 or (seg_pred.shape[0], seg_pred.shape[2], seg_pred.shape[3]) != (b, h, w):
        raise RuntimeError(f"seg_pred must be [b,C,h,w] with C >= 2 and (b,h,w)={(b, h, w)}, got {tuple(seg_pred.shape)}")
    if tuple(vertex_pred.shape) != (b, 2 * vn, h, w):
        raise RuntimeError(f"vertex_pred must be [b,2vn,h,w]={(b, 2 * vn, h, w)}, got {tuple(vertex_pred.shape)}")
    if seg_pred.dtype not in _LOGITS_FLAGS or vertex_pred.dtype not in _VERTEX_FLAGS:
        raise RuntimeError("seg_pred and vertex_pred must be float32, float16 or bfloat16")
    flags = int(flags) | _LOGITS_FLAGS[seg_pred.dtype] | _VERTEX_FLAGS[vertex_pred.dtype] | (TARGETS_F_MOTION if use_motion else 0)
    return dev, b, int(seg_pred.shape[1]), h, w, vn, hc, weight_scale, flags


def head_metrics_from_keypoints(seg_pred, vertex_pred, mask, hcoords, weight_scale=None, sigma=1.0, use_motion=False, out=None,
                                workspace=None, flags=0):
    """``head_metrics_device`` on the targets of ``vertex_targets_device(mask, hcoords, weight_scale, use_motion)`` without making
    them: the target and the weight of a pixel are computed in registers.  Same ``(losses, counts, status)``, bit for bit; the other
    parameters are those of ``head_metrics_device``."""
    lib = load_targets_library()
    dev, b, nc, h, w, vn, hc, weight_scale, flags = _kp_head_inputs(seg_pred, vertex_pred, mask, hcoords, weight_scale, flags, use_motion)
    with torch.cuda.device(dev):
        losses, counts, status = _metric_outputs(out, b, dev)
        if b == 0:
            return losses, counts, status
        ws = _workspace(workspace, lib.pvnet_head_metrics_kp_workspace_bytes(b, h, w), dev)
        _check(lib.pvnet_head_metrics_kp(
            _ptr(seg_pred), _strides(seg_pred, (0, 1, 2, 3)), nc,
            _ptr(vertex_pred), _strides(vertex_pred, (0, 1, 2, 3)),
            _ptr(hc), _ptr(weight_scale),
            _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)),
            b, h, w, vn, float(sigma), flags,
            _ptr(losses), _ptr(counts), _ptr(status),
            _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_head_metrics_kp")
    return losses, counts, status


def head_grad_from_keypoints(seg_pred, vertex_pred, mask, hcoords, upstream, weight_scale=None, sigma=1.0, use_motion=False,
                             need=(True, True), out=None, workspace=None, flags=0):
    """``head_grad_device`` on the targets of ``vertex_targets_device(mask, hcoords, weight_scale, use_motion)`` without making them.
    Same ``(grad_seg, grad_vertex, status)``, bit for bit; ``upstream``, ``need``, ``out``, ``workspace`` and ``flags`` as there."""
    lib = load_targets_library()
    dev, b, nc, h, w, vn, hc, weight_scale, flags = _kp_head_inputs(seg_pred, vertex_pred, mask, hcoords, weight_scale, flags, use_motion)
    with torch.cuda.device(dev):
        grad_seg, grad_vertex, status = _grad_outputs(seg_pred, vertex_pred, upstream, need, out, b, dev)
        if b == 0:
            return grad_seg, grad_vertex, status
        ws = _workspace(workspace, lib.pvnet_head_grad_kp_workspace_bytes(b, h, w), dev)
        _check(lib.pvnet_head_grad_kp(
            _ptr(seg_pred), _strides(seg_pred, (0, 1, 2, 3)), nc,
            _ptr(vertex_pred), _strides(vertex_pred, (0, 1, 2, 3)),
            _ptr(hc), _ptr(weight_scale),
            _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)),
            b, h, w, vn, float(sigma), flags, _ptr(upstream),
            _ptr(grad_seg), _opt_strides(grad_seg, (0, 1, 2, 3)), _ptr(grad_vertex), _opt_strides(grad_vertex, (0, 1, 2, 3)),
            _ptr(status), _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_head_grad_kp")
    return grad_seg, grad_vertex, status


# ---- the targets of several objects: a label image and key-points per class (libpvnet_class_targets.so) ------------------------------
def _class_keypoint_inputs(labels, hcoords, weight_scale, class_num=None):
    """the checks the class key-point entries share -> (device, b, h, w, class_num, vn, hcoords [b,C-1,vn,3] float64 contiguous,
    weight_scale [b,C-1] float32 or None).  ``class_num``: what the logits say C is, where there are logits."""
    for name, t in (("labels", labels), ("hcoords", hcoords)) + ((("weight_scale", weight_scale),) if weight_scale is not None else ()):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name} must be a CUDA tensor (there is no CPU fallback)")
    dev = labels.device
    if labels.dim() != 3 or labels.dtype not in _MASK_CODES:
        raise RuntimeError(f"labels must be [b,h,w], uint8, bool, int32 or int64, got {tuple(labels.shape)} {labels.dtype}")
    b, h, w = (int(x) for x in labels.shape)
    want = "[b,C-1,vn,3]" if class_num is None else f"[b,C-1,vn,3] with C-1={class_num - 1}"
    if hcoords.device != dev or hcoords.dim() != 4 or hcoords.shape[0] != b or hcoords.shape[1] < 1 or hcoords.shape[2] < 1 or \
            hcoords.shape[3] not in (2, 3) or hcoords.dtype not in (torch.float32, torch.float64) or \
            (class_num is not None and hcoords.shape[1] != class_num - 1):
        raise RuntimeError(f"hcoords must be {want} (or [b,C-1,vn,2]: hz = 1) float32 or float64 on {dev} with b={b}: row k holds the "
                           f"key-points of class k + 1; got {tuple(hcoords.shape)} {hcoords.dtype}")
    nk, vn = int(hcoords.shape[1]), int(hcoords.shape[2])
    if nk + 1 > CLASS_TARGETS_MAX_CLASSES or nk * vn > CLASS_TARGETS_MAX_TABLE:
        raise RuntimeError(f"hcoords [b,C-1,vn,3]: at most {CLASS_TARGETS_MAX_CLASSES} classes (the background counted) and "
                           f"(C-1) * vn <= {CLASS_TARGETS_MAX_TABLE}, got C-1={nk}, vn={vn}")
    hc = hcoords.to(torch.float64)   # (float32 widens exactly)
    if hc.shape[3] == 2:
        hc = torch.cat([hc, torch.ones_like(hc[..., :1])], 3)
    hc = hc.contiguous()
    if weight_scale is not None:
        if weight_scale.device != dev or tuple(weight_scale.shape) not in ((b,), (b, nk)) or not weight_scale.dtype.is_floating_point:
            raise RuntimeError(f"weight_scale must be a floating-point tensor of shape {(b,)} or [b,C-1]={(b, nk)} on {dev}")
        weight_scale = weight_scale.to(torch.float32)
        if weight_scale.dim() == 1:
            weight_scale = weight_scale[:, None].expand(b, nk)   # one factor per image, for every class
        weight_scale = weight_scale.contiguous()
    return dev, b, h, w, nk + 1, vn, hc, weight_scale


def vertex_targets_classes_device(labels, hcoords, weight_scale=None, use_motion=False, out=None):
    """``vertex_targets_device`` for images of several objects: the key-points of a pixel are picked by its label, in ONE launch
    (include/pvnet_class_targets.h states the definition).  Enqueued on the current stream -- no synchronisation, no host copy.

    :param labels:       [b,h,w] uint8 / bool / int32 / int64 CUDA tensor, any strides: 0 is the background, k + 1 the class of row k
    :param hcoords:      [b,C-1,vn,3] homogeneous 2-D key-points per class (float64, or float32 which widens exactly); [b,C-1,vn,2] is
                         taken as hz = 1.  C, the class count with the background, is at most 64 and (C-1) * vn at most 1024
    :param weight_scale: None (1), [b] (one factor per image) or [b,C-1] (one per image and class)
    :param use_motion:   the targets are not normalised
    :param out:          None, or caller-owned float32 ``(vertex [b,2vn,h,w], vertex_weights [b,1,h,w])``, ANY strides; either may be
                         ``None`` to skip that output
    :return: ``(vertex, vertex_weights)``.  On the pixels of label k + 1 both equal, bit for bit, what ``vertex_targets_device`` gives
             for the binary mask ``labels == k + 1`` and ``hcoords[:, k]``; every other pixel (label 0, negative, >= C) has targets
             +0 and weight 0 -- a selection by label, not a sum over the classes.  With C = 2 on a 0/1 mask that is
             ``vertex_targets_device`` itself; a mask VALUE of 2 weighs 0 here and 2 there, the one deliberate difference."""
    lib = load_class_targets_library()
    dev, b, h, w, class_num, vn, hc, weight_scale = _class_keypoint_inputs(labels, hcoords, weight_scale)
    with torch.cuda.device(dev):
        if out is None:
            vertex = torch.empty((b, 2 * vn, h, w), dtype=torch.float32, device=dev)
            weights = torch.empty((b, 1, h, w), dtype=torch.float32, device=dev)
        else:
            vertex, weights = out
            for t, shape, name in ((vertex, (b, 2 * vn, h, w), "out[0]"), (weights, (b, 1, h, w), "out[1]")):
                if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and
                                          tuple(t.shape) == shape):
                    raise RuntimeError(f"{name} must be a float32 CUDA tensor of shape {shape} on {dev}")
            if vertex is None and weights is None:
                raise RuntimeError("out: at least one of the two outputs must be asked for")
        if b == 0:
            return vertex, weights
        _check(lib.pvnet_vertex_targets_classes(
            _ptr(labels), _MASK_CODES[labels.dtype], _strides(labels, (0, 1, 2)), _ptr(hc),
            _ptr(weight_scale), class_num, b, h, w, vn, TARGETS_F_MOTION if use_motion else 0,
            _ptr(vertex), _opt_strides(vertex, (0, 1, 2, 3)), _ptr(weights), _opt_strides(weights, (0, 2, 3)),
            _stream(dev)), "pvnet_vertex_targets_classes")
    return vertex, weights


def _ckp_head_inputs(seg_pred, vertex_pred, labels, hcoords, weight_scale, flags, use_motion):
    """the checks ``head_metrics_from_class_keypoints`` and ``head_grad_from_class_keypoints`` share"""
    for name, t in (("seg_pred", seg_pred), ("vertex_pred", vertex_pred)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name} must be a CUDA tensor (there is no CPU fallback)")
    if seg_pred.dim() != 4 or seg_pred.shape[1] < 2:
        raise RuntimeError(f"seg_pred must be [b,C,h,w] with C >= 2, got {tuple(seg_pred.shape)}")
    dev, b, h, w, nc, vn, hc, weight_scale = _class_keypoint_inputs(labels, hcoords, weight_scale, class_num=int(seg_pred.shape[1]))
    if seg_pred.device != dev or vertex_pred.device != dev:
        raise RuntimeError("seg_pred, vertex_pred, labels and hcoords must live on the same device")
    if (seg_pred.shape[0], seg_pred.shape[2], seg_pred.shape[3]) != (b, h, w):
        raise RuntimeError(f"seg_pred must be [b,C,h,w] with (b,h,w)={(b, h, w)}, got {tuple(seg_pred.shape)}")
    if tuple(vertex_pred.shape) != (b, 2 * vn, h, w):
        raise RuntimeError(f"vertex_pred must be [b,2vn,h,w]={(b, 2 * vn, h, w)}, got {tuple(vertex_pred.shape)}")
    if seg_pred.dtype not in _LOGITS_FLAGS or vertex_pred.dtype not in _VERTEX_FLAGS:
        raise RuntimeError("seg_pred and vertex_pred must be float32, float16 or bfloat16")
    flags = int(flags) | _LOGITS_FLAGS[seg_pred.dtype] | _VERTEX_FLAGS[vertex_pred.dtype] | (TARGETS_F_MOTION if use_motion else 0)
    return dev, b, nc, h, w, vn, hc, weight_scale, flags


def head_metrics_from_class_keypoints(seg_pred, vertex_pred, labels, hcoords, weight_scale=None, sigma=1.0, use_motion=False, out=None,
                                      workspace=None, flags=0):
    """``head_metrics_device`` on the targets of ``vertex_targets_classes_device(labels, hcoords, weight_scale, use_motion)`` without
    making them.  ``seg_pred`` is [b,C,h,w] and ``hcoords`` [b,C-1,vn,3]: the logits' class count is the targets'.  Same ``(losses,
    counts, status)``, bit for bit; the other parameters are those of ``head_metrics_device``."""
    lib = load_class_targets_library()
    dev, b, nc, h, w, vn, hc, weight_scale, flags = _ckp_head_inputs(seg_pred, vertex_pred, labels, hcoords, weight_scale, flags, use_motion)
    with torch.cuda.device(dev):
        losses, counts, status = _metric_outputs(out, b, dev)
        if b == 0:
            return losses, counts, status
        ws = _workspace(workspace, lib.pvnet_head_metrics_ckp_workspace_bytes(b, h, w), dev)
        _check(lib.pvnet_head_metrics_ckp(
            _ptr(seg_pred), _strides(seg_pred, (0, 1, 2, 3)), nc,
            _ptr(vertex_pred), _strides(vertex_pred, (0, 1, 2, 3)),
            _ptr(hc), _ptr(weight_scale),
            _ptr(labels), _MASK_CODES[labels.dtype], _strides(labels, (0, 1, 2)),
            b, h, w, vn, float(sigma), flags,
            _ptr(losses), _ptr(counts), _ptr(status),
            _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_head_metrics_ckp")
    return losses, counts, status


def head_grad_from_class_keypoints(seg_pred, vertex_pred, labels, hcoords, upstream, weight_scale=None, sigma=1.0, use_motion=False,
                                   need=(True, True), out=None, workspace=None, flags=0):
    """``head_grad_device`` on the targets of ``vertex_targets_classes_device(labels, hcoords, weight_scale, use_motion)`` without
    making them.  Same ``(grad_seg, grad_vertex, status)``, bit for bit; ``upstream``, ``need``, ``out``, ``workspace`` and ``flags`` as
    there."""
    lib = load_class_targets_library()
    dev, b, nc, h, w, vn, hc, weight_scale, flags = _ckp_head_inputs(seg_pred, vertex_pred, labels, hcoords, weight_scale, flags, use_motion)
    with torch.cuda.device(dev):
        grad_seg, grad_vertex, status = _grad_outputs(seg_pred, vertex_pred, upstream, need, out, b, dev)
        if b == 0:
            return grad_seg, grad_vertex, status
        ws = _workspace(workspace, lib.pvnet_head_grad_ckp_workspace_bytes(b, h, w), dev)
        _check(lib.pvnet_head_grad_ckp(
            _ptr(seg_pred), _strides(seg_pred, (0, 1, 2, 3)), nc,
            _ptr(vertex_pred), _strides(vertex_pred, (0, 1, 2, 3)),
            _ptr(hc), _ptr(weight_scale),
            _ptr(labels), _MASK_CODES[labels.dtype], _strides(labels, (0, 1, 2)),
            b, h, w, vn, float(sigma), flags, _ptr(upstream),
            _ptr(grad_seg), _opt_strides(grad_seg, (0, 1, 2, 3)), _ptr(grad_vertex), _opt_strides(grad_vertex, (0, 1, 2, 3)),
            _ptr(status), _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_head_grad_ckp")
    return grad_seg, grad_vertex, status


def _upstream(grad_seg_loss, grad_vertex_loss, b, dev):
    """[b,2] float64 from the two incoming gradients of a backward; a missing one is zeros"""
    cols = [torch.zeros((b,), dtype=torch.float64, device=dev) if g is None else g.to(torch.float64) for g in (grad_seg_loss, grad_vertex_loss)]
    return torch.stack(cols, 1)


_CLASS_KEYPOINTS = 2   # ``keypoints`` of ``_HeadLossFn``: the third target source (False: loaded targets, True: key-points per image)


class _HeadLossFn(torch.autograd.Function):
    """The six forms of ``HeadLoss``.  ``apply(pred, pred2, seg_dim, mask, source, source2, sigma, use_motion, keypoints)``:

    * the predictions are ``(pred, pred2) = (seg_pred, vertex_pred)`` with ``seg_dim`` None, or the two channel slices of the ONE tensor
      ``pred`` at ``seg_dim`` (``pred2`` None): the backward then writes both halves into one gradient tensor of its shape;
    * the targets are ``(source, source2) = (vertex, vertex_weights)``, or with ``keypoints`` ``(hcoords, weight_scale or None)``:
      ``True`` for one set per image, ``_CLASS_KEYPOINTS`` for one per class, picked by the label (``mask`` is a label image then).

    forward: ``head_metrics_device`` / ``head_metrics_from_keypoints`` / ``head_metrics_from_class_keypoints``; backward: ONE
    ``head_grad_device`` / ``head_grad_from_keypoints`` / ``head_grad_from_class_keypoints`` on the saved inputs -- with key-points
    those are the predictions, the mask and the key-points only."""

    @staticmethod
    def _predictions(pred, pred2, seg_dim):
        return (pred, pred2) if seg_dim is None else (pred[:, :seg_dim], pred[:, seg_dim:])

    @staticmethod
    def forward(ctx, pred, pred2, seg_dim, mask, source, source2, sigma, use_motion, keypoints):
        seg_pred, vertex_pred = _HeadLossFn._predictions(pred, pred2, seg_dim)
        if keypoints == _CLASS_KEYPOINTS:
            losses, _, _ = head_metrics_from_class_keypoints(seg_pred, vertex_pred, mask, source, source2, sigma=sigma,
                                                             use_motion=use_motion)
        elif keypoints:
            losses, _, _ = head_metrics_from_keypoints(seg_pred, vertex_pred, mask, source, source2, sigma=sigma, use_motion=use_motion)
        else:
            losses, _, _ = head_metrics_device(seg_pred, vertex_pred, mask, source, source2, sigma=sigma)
        ctx.present = tuple(t is not None for t in (pred, pred2, mask, source, source2))   # pred2 / weight_scale may be None
        ctx.save_for_backward(*(t for t in (pred, pred2, mask, source, source2) if t is not None))
        ctx.seg_dim, ctx.sigma, ctx.use_motion, ctx.keypoints = seg_dim, sigma, use_motion, keypoints
        loss_seg, loss_vertex, precision, recall = losses.to(torch.float32).unbind(1)
        ctx.mark_non_differentiable(precision, recall)
        return loss_seg, loss_vertex, precision, recall

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_seg, g_vertex, _g_precision, _g_recall):
        saved = iter(ctx.saved_tensors)
        pred, pred2, mask, source, source2 = (next(saved) if there else None for there in ctx.present)
        packed = ctx.seg_dim is not None
        need = (True, True) if packed else ctx.needs_input_grad[:2]
        if not (ctx.needs_input_grad[0] if packed else any(need)):
            return (None,) * 9
        seg_pred, vertex_pred = _HeadLossFn._predictions(pred, pred2, ctx.seg_dim)
        upstream = _upstream(g_seg, g_vertex, pred.shape[0], pred.device)
        grad = torch.empty_like(pred) if packed else None
        out = _HeadLossFn._predictions(grad, None, ctx.seg_dim) if packed else None
        if ctx.keypoints == _CLASS_KEYPOINTS:
            grad_seg, grad_vertex, _ = head_grad_from_class_keypoints(seg_pred, vertex_pred, mask, source, upstream, source2,
                                                                      sigma=ctx.sigma, use_motion=ctx.use_motion, need=need, out=out)
        elif ctx.keypoints:
            grad_seg, grad_vertex, _ = head_grad_from_keypoints(seg_pred, vertex_pred, mask, source, upstream, source2, sigma=ctx.sigma,
                                                                use_motion=ctx.use_motion, need=need, out=out)
        else:
            grad_seg, grad_vertex, _ = head_grad_device(seg_pred, vertex_pred, mask, source, source2, upstream, sigma=ctx.sigma, need=need,
                                                        out=out)
        return ((grad, None) if packed else (grad_seg, grad_vertex)) + (None,) * 7


class HeadLoss(torch.nn.Module):
    """The four loss lines of the reference's ``NetWrapper.forward`` (tools/train_linemod.py:87-91) as a differentiable module:
    ``forward(seg_pred, vertex_pred, mask, vertex, vertex_weights) -> (loss_seg, loss_vertex, precision, recall)``, float32 [b] each,
    bit for bit the values of ``HeadMetrics``.  ``loss_seg`` and ``loss_vertex`` carry a ``grad_fn``; ``precision`` and ``recall`` are
    marked non-differentiable.  The backward is one ``pvnet_head_grad`` call that honours ``needs_input_grad``; it is
    once-differentiable and gives no gradient for the mask, the targets or the weights.

    ``packed(head_out, seg_dim, mask, vertex, vertex_weights)`` takes the network's output before it is sliced into the two
    predictions (lib/networks/model_repository.py:76-78: ``x[:, :seg_dim]``, ``x[:, seg_dim:]``) and writes both gradients into one
    tensor of its shape -- without the two zero-fill-and-copy passes the backward of torch's slices adds.  Same values.

    ``from_keypoints(seg_pred, vertex_pred, mask, hcoords, weight_scale=None, use_motion=False)`` and ``packed_from_keypoints(head_out,
    seg_dim, mask, hcoords, weight_scale=None, use_motion=False)`` take the loader's ``hcoords [b,vn,3]`` instead of the target field and
    its weights (``vertex_targets_device`` states what they and ``use_motion`` stand for; the switch is per call here as in every
    other key-point entry).  Forward and backward compute a pixel's target in registers; the autograd functions save the predictions,
    the mask and the key-points only.
    Same values and gradients as the two forms above on ``vertex_targets_device(mask, hcoords, weight_scale)``, bit for bit; no
    gradient for the mask, the key-points or the scale.

    ``from_class_keypoints(seg_pred, vertex_pred, labels, hcoords, weight_scale=None, use_motion=False)`` and
    ``packed_from_class_keypoints(head_out, seg_dim, labels, hcoords, ...)`` are the same for images of several objects: ``labels`` is a
    label image, ``hcoords [b,C-1,vn,3]`` holds the key-points of class k + 1 in row k and ``weight_scale`` is None, [b] or [b,C-1]
    (``vertex_targets_classes_device`` states the definition).  They equal the first two forms on its output bit for bit and save the
    predictions, the labels and the key-points only."""

    def __init__(self, sigma=1.0):
        super().__init__()
        self.sigma = float(sigma)

    def forward(self, seg_pred, vertex_pred, mask, vertex, vertex_weights):
        return _HeadLossFn.apply(seg_pred, vertex_pred, None, mask, vertex, vertex_weights, self.sigma, False, False)

    @staticmethod
    def _seg_dim(head_out, seg_dim):
        seg_dim = int(seg_dim)
        if not (isinstance(head_out, torch.Tensor) and head_out.dim() == 4 and 2 <= seg_dim < head_out.shape[1]):
            raise RuntimeError("head_out must be [b,seg_dim+2vn,h,w] with seg_dim >= 2")
        return seg_dim

    def packed(self, head_out, seg_dim, mask, vertex, vertex_weights):
        return _HeadLossFn.apply(head_out, None, self._seg_dim(head_out, seg_dim), mask, vertex, vertex_weights, self.sigma, False, False)

    def from_keypoints(self, seg_pred, vertex_pred, mask, hcoords, weight_scale=None, use_motion=False):
        return _HeadLossFn.apply(seg_pred, vertex_pred, None, mask, hcoords, weight_scale, self.sigma, bool(use_motion), True)

    def packed_from_keypoints(self, head_out, seg_dim, mask, hcoords, weight_scale=None, use_motion=False):
        return _HeadLossFn.apply(head_out, None, self._seg_dim(head_out, seg_dim), mask, hcoords, weight_scale, self.sigma,
                                 bool(use_motion), True)

    def from_class_keypoints(self, seg_pred, vertex_pred, labels, hcoords, weight_scale=None, use_motion=False):
        return _HeadLossFn.apply(seg_pred, vertex_pred, None, labels, hcoords, weight_scale, self.sigma, bool(use_motion),
                                 _CLASS_KEYPOINTS)

    def packed_from_class_keypoints(self, head_out, seg_dim, labels, hcoords, weight_scale=None, use_motion=False):
        return _HeadLossFn.apply(head_out, None, self._seg_dim(head_out, seg_dim), labels, hcoords, weight_scale, self.sigma,
                                 bool(use_motion), _CLASS_KEYPOINTS)


class ValStep(object):
    """One validation step behind the backbone (tools/train_linemod.py:200-215), composed of what exists, all on the current
    stream: ``head_metrics_device``, ``voting.PoseEvalWrapper`` (fused arg-max voting, pose solve), ``pose_metrics_device`` with the
    evaluator's class table -- the device part of ``Evaluator.evaluate_batch``.

    ``enqueue(...)`` returns device tensors ``(losses [b,4], counts [b,3], head_status [b], poses [b,3,4], pose_status [b],
    errors [b,4], passed [b,3], metric_status [b])`` without synchronising: it is what ``torch.cuda.graph`` captures (for repeatable votes seed torch's
    CPU generator, ``torch.default_generator.manual_seed``, before each call: the vote draws its seed there).  ``__call__`` is ``enqueue`` plus ONE
    device-to-host copy; it fills the evaluator's recorders as ``evaluate_batch`` does and returns the head metrics as a dict of
    numpy arrays (``loss_seg``, ``loss_vertex``, ``precision``, ``recall``, float32 as the reference's) and the poses."""

    def __init__(self, evaluator, class_type, K=None, intri_type="blender", round_hyp_num=512, inlier_thresh=0.99, max_num=30000,
                 sigma=1.0, sym_projection=False):
        from .voting import PoseEvalWrapper
        self.evaluator, self.class_type = evaluator, class_type
        self.K = evaluator._intrinsics(intri_type) if K is None else K
        self.sigma, self.sym_projection = float(sigma), bool(sym_projection)
        self.eval_net = PoseEvalWrapper(evaluator.points_3d[class_type], self.K, round_hyp_num=round_hyp_num,
                                        inlier_thresh=inlier_thresh, max_num=max_num)

    def _after_head(self, head, seg_pred, vertex_pred, pose_targets):
        """the chain behind the head's ``(losses, counts, status)``: vote, pose solve, pose metrics"""
        from .evaluation import pose_metrics_device
        losses, counts, hstatus = head
        poses, pstatus, _, _ = self.eval_net(seg_pred, vertex_pred, return_all=True)
        _, Kd = self.eval_net._constants(poses.device)
        errors, passed, mstatus = pose_metrics_device(poses, pose_targets, Kd, self.evaluator.device_models(poses.device),
                                                      class_ids=self.class_type, sym_projection=self.sym_projection)
        return losses, counts, hstatus, poses, pstatus, errors, passed, mstatus

    def enqueue(self, seg_pred, vertex_pred, mask, vertex, vertex_weights, pose_targets):
        head = head_metrics_device(seg_pred, vertex_pred, mask, vertex, vertex_weights, sigma=self.sigma)
        return self._after_head(head, seg_pred, vertex_pred, pose_targets)

    def enqueue_from_keypoints(self, seg_pred, vertex_pred, mask, hcoords, pose_targets, weight_scale=None, use_motion=False):
        """``enqueue`` with the head metrics taken from the loader's ``hcoords`` (``head_metrics_from_keypoints``): the same chain, the
        same eight tensors, no target field"""
        head = head_metrics_from_keypoints(seg_pred, vertex_pred, mask, hcoords, weight_scale, sigma=self.sigma, use_motion=use_motion)
        return self._after_head(head, seg_pred, vertex_pred, pose_targets)

    def __call__(self, seg_pred, vertex_pred, mask, vertex, vertex_weights, pose_targets):
        losses, _, _, poses, _, errors, passed, _ = self.enqueue(seg_pred, vertex_pred, mask, vertex, vertex_weights, pose_targets)
        host = torch.cat([losses, errors, passed.to(torch.float64)], 1).cpu().numpy()   # the one copy (it waits for the stream)
        ev = self.evaluator
        for e, ok in zip(host[:, 4:8], host[:, 8:]):
            ev.add_dists.append(float(e[1]))
            ev.add_recorder.append(bool(ok[1]))
            ev.proj_mean_diffs.append(float(e[0]))
            ev.projection_2d_recorder.append(bool(ok[0]))
            ev.cm_degree_5_recorder.append(bool(ok[2]))
        head = {k: host[:, i].astype("float32") for i, k in enumerate(("loss_seg", "loss_vertex", "precision", "recall"))}
        return head, poses
