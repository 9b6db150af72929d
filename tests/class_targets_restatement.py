"""The float64 numpy restatement of the targets of several objects (include/pvnet_class_targets.h), the oracle of the device kernels.

Built on the single-class restatement, tests/targets_restatement.vertex_targets_f64, once per class on the binary mask
``labels == k + 1`` with ``hcoords[:, k]``, and combined by SELECTION -- ``np.where(labels == k + 1, ...)`` -- never by addition: a
target of ``-0.0`` on a pixel of class k + 1 stays ``-0.0``, which ``0.0 + -0.0`` would not keep.  Every pixel whose label is not in
1 .. C-1 keeps target ``+0.0`` and weight ``0.0``; the weight of a pixel of class k + 1 is ``weight_scale[i, k]`` (1 without a scale)."""
import numpy as np

from tests.targets_restatement import vertex_targets_f64


def class_weight_scale(weight_scale, b, nk):
    """None, [b] or [b,nk] -> [b,nk] float32"""
    if weight_scale is None:
        return np.ones((b, nk), np.float32)
    ws = np.asarray(weight_scale, np.float32)
    return np.ascontiguousarray(np.broadcast_to(ws[:, None] if ws.ndim == 1 else ws, (b, nk)))


def vertex_targets_classes_f64(labels, hcoords, weight_scale=None, use_motion=False):
    """labels [b,h,w] integers, hcoords [b,nk,vn,3] (or [...,2]: hz = 1), weight_scale None / [b] / [b,nk]
    -> (vertex [b,2vn,h,w] float32, vertex_weights [b,1,h,w] float32)"""
    labels = np.asarray(labels)
    hc = np.asarray(hcoords, np.float64)
    b, h, w = labels.shape
    nk, vn = hc.shape[1], hc.shape[2]
    ws = class_weight_scale(weight_scale, b, nk)
    vertex = np.zeros((b, 2 * vn, h, w), np.float32)
    weights = np.zeros((b, 1, h, w), np.float32)
    for k in range(nk):
        own = labels == k + 1
        v, _ = vertex_targets_f64(own.astype(np.int64), hc[:, k], None, use_motion)
        vertex = np.where(own[:, None], v, vertex)
        weights = np.where(own[:, None], ws[:, k][:, None, None, None], weights)
    return vertex, weights.astype(np.float32)
