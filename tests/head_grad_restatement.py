"""The float64 restatement of the head losses' gradients (include/pvnet_train.h), on the host: the oracle of the device kernel
(tests/test_head_grad_device.py) and the float64 columns of tests/golden/head_grad.npz (tests/golden/make_head_grad_golden.py).

The closed-form derivative of what tests/head_restatement.py computes forward (the reference's NetWrapper.forward,
tools/train_linemod.py:85-91 with lib/utils/net_utils.py:54-79), on the inputs as stored, widened to float64.

Machine-independent for the same reasons as the forward's restatement: the elementwise steps are single IEEE operations in a stated
order, the sum of the weights is ``math.fsum`` and exp is the C library's through ``math``.
"""
import numpy as np

from tests.head_restatement import _elementwise, _exp, _fsum


def head_grad_f64(seg_pred, vertex_pred, mask, vertex, vertex_weights, upstream_seg, upstream_vertex, sigma=1.0):
    """numpy in (any float / integer dtypes; the two upstream vectors [b]), ``(grad_seg [b,C,h,w] float64, grad_vertex [b,2vn,h,w]
    float64, status [b] int32)`` out.  status 1 for an image with a label outside 0 .. C-1: that pixel's C gradients are NaN."""
    s = np.asarray(seg_pred).astype(np.float64)
    p = np.asarray(vertex_pred).astype(np.float64)
    t = np.asarray(vertex).astype(np.float64)
    w = np.asarray(vertex_weights).astype(np.float64)
    lab = np.asarray(mask).astype(np.int64)
    us = np.asarray(upstream_seg, np.float64)
    uv = np.asarray(upstream_vertex, np.float64)
    b, C, h, wd = s.shape
    planes = p.shape[1]
    s2 = float(sigma) * float(sigma)
    inv = 1.0 / s2
    gs = np.zeros_like(s)
    gv = np.zeros_like(p)
    status = np.zeros((b,), np.int32)
    for i in range(b):
        with np.errstate(all="ignore"):
            m = np.max(s[i], 0)   # NaN where a logit is NaN: the pixel's gradients are NaN
            bad = (lab[i] < 0) | (lab[i] >= C)
            e = [_elementwise(_exp, s[i, c] - m) for c in range(C)]
            total = np.zeros_like(m)
            rest = np.zeros_like(m)   # the share of the classes other than the label's, in class order
            for c in range(C):
                total = total + e[c]
                rest = rest + np.where(lab[i] == c, 0.0, e[c])
            ks = us[i] / float(h * wd)
            for c in range(C):
                g = np.where(lab[i] == c, -(ks * (rest / total)), ks * (e[c] / total))
                gs[i, c] = np.where(bad, np.nan, g)
            kv = uv[i] / (planes * _fsum(w[i]) + 1e-3)
            d = w[i] * (p[i] - t[i])   # [1,h,w] broadcast over the planes
            sgn = np.where(d > 0.0, 1.0, np.where(d < 0.0, -1.0, d))   # a NaN stays a NaN
            gv[i] = np.where(np.abs(d) < inv, w[i] * (d * s2), w[i] * sgn) * kv
        status[i] = int(bad.any())
    return gs, gv, status


def ulp(x, dtype):
    """the bar of the device test: one unit in the last place of ``dtype`` at |x| taken relatively -- 2^-23 |x| for float32, 2^-10 |x|
    for float16, 2^-7 |x| for bfloat16 -- or one subnormal step of the type where that is larger"""
    rel, step = {"float32": (2.0 ** -23, 2.0 ** -149), "float16": (2.0 ** -10, 2.0 ** -24), "bfloat16": (2.0 ** -7, 2.0 ** -133)}[dtype]
    return np.maximum(rel * np.abs(np.asarray(x, np.float64)), step)

