"""The float64 restatement of the network-head metrics (include/pvnet_head.h), on the host: the oracle of the device kernel
(tests/test_head_metrics_device.py) and the float64 column of tests/golden/head_metrics.npz (tests/golden/make_head_golden.py).

Term for term what the reference's NetWrapper.forward computes (tools/train_linemod.py:85-91, lib/utils/net_utils.py:54-79 and
:329-348), on the inputs as stored, widened to float64.

Written so that its results do not depend on the machine: the elementwise steps are single IEEE operations; every sum is
``math.fsum`` (the correctly rounded sum, whatever the order) and exp / log are the C library's through ``math`` -- numpy's own
sums and transcendental loops change with the vector width of the CPU they run on.
"""
import math

import numpy as np

_exp = np.frompyfunc(math.exp, 1, 1)
_log = np.frompyfunc(math.log, 1, 1)


def _elementwise(f, x):
    """f over a float64 array.  The arguments met here never make ``math`` raise: exp sees s - max <= 0 (or NaN), log a sum that
    holds exp(0) = 1 (or NaN / inf)."""
    return f(np.asarray(x, np.float64)).astype(np.float64)


def _fsum(x):
    x = np.asarray(x, np.float64).ravel()
    if not np.isfinite(x).all():
        return float(np.sum(x))   # NaN / inf: only which of them comes out matters
    return math.fsum(x.tolist())


def head_metrics_f64(seg_pred, vertex_pred, mask, vertex, vertex_weights, sigma=1.0):
    """numpy in (any float / integer dtypes), ``(losses [b,4] float64, counts [b,3] int64, status [b] int32)`` out:
    losses = (loss_seg, loss_vertex, precision, recall), counts = (tp, fp, fn), status 1 for an image with a label outside
    0 .. C-1 (its loss_seg is NaN; such a pixel counts as foreground)."""
    s = np.asarray(seg_pred).astype(np.float64)
    p = np.asarray(vertex_pred).astype(np.float64)
    t = np.asarray(vertex).astype(np.float64)
    w = np.asarray(vertex_weights).astype(np.float64)
    lab = np.asarray(mask).astype(np.int64)
    b, C, h, wd = s.shape
    planes = p.shape[1]
    s2 = float(sigma) * float(sigma)
    losses = np.zeros((b, 4))
    counts = np.zeros((b, 3), np.int64)
    status = np.zeros((b,), np.int32)
    for i in range(b):
        with np.errstate(all="ignore"):
            # argmax as torch: the first maximum wins, a NaN counts as the maximum (numpy's argmax has the same rule)
            pred = np.argmax(s[i], 0)
            m = np.max(s[i], 0)   # NaN where a logit is NaN
            bad = (lab[i] < 0) | (lab[i] >= C)
            sl = np.take_along_axis(s[i], np.where(bad, 0, lab[i])[None], 0)[0]
            acc = np.zeros_like(m)
            for c in range(C):   # sum_c exp(s_c - max) in class order, as the kernel adds them
                acc = acc + _elementwise(_exp, s[i, c] - m)
            ce = _elementwise(_log, acc) - (sl - m)   # log_softmax's form: the maximum subtracted first
            d = w[i] * (p[i] - t[i])   # [1,h,w] broadcast over the planes
            a = np.abs(d)
            term = np.where(a < 1.0 / s2, d * d * (s2 / 2.0), a - 0.5 / s2)
        losses[i, 0] = np.nan if bad.any() else _fsum(ce) / (h * wd)
        losses[i, 1] = _fsum(term) / (planes * _fsum(w[i]) + 1e-3)
        fg, pf = lab[i] != 0, pred != 0
        tp, fp, fn = int((pf & fg).sum()), int((pf & ~fg).sum()), int((~pf & fg).sum())
        losses[i, 2] = (tp + 1.0) / (tp + fp + 1.0)
        losses[i, 3] = (tp + 1.0) / (tp + fn + 1.0)
        counts[i] = (tp, fp, fn)
        status[i] = int(bad.any())
    return losses, counts, status
