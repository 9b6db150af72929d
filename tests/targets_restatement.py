"""The float64 numpy restatement of the target field and its weights (include/pvnet_targets.h), the oracle of the device kernels.

Written from the formula, not from the reference's code: for a pixel with ``mask == 1`` at column x, row y and the key-point
(hx, hy, hz)

    v = (hx - x hz, hy - y hz);  n = sqrt(vx vx + vy vy);  if n < 1e-3: n = n + 1e-3;  t = (vx / n, vy / n)

every operation one IEEE float64 operation, t rounded once to float32; with ``use_motion`` t = v.  Every other pixel gets 0.  The
weight of a pixel is ``float32(mask) * weight_scale[image]`` in float32.  tests/test_targets_cpu.py holds it bit for bit against what
the reference's own ``compute_vertex_hcoords`` returned (tests/golden/vertex_targets.npz)."""
import numpy as np


def vertex_targets_f64(mask, hcoords, weight_scale=None, use_motion=False):
    """mask [b,h,w] integers, hcoords [b,vn,3] (or [b,vn,2]: hz = 1) -> (vertex [b,2vn,h,w] float32, vertex_weights [b,1,h,w] float32)"""
    mask = np.asarray(mask)
    hc = np.asarray(hcoords, np.float64)
    if hc.shape[2] == 2:
        hc = np.concatenate([hc, np.ones_like(hc[:, :, :1])], 2)
    b, h, w = mask.shape
    vn = hc.shape[1]
    x = np.arange(w, dtype=np.float64)[None, None, :]
    y = np.arange(h, dtype=np.float64)[None, :, None]
    target = mask == 1
    vertex = np.zeros((b, 2 * vn, h, w), np.float32)
    with np.errstate(all="ignore"):
        for i in range(b):
            for k in range(vn):
                hx, hy, hz = hc[i, k]
                vx = np.broadcast_to(hx - x * hz, (1, h, w))[0]
                vy = np.broadcast_to(hy - y * hz, (1, h, w))[0]
                if not use_motion:
                    n = np.sqrt(vx * vx + vy * vy)
                    n = np.where(n < 1e-3, n + 1e-3, n)
                    vx, vy = vx / n, vy / n
                vertex[i, 2 * k] = np.where(target[i], vx, 0.0).astype(np.float32)
                vertex[i, 2 * k + 1] = np.where(target[i], vy, 0.0).astype(np.float32)
    scale = np.ones((b,), np.float32) if weight_scale is None else np.asarray(weight_scale, np.float32)
    weights = mask.astype(np.float32)[:, None] * scale[:, None, None, None]
    return vertex, weights.astype(np.float32)
