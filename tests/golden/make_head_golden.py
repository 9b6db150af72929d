"""Regenerates tests/golden/head_metrics.npz: small inputs of the network-head metrics with what the REFERENCE computes from them.

    python tests/golden/make_head_golden.py <root of a zju3dv/pvnet checkout>

CPU only.  Per case it runs the reference's own code -- ``smooth_l1_loss`` and ``compute_precision_recall`` imported from its
lib/utils/net_utils.py and ``nn.CrossEntropyLoss(reduce=False)`` used exactly as its NetWrapper.forward does
(tools/train_linemod.py:83-90) -- on CPU torch in float32, and the float64 restatement (tests/head_restatement.py) on the same
inputs.  The third-party modules net_utils.py imports but these functions never touch (easydict, tensorboardX, torchvision) are
stubbed by tools/refshim.py.

The file holds data only: per case the inputs (float16-exact values stored as float16, masks as uint8: widen before use), sigma,
the reference's float32 outputs ``ref32 [b,4]`` (loss_seg, loss_vertex, precision, recall) and the restatement's ``f64 [b,4]``,
``counts [b,3]``.  |ref32 - f64| is the reference's own rounding distance: the only allowance the device test gives it.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "head_metrics.npz")


def f16(x):
    """round to float16-exact values: the fixture stores them in half the bytes and loses nothing"""
    return np.asarray(x, np.float32).astype(np.float16)


def blob_mask(rng, b, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((b, h, w), np.uint8)
    for i in range(b):
        cy, cx, r = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w, rng.uniform(0.15, 0.3) * min(h, w)
        m[i] = ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r)
    return m


def typical(rng, b, h, w, vn, noise=0.3, logit_scale=3.0):
    mask = blob_mask(rng, b, h, w)
    seg = rng.normal(0.0, logit_scale, (b, 2, h, w))
    seg[:, 1] += (mask * 2.0 - 1.0) * 2.0   # mostly right, some false positives and negatives
    vt = rng.normal(0.0, 1.0, (b, 2 * vn, h, w)) * mask[:, None]
    vp = vt + rng.normal(0.0, noise, vt.shape) + rng.normal(0.0, 2.0, vt.shape) * (rng.random(vt.shape) < 0.1)
    return dict(seg_pred=f16(seg), vertex_pred=f16(vp), mask=mask, vertex=f16(vt), vertex_weights=f16(mask[:, None]), sigma=1.0)


def cases():
    rng = np.random.default_rng(20240611)
    out = {}
    out["typical"] = typical(rng, 2, 40, 48, 9)
    out["large_one_keypoint"] = typical(rng, 1, 96, 128, 1)
    # |d| = 1 / sigma^2 exactly, and its float16 neighbours on both sides, in every plane (sigma = 1 and weight 1: d = p - t)
    c = typical(rng, 1, 8, 16, 2)
    c["mask"][:] = 1
    c["vertex_weights"][:] = 1
    c["vertex"][:] = f16(0.5)
    steps = np.array([1.0, -1.0, np.nextafter(np.float16(1.0), np.float16(2.0)), np.nextafter(np.float16(1.0), np.float16(0.0)), 0.0, 3.0, -0.25,
                      0.999], np.float32)
    c["vertex_pred"][:] = f16(0.5 + np.resize(steps, c["vertex_pred"].shape))
    out["boundary"] = c
    c = typical(rng, 2, 24, 32, 3)
    c["mask"][:] = 0
    c["vertex_weights"][:] = 0   # sum w = 0: 0 / 1e-3
    out["all_background"] = c
    c = typical(rng, 2, 24, 32, 3)
    c["mask"][:] = 1
    c["vertex_weights"][:] = 1
    out["all_foreground"] = c
    c = typical(rng, 1, 24, 40, 2)
    tie = rng.random(c["mask"].shape) < 0.5
    c["seg_pred"][:, 1][tie] = c["seg_pred"][:, 0][tie]   # tied logits: the first maximum (background) wins
    out["tied_logits"] = c
    c = typical(rng, 3, 37, 53, 4, noise=0.2)   # h * w not a multiple of 8
    c["sigma"] = 3.0
    out["sigma_3_odd_size"] = c
    c = typical(rng, 2, 16, 24, 5, noise=1.5)
    c["sigma"] = 0.5
    c["vertex_weights"] = f16(c["vertex_weights"] * rng.uniform(0.25, 2.0, c["vertex_weights"].shape))   # weights other than 0 / 1
    out["sigma_half_weighted"] = c
    return out


def reference_outputs(net_utils, c):
    """NetWrapper.forward's three lines (tools/train_linemod.py:87-90) on CPU float32 tensors"""
    import torch
    from torch import nn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        criterion = nn.CrossEntropyLoss(reduce=False)
    seg_pred = torch.from_numpy(c["seg_pred"].astype(np.float32))
    vertex_pred = torch.from_numpy(c["vertex_pred"].astype(np.float32))
    vertex = torch.from_numpy(c["vertex"].astype(np.float32))
    vertex_weights = torch.from_numpy(c["vertex_weights"].astype(np.float32))
    mask = torch.from_numpy(c["mask"].astype(np.int64))
    loss_seg = criterion(seg_pred, mask)
    loss_seg = torch.mean(loss_seg.view(loss_seg.shape[0], -1), 1)
    if c["sigma"] == 1.0:
        loss_vertex = net_utils.smooth_l1_loss(vertex_pred, vertex, vertex_weights, reduce=False)
    else:
        loss_vertex = net_utils.smooth_l1_loss(vertex_pred, vertex, vertex_weights, sigma=c["sigma"], reduce=False)
    precision, recall = net_utils.compute_precision_recall(seg_pred, mask)
    return torch.stack([loss_seg, loss_vertex, precision, recall], 1).numpy().astype(np.float32)


def main(reference_root):
    import refshim
    from tests.head_restatement import head_metrics_f64
    refshim.install(reference_root)
    spec = importlib.util.spec_from_file_location("reference_net_utils", os.path.join(reference_root, "lib", "utils", "net_utils.py"))
    net_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(net_utils)
    arrays = {}
    names = []
    for name, c in cases().items():
        ref32 = reference_outputs(net_utils, c)
        f64, counts, status = head_metrics_f64(c["seg_pred"], c["vertex_pred"], c["mask"], c["vertex"], c["vertex_weights"], c["sigma"])
        assert not status.any()
        names.append(name)
        for k in ("seg_pred", "vertex_pred", "mask", "vertex", "vertex_weights"):
            arrays[f"{name}.{k}"] = c[k]
        arrays[f"{name}.sigma"] = np.float64(c["sigma"])
        arrays[f"{name}.ref32"] = ref32
        arrays[f"{name}.f64"] = f64
        arrays[f"{name}.counts"] = counts
        rel = np.abs(ref32.astype(np.float64) - f64) / np.maximum(np.abs(f64), 1e-300)
        print(f"{name:22s} b={ref32.shape[0]} max relative |ref32 - f64|: loss_seg {rel[:, 0].max():.1e} loss_vertex {rel[:, 1].max():.1e} "
              f"precision/recall {rel[:, 2:].max():.1e}")
    arrays["cases"] = np.array(names)
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
