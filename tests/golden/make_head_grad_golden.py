"""Regenerates tests/golden/head_grad.npz: small inputs of the head losses with the gradients the REFERENCE's autograd gives for them.

    python tests/golden/make_head_grad_golden.py <root of a zju3dv/pvnet checkout>

CPU only.  Per case it runs the reference's own code -- ``smooth_l1_loss`` imported from its lib/utils/net_utils.py and
``nn.CrossEntropyLoss(reduce=False)`` used exactly as its NetWrapper.forward does (tools/train_linemod.py:83-90) -- on CPU torch in
float32 UNDER AUTOGRAD, backpropagates ``sum_i u_s[i] loss_seg[i] + u_v[i] loss_vertex[i]`` with non-uniform upstream gradients per
image, and evaluates the float64 restatement (tests/head_grad_restatement.py) on the same inputs.  The third-party modules
net_utils.py imports are stubbed by tools/refshim.py, as in make_head_golden.py, whose input builders this file shares.

The file holds data only: per case the inputs (float16-exact values stored as float16, masks as uint8: widen before use), sigma,
the upstream vectors ``upstream_seg [b]`` / ``upstream_vertex [b]`` (float64), the reference's float32 gradients ``ref32_grad_seg``
/ ``ref32_grad_vertex`` and the restatement's ``f64_grad_seg`` / ``f64_grad_vertex``.  |ref32 - f64| is the reference's own rounding
distance: the only allowance the device test gives it.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "head_grad.npz")


def cases():
    from tests.golden.make_head_golden import f16, typical
    rng = np.random.default_rng(20240927)
    out = {}
    out["typical"] = typical(rng, 2, 24, 32, 3)
    # |d| = 1 / sigma^2 exactly, and its float16 neighbours on both sides, in every plane (sigma = 1 and weight 1: d = p - t)
    c = typical(rng, 1, 8, 16, 2)
    c["mask"][:] = 1
    c["vertex_weights"][:] = 1
    c["vertex"][:] = f16(0.5)
    steps = np.array([1.0, -1.0, np.nextafter(np.float16(1.0), np.float16(2.0)), np.nextafter(np.float16(1.0), np.float16(0.0)), 0.0, 3.0, -0.25,
                      0.999, -np.nextafter(np.float16(1.0), np.float16(2.0)), -np.nextafter(np.float16(1.0), np.float16(0.0))], np.float32)
    c["vertex_pred"][:] = f16(0.5 + np.resize(steps, c["vertex_pred"].shape))
    out["boundary"] = c
    c = typical(rng, 2, 24, 32, 3)
    c["mask"][:] = 0
    c["vertex_weights"][:] = 0   # sum w = 0: D = 1e-3, every field gradient an exact zero
    out["all_background"] = c
    c = typical(rng, 2, 16, 24, 3, noise=1.5)
    c["sigma"] = 0.5
    c["vertex_weights"] = f16(c["vertex_weights"] * rng.uniform(0.25, 2.0, c["vertex_weights"].shape))   # weights other than 0 / 1
    out["sigma_half_weighted"] = c
    c = typical(rng, 1, 24, 32, 2, logit_scale=8.0)   # margins past 20: e_m / S - 1 cancels in float32, the others' share does not
    tie = rng.random(c["mask"].shape) < 0.5
    c["seg_pred"][:, 1][tie] = c["seg_pred"][:, 0][tie]   # tied logits: both classes get +-u / (2 h w)
    out["tied_logits"] = c
    for c in out.values():
        b = c["mask"].shape[0]
        c["upstream_seg"] = np.linspace(0.5, 1.5, b)
        c["upstream_vertex"] = np.linspace(2.0, 0.25, b)
    return out


def reference_gradients(net_utils, c):
    """NetWrapper.forward's loss lines (tools/train_linemod.py:87-89) on CPU float32 tensors, backpropagated by torch's autograd"""
    import torch
    from torch import nn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        criterion = nn.CrossEntropyLoss(reduce=False)
    seg_pred = torch.from_numpy(c["seg_pred"].astype(np.float32)).requires_grad_(True)
    vertex_pred = torch.from_numpy(c["vertex_pred"].astype(np.float32)).requires_grad_(True)
    vertex = torch.from_numpy(c["vertex"].astype(np.float32))
    vertex_weights = torch.from_numpy(c["vertex_weights"].astype(np.float32))
    mask = torch.from_numpy(c["mask"].astype(np.int64))
    loss_seg = criterion(seg_pred, mask)
    loss_seg = torch.mean(loss_seg.view(loss_seg.shape[0], -1), 1)
    if c["sigma"] == 1.0:
        loss_vertex = net_utils.smooth_l1_loss(vertex_pred, vertex, vertex_weights, reduce=False)
    else:
        loss_vertex = net_utils.smooth_l1_loss(vertex_pred, vertex, vertex_weights, sigma=c["sigma"], reduce=False)
    us = torch.from_numpy(c["upstream_seg"].astype(np.float32))
    uv = torch.from_numpy(c["upstream_vertex"].astype(np.float32))
    ((us * loss_seg).sum() + (uv * loss_vertex).sum()).backward()
    return seg_pred.grad.numpy().astype(np.float32), vertex_pred.grad.numpy().astype(np.float32)


def main(reference_root):
    import refshim
    from tests.head_grad_restatement import head_grad_f64
    refshim.install(reference_root)
    spec = importlib.util.spec_from_file_location("reference_net_utils", os.path.join(reference_root, "lib", "utils", "net_utils.py"))
    net_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(net_utils)
    arrays = {}
    names = []
    for name, c in cases().items():
        rs, rv = reference_gradients(net_utils, c)
        gs, gv, status = head_grad_f64(c["seg_pred"], c["vertex_pred"], c["mask"], c["vertex"], c["vertex_weights"], c["upstream_seg"],
                                       c["upstream_vertex"], c["sigma"])
        assert not status.any()
        names.append(name)
        for k in ("seg_pred", "vertex_pred", "mask", "vertex", "vertex_weights", "upstream_seg", "upstream_vertex"):
            arrays[f"{name}.{k}"] = c[k]
        arrays[f"{name}.sigma"] = np.float64(c["sigma"])
        arrays[f"{name}.ref32_grad_seg"], arrays[f"{name}.ref32_grad_vertex"] = rs, rv
        arrays[f"{name}.f64_grad_seg"], arrays[f"{name}.f64_grad_vertex"] = gs, gv
        ds, dv = np.abs(rs - gs), np.abs(rv - gv)
        with np.errstate(all="ignore"):
            print(f"{name:22s} b={rs.shape[0]} |ref32 - f64| over the largest entry: seg {ds.max() / np.abs(gs).max():.1e} "
                  f"field {dv.max() / max(np.abs(gv).max(), 1e-300):.1e}; per element, relative: seg {np.nanmax(ds / np.abs(gs)):.1e}")
    arrays["cases"] = np.array(names)
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
