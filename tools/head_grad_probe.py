"""Measures the training head on the GPU (pvnet_amd/validation.py: HeadLoss, pvnet_head_grad) -> profiles/head_grad_probe.txt.

    python tools/head_grad_probe.py [--out FILE] [--rounds N] [--b B]

At b = 32, 480 x 640, vn = 9, C = 2, int64 masks, float32 and bfloat16 predictions, with enough DISTINCT input sets cycled that more
than the 256 MiB Infinity Cache lies between two uses of a set, in one process, device events on one stream, the variants
alternating:
  (a) the step a user of this project runs: ``HeadLoss`` forward + backward of mean(loss_seg) + 0.5 mean(loss_vertex), two-tensor and
      ``packed`` entry;
  (b) the eager composition of the same formula on PyTorch, forward + backward: what a user runs today;
  (c) the gradient call alone (``head_grad_device`` into preallocated tensors), its achieved bytes/s over the bytes it must move
      (244 B per pixel with float32 predictions: 164 read, 80 written; 204 with bfloat16 predictions), with the default plain
      stores, with everything plain (NT_NONE) and with every load and store non-temporal (NT_ALL).
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pvnet_amd import validation as V  # noqa: E402
from head_metrics_probe import H, W, VN, CACHE, make_set, time_ms  # noqa: E402


def torch_step(seg_pred, vertex_pred, mask, vertex, vertex_weights, criterion):
    """the reference's loss lines (tools/train_linemod.py:87-89, 147-148) and their backward, as torch composes them"""
    b = seg_pred.shape[0]
    seg_pred.grad = vertex_pred.grad = None
    loss_seg = criterion(seg_pred, mask).view(b, -1).mean(1)
    diff = vertex_weights * (vertex_pred - vertex)
    a = diff.abs()
    near = (a < 1.0).detach().float()
    in_loss = diff.pow(2) * 0.5 * near + (a - 0.5) * (1.0 - near)
    loss_vertex = in_loss.view(b, -1).sum(1) / (vertex_pred.shape[1] * vertex_weights.view(b, -1).sum(1) + 1e-3)
    (loss_seg.mean() + 0.5 * loss_vertex.mean()).backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_grad_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--b", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    b = args.b
    say(f"head_grad_probe: {torch.cuda.get_device_name(0)}, b={b}, {H}x{W}, vn={VN}, C=2, int64 masks, sigma=1; times are means of "
        f"device-event windows, median over {args.rounds} alternating rounds (min..max)")
    criterion = torch.nn.CrossEntropyLoss(reduction="none")
    loss = V.HeadLoss()
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
        esz = 2 if dtype == torch.bfloat16 else 4
        planes = 2 + 2 * VN
        bpp = 2 * planes * esz + 2 * VN * 4 + 4 + 8   # predictions read, gradients written, targets, weights, mask
        nbytes = b * H * W * bpp
        nsets = max(2, math.ceil(1.25 * CACHE / nbytes) + 1)
        sets = []
        for k in range(nsets):
            seg, vp, mask, vt, vw = make_set(b, dtype, dev, 1000 * b + k)
            packed = torch.cat([seg, vp], 1).requires_grad_(True)
            sets.append((seg.requires_grad_(True), vp.requires_grad_(True), mask, vt, vw, packed))
        ws = torch.empty(V.head_grad_workspace_bytes(b, H, W), dtype=torch.uint8, device=dev)
        out = (torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1]))
        up = torch.tensor([[1.0 / b, 0.5 / b]] * b, dtype=torch.float64, device=dev)

        def fused(s):
            s[0].grad = s[1].grad = None
            ls, lv, _, _ = loss(*s[:5])
            (ls.mean() + 0.5 * lv.mean()).backward()

        def fused_packed(s):
            s[5].grad = None
            ls, lv, _, _ = loss.packed(s[5], 2, *s[2:5])
            (ls.mean() + 0.5 * lv.mean()).backward()

        def sliced(s):   # HeadLoss on torch's slices of the packed tensor: what packed saves
            s[5].grad = None
            ls, lv, _, _ = loss(s[5][:, :2], s[5][:, 2:], *s[2:5])
            (ls.mean() + 0.5 * lv.mean()).backward()

        def grad_only(flags):
            return lambda s: V.head_grad_device(*[t.detach() for t in s[:2]], *s[2:5], up, out=out, workspace=ws, flags=flags)

        variants = [("HeadLoss fwd+bwd", fused), ("HeadLoss.packed fwd+bwd", fused_packed), ("HeadLoss on slices fwd+bwd", sliced),
                    ("torch eager fwd+bwd", lambda s: torch_step(*s[:5], criterion)),
                    ("forward alone (head_metrics)", lambda s: V.head_metrics_device(*[t.detach() for t in s[:2]], *s[2:5])),
                    ("grad alone (plain stores)", grad_only(0)), ("grad alone (NT_NONE)", grad_only(V.HEAD_F_NT_NONE)),
                    ("grad alone (NT_ALL)", grad_only(V.HEAD_F_NT_ALL))]
        # the two agree before either is timed
        fused(sets[0])
        gs, gv = sets[0][0].grad.clone(), sets[0][1].grad.clone()
        torch_step(*sets[0][:5], criterion)
        agree = [float((a.float() - c.float()).abs().max() / c.float().abs().max()) for a, c in ((gs, sets[0][0].grad), (gv, sets[0][1].grad))]
        reps = max(1, 64 // (b * nsets))
        for _, fn in variants:   # warm-up: every shape, every variant
            time_ms(fn, sets, 1)
        t = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, fn in variants:
                t[n].append(time_ms(fn, sets, reps))
        med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
        say()
        say(f"== {name} predictions: {bpp} B/pixel for the gradient call, {nbytes / 1e6:.1f} MB per call, {nsets} input sets cycled; fused vs "
            f"torch gradients, max difference over the largest entry: seg {agree[0]:.1e} field {agree[1]:.1e}")
        for n, _ in variants:
            v = t[n]
            extra = f"  {nbytes / (med[n] * 1e-3) / 1e9:7.0f} GB/s over the compulsory bytes" if n.startswith("grad alone") else ""
            say(f"  {n:30s} {med[n] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
        a, bt = med["HeadLoss fwd+bwd"], med["torch eager fwd+bwd"]
        say(f"  torch eager / HeadLoss = {bt / a:.2f}x;  torch eager / HeadLoss.packed = {bt / med['HeadLoss.packed fwd+bwd']:.2f}x;  "
            f"HeadLoss on slices / HeadLoss.packed = {med['HeadLoss on slices fwd+bwd'] / med['HeadLoss.packed fwd+bwd']:.2f}x")
        del sets, ws, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
