"""Measures the targets from key-points on the GPU (pvnet_amd/validation.py: vertex_targets_device, HeadLoss.from_keypoints)
-> profiles/targets_probe.txt.

    python tools/targets_probe.py [--out FILE] [--rounds N] [--b B]

At b = 32, 480 x 640, vn = 9, C = 2, int64 masks, float32 and bfloat16 predictions, with enough DISTINCT input sets cycled that more
than the 256 MiB Infinity Cache lies between two uses of a set, in one process, device events on one stream, the variants
alternating:
  (a) the path before this library: ``HeadLoss`` forward + backward of mean(loss_seg) + 0.5 mean(loss_vertex) on target tensors that
      are already resident on the device -- the case most favourable to it, it is not charged the copy of (d);
  (b) ``vertex_targets_device`` into preallocated tensors, then (a) on them;
  (c) ``HeadLoss.from_keypoints`` forward + backward: no target field anywhere;
  (d) the host-to-device copy of the target field and the weights (pinned memory) that (b) and (c) no longer need, reported apart;
and, to place a difference, the pieces alone: the materialising kernel, the two forwards, the two gradient calls.
The targets of (a) are those ``vertex_targets_device`` makes from the key-points of (c): the three compute the same numbers.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_probe.txt"))
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
    say(f"targets_probe: {torch.cuda.get_device_name(0)}, b={b}, {H}x{W}, vn={VN}, C=2, int64 masks, sigma=1; times are means of "
        f"device-event windows, median over {args.rounds} alternating rounds (min..max)")
    loss = V.HeadLoss()
    verdicts = []
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
        esz = 2 if dtype == torch.bfloat16 else 4
        planes = 2 + 2 * VN
        moved_a = (2 * planes * esz + 2 * (2 * VN * 4 + 4 + 8)) + planes * esz   # forward reads + backward reads, gradients written
        moved_c = 2 * (planes * esz + 8) + planes * esz
        nbytes = b * H * W * moved_c
        nsets = max(2, math.ceil(1.25 * CACHE / nbytes) + 1)
        sets = []
        for k in range(nsets):
            seg, vp, mask, _, _ = make_set(b, dtype, dev, 1000 * b + k)
            g = torch.Generator(device="cpu").manual_seed(k)
            centre = torch.stack([(mask[i] > 0).nonzero().double().mean(0).flip(0) for i in range(b)]).cpu()   # (x, y)
            hc = torch.cat([centre[:, None, :] + (torch.rand((b, VN, 2), generator=g, dtype=torch.float64) - 0.5) * 120.0,
                            torch.ones((b, VN, 1), dtype=torch.float64)], 2).to(dev)
            vt, vw = V.vertex_targets_device(mask, hc)
            sets.append((seg.requires_grad_(True), vp.requires_grad_(True), mask, vt, vw, hc))
        torch.cuda.synchronize()
        out_t = (torch.empty_like(sets[0][3]), torch.empty_like(sets[0][4]))
        out_g = (torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1]))
        ws = torch.empty(V.head_grad_workspace_bytes(b, H, W), dtype=torch.uint8, device=dev)
        up = torch.tensor([[1.0 / b, 0.5 / b]] * b, dtype=torch.float64, device=dev)
        host = (sets[0][3].cpu().pin_memory(), sets[0][4].cpu().pin_memory())
        copy_bytes = sum(t.numel() * t.element_size() for t in host)

        def path_a(s):
            s[0].grad = s[1].grad = None
            ls, lv, _, _ = loss(*s[:5])
            (ls.mean() + 0.5 * lv.mean()).backward()

        def path_b(s):
            V.vertex_targets_device(s[2], s[5], out=out_t)
            s[0].grad = s[1].grad = None
            ls, lv, _, _ = loss(s[0], s[1], s[2], *out_t)
            (ls.mean() + 0.5 * lv.mean()).backward()

        def path_c(s):
            s[0].grad = s[1].grad = None
            ls, lv, _, _ = loss.from_keypoints(s[0], s[1], s[2], s[5])
            (ls.mean() + 0.5 * lv.mean()).backward()

        def copy_d(s):
            out_t[0].copy_(host[0], non_blocking=True)
            out_t[1].copy_(host[1], non_blocking=True)

        det = lambda s: [t.detach() for t in s[:2]]   # noqa: E731
        variants = [("(a) HeadLoss fwd+bwd, resident targets", path_a), ("(b) vertex_targets_device + (a)", path_b),
                    ("(c) HeadLoss.from_keypoints fwd+bwd", path_c), ("(d) host-to-device copy of the targets", copy_d),
                    ("vertex_targets_device alone", lambda s: V.vertex_targets_device(s[2], s[5], out=out_t)),
                    ("forward alone, targets", lambda s: V.head_metrics_device(*det(s), *s[2:5])),
                    ("forward alone, key-points", lambda s: V.head_metrics_from_keypoints(*det(s), s[2], s[5])),
                    ("grad alone, targets", lambda s: V.head_grad_device(*det(s), *s[2:5], up, out=out_g, workspace=ws)),
                    ("grad alone, key-points", lambda s: V.head_grad_from_keypoints(*det(s), s[2], s[5], up, out=out_g, workspace=ws))]
        # the three paths agree before any is timed
        path_a(sets[0])
        ga = (sets[0][0].grad.clone(), sets[0][1].grad.clone())
        path_c(sets[0])
        agree = all(torch.equal(x, y) for x, y in zip(ga, (sets[0][0].grad, sets[0][1].grad)))
        path_b(sets[0])
        agree = agree and all(torch.equal(x, y) for x, y in zip(ga, (sets[0][0].grad, sets[0][1].grad)))
        reps = max(1, 64 // (b * nsets))
        for _, fn in variants:   # warm-up: every shape, every variant
            time_ms(fn, sets, 1)
        t = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, fn in variants:
                t[n].append(time_ms(fn, sets, reps))
        med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
        say()
        say(f"== {name} predictions: forward + backward move {moved_a} B/pixel on targets, {moved_c} B/pixel on key-points; {nsets} input "
            f"sets cycled; gradients of (a), (b), (c) bitwise equal: {agree}")
        for n, _ in variants:
            v = t[n]
            extra = f"  {copy_bytes / (med[n] * 1e-3) / 1e9:6.1f} GB/s, {copy_bytes / 1e6:.0f} MB" if n.startswith("(d)") else ""
            say(f"  {n:42s} {med[n] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
        a, c = "(a) HeadLoss fwd+bwd, resident targets", "(c) HeadLoss.from_keypoints fwd+bwd"
        ok = med[c] <= med[a]
        verdicts.append(ok)
        say(f"  (c) / (a) = {med[c] / med[a]:.3f};  (b) / (a) = {med['(b) vertex_targets_device + (a)'] / med[a]:.3f};  spread of (a) "
            f"{(max(t[a]) - min(t[a])) / med[a] * 100:.1f} %;  median of (c) no slower than median of (a): {'yes' if ok else 'NO'}")
        del sets, ws, out_t, out_g, host
        torch.cuda.empty_cache()
    say()
    say(f"requirement (median of (c) <= median of (a), both prediction types): {'met' if all(verdicts) else 'NOT met'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
