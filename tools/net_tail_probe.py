"""Measures the fused network tail (pvnet_amd/tail.py, libpvnet_tail.so) -> profiles/net_tail_probe.txt.

    python tools/net_tail_probe.py [--out FILE] [--rounds N] [--b B]

(tools/tail_probe.py is an older tool about the scoring grid's tail; hence this one's name.)

One MI355X, b = 32, 480 x 640, in one process, device events on one stream, the variants alternating, medians over the rounds.  One pass
of any variant moves more than the 256 MiB Infinity Cache, so one input set is enough.
  (a) ``fused_tail``, bfloat16 features and image in, bfloat16 out, into a preallocated output;
  (b) the eager tail of the stand-in network (tools/e2e_amd.py) in eval(): ``convraw(cat([up(fm), image], 1))`` under
      ``torch.autocast(bfloat16)`` on the same inputs;
  (c) (b) in float32 on float32 copies of the inputs;
  (d) ``fused_tail`` with ``precision="f32"``, float32 in and out;
  (e) a bare device pass over the bytes of (a): the inputs' bytes copied, the rest of the output's bytes filled;
  (f) the stand-in network whole, eager and through ``FusedTailNet``, under autocast(bfloat16) and in float32.
No threshold: the times and (b) / (a), (c) / (d), (a) / (e) are reported.  Then, at a small size, the worst observed ratio of the device's
error to every bar of tests/test_tail_device.py (tests/tail_restatement.py states them).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pvnet_amd import tail as T  # noqa: E402
from head_metrics_probe import H, W, time_ms  # noqa: E402
import e2e_amd  # noqa: E402


def bars(say, dev):
    from tests import tail_cases as TC
    from tests import tail_restatement as TR
    say()
    say("== worst observed ratio of the device's error to each bar (every element; < 1 passes)")
    fm, image, params = TC.seeded(2, 120, 160, 20, seed=5)
    P = T.TailParams(*params)
    for precision in ("bf16", "f32"):
        E = TR.forward_exact(fm, image, *params, precision)
        X = T.fused_tail(fm.to(dev), image.to(dev), P, precision=precision, raw=True).cpu()
        r1 = np.abs(X.double().numpy() - E["X"]) / TR.bar1(E["A1"])
        y_want, A2 = TR.out_exact(TR.stage2_input(X, precision), E["w2"], params[3])
        line = f"  {precision}: stage 1 (2 (K1 + 3) u32 A1) {r1.max():.3f}"
        for dt in (torch.float32, torch.bfloat16):
            y = T.fused_tail(fm.to(dev), image.to(dev), P, precision=precision, out_dtype=dt).cpu()
            r2 = np.abs(y.double().numpy() - y_want) / TR.bar2(A2, y_want, dt)
            line += f";  stage 2, {str(dt).split('.')[1]} out {r2.max():.3f}"
        say(line + "   (2 x 120 x 160, seeded)")
    fm, x, params, seg, ver = TC.g9()
    ref = np.concatenate([seg, ver], 1)
    P = T.TailParams(*params)
    y32 = T.fused_tail(fm.to(dev), x.to(dev), P, precision="f32").cpu().double().numpy()
    y16 = T.fused_tail(fm.to(dev), x.to(dev), P, precision="bf16", out_dtype=torch.float32).cpu().double().numpy()
    bound, _ = TR.bf16_bound(fm, x, *params)
    say(f"  fixture G9: f32 tier / (1e-5 + 1e-5 |ref|) {(np.abs(y32 - ref) / (1e-5 + 1e-5 * np.abs(ref))).max():.3f} "
        f"(max |d| {np.abs(y32 - ref).max():.2e});  bf16 tier / a-priori bound {(np.abs(y16 - ref) / (bound + 1e-5 + 1e-5 * np.abs(ref))).max():.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_tail_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--b", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    b = args.b
    torch.manual_seed(0)
    net = e2e_amd.StandInResnet18_8s().to(dev).eval()
    P = T.TailParams.from_network(net)
    g = torch.Generator(device=dev).manual_seed(1)
    fm32 = torch.nn.functional.leaky_relu(torch.randn((b, 32, H // 2, W // 2), generator=g, device=dev), 0.1)
    im32 = torch.randn((b, 3, H, W), generator=g, device=dev)
    fm16, im16 = fm32.bfloat16(), im32.bfloat16()
    out16 = torch.empty((b, P.cout, H, W), dtype=torch.bfloat16, device=dev)
    out32 = torch.empty((b, P.cout, H, W), dtype=torch.float32, device=dev)
    n_in, n_out = fm16.numel() * 2 + im16.numel() * 2, out16.numel() * 2
    src_flat = torch.empty(n_in, dtype=torch.uint8, device=dev)
    dst_flat = torch.empty(n_out, dtype=torch.uint8, device=dev)
    fused = T.FusedTailNet(net)
    say(f"net_tail_probe: {torch.cuda.get_device_name(0)}, b={b}, {H}x{W}, cout={P.cout}; times are means of device-event windows, median "
        f"over {args.rounds} alternating rounds (min..max)")

    def path_a(_):
        T.fused_tail(fm16, im16, P, precision="bf16", out=out16)

    def path_b(_):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            net.convraw(torch.cat([net.up(fm16), im16], 1))

    def path_c(_):
        with torch.no_grad():
            net.convraw(torch.cat([net.up(fm32), im32], 1))

    def path_d(_):
        T.fused_tail(fm32, im32, P, precision="f32", out=out32)

    def path_e(_):
        dst_flat[:n_in].copy_(src_flat)
        dst_flat[n_in:].zero_()

    def net_eager16(_):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            net(im32)

    def net_fused16(_):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            fused(im32)

    def net_eager32(_):
        with torch.no_grad():
            net(im32)

    def net_fused32(_):
        fused(im32)

    variants = [("(a) fused_tail bf16 in / bf16 out", path_a), ("(b) eager tail, autocast(bfloat16)", path_b), ("(c) eager tail, float32", path_c),
                ("(d) fused_tail precision=f32, float32 in / out", path_d), ("(e) device pass over the bytes of (a)", path_e),
                ("(f) network, eager, autocast(bfloat16)", net_eager16), ("(f) network, FusedTailNet, autocast(bfloat16)", net_fused16),
                ("(f) network, eager, float32", net_eager32), ("(f) network, FusedTailNet, float32", net_fused32)]
    one = [None]
    for _, fn in variants:   # warm-up (and the convolution library's search)
        time_ms(fn, one, 2)
    t = {n: [] for n, _ in variants}
    for _ in range(args.rounds):
        for n, fn in variants:
            t[n].append(time_ms(fn, one, 2))
    med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
    say()
    say(f"== (a) moves {(n_in + n_out) / 1e6:.0f} MB per batch: {n_in / 1e6:.0f} MB in, {n_out / 1e6:.0f} MB out")
    for n, _ in variants:
        v = t[n]
        extra = f"  {(n_in + n_out) / (med[n] * 1e-3) / 1e9:7.1f} GB/s" if n[:3] in ("(a)", "(e)") else ""
        say(f"  {n:50s} {med[n] * 1e3:10.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
    a, bb, c, d, e, n16, f16, n32, f32 = (v[0] for v in variants)
    say(f"  (b) / (a) = {med[bb] / med[a]:.2f};  (c) / (d) = {med[c] / med[d]:.2f};  (a) / (e) = {med[a] / med[e]:.2f};  network "
        f"autocast: {med[n16]:.2f} -> {med[f16]:.2f} ms ({(med[f16] / med[n16] - 1) * 100:+.1f} %), float32: {med[n32]:.2f} -> {med[f32]:.2f} ms "
        f"({(med[f32] / med[n32] - 1) * 100:+.1f} %)")
    bars(say, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
