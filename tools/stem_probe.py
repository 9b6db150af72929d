"""Measures the fused stem (pvnet_amd/stem.py, libpvnet_stem.so) -> profiles/stem_probe.txt.

    python tools/stem_probe.py [--out FILE] [--rounds N] [--b B]

One MI355X, b = 32, 480 x 640 (x2s at 240 x 320, the pooled tensor at 120 x 160), in one process, device events on one stream, the
variants alternating, medians over the rounds with min and max.
  (a) ``fused_stem``, float32 image in, bfloat16 out, both outputs, into preallocated tensors;
  (b) the eager stem and pool of the stand-in network (tools/e2e_amd.py) in eval(): ``pool(stem(image))`` under
      ``torch.autocast(bfloat16)`` on the same image -- the yardstick;
  (c) a bare device pass over the bytes of (a): the image is smaller than the outputs, so as many bytes copied as it has and the rest
      of the outputs' bytes written by a fill.
Then the stand-in network whole under autocast(bfloat16): eager, ``FusedDecoderNet``, ``FusedStemNet`` with the stem fused and with its
default.  No time is fixed in advance.  The rule the report applies: the stem is fused by default in ``FusedStemNet`` (``DEFAULT_STEM``)
when (a) is below (b) by more than the spread (max - min) of (b)'s rounds.  Then, at the size of the device tests' network case, what
the eager network under autocast differs from the eager float32 network by (e) and what the fused networks do.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pvnet_amd import decoder as D  # noqa: E402
from pvnet_amd import stem as S  # noqa: E402
from head_metrics_probe import H, W, network_error, time_ms  # noqa: E402
import e2e_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_probe.txt"))
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
    g = torch.Generator(device=dev).manual_seed(1)
    say(f"stem_probe: {torch.cuda.get_device_name(0)}, b={b}, network input {H}x{W}; times are means of device-event windows, median over "
        f"{args.rounds} alternating rounds (min..max)")
    im = torch.randn((b, 3, H, W), generator=g, device=dev)
    P = S.StemParams.from_network(net)
    ho, wo, hp, wp = S.out_sizes(H, W)
    out = (torch.empty((b, 64, ho, wo), dtype=torch.bfloat16, device=dev), torch.empty((b, 64, hp, wp), dtype=torch.bfloat16, device=dev))
    n_in, n_out = im.numel() * 4, (out[0].numel() + out[1].numel()) * 2
    src, dst = torch.zeros(n_in // 4, dtype=torch.float32, device=dev), torch.empty(n_out // 4, dtype=torch.float32, device=dev)
    flop = 2 * 147 * 64 * b * ho * wo

    def path_a(_):
        S.fused_stem(im, P, out=out)

    def path_b(_):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            net.pool(net.stem(im))

    def path_c(_):   # the image is smaller than the outputs: as many bytes copied as it has, the rest only written
        m = min(src.numel(), dst.numel())
        dst[:m].copy_(src[:m])
        if dst.numel() > m:
            dst[m:].zero_()
        if src.numel() > m:
            src[m:].sum()

    variants = [("stem (a) fused_stem f32 in / bf16 out, x2s and pooled", path_a), ("stem (b) eager stem + pool, autocast(bfloat16)", path_b),
                ("stem (c) device pass over the bytes of (a)", path_c)]
    nets = {"eager": net, "FusedDecoderNet": D.FusedDecoderNet(net), "FusedStemNet, stem fused": S.FusedStemNet(net, stem=True),
            f"FusedStemNet, default (stem={S.DEFAULT_STEM})": S.FusedStemNet(net)}
    for name, m in nets.items():
        def run_net(_, m=m):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                m(im)
        variants.append((f"network, {name}", run_net))
    one = [None]
    for _, fn in variants:   # warm-up (and the convolution library's search)
        time_ms(fn, one, 2)
    t = {n: [] for n, _ in variants}
    for _ in range(args.rounds):
        for n, fn in variants:
            t[n].append(time_ms(fn, one, 2))
    med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
    say()
    say(f"== stem: (a) moves {(n_in + n_out) / 1e6:.0f} MB per batch ({n_in / 1e6:.0f} MB in, {n_out / 1e6:.0f} MB out) and computes {flop / 1e9:.0f} GFLOP")
    a, bb, c = (n for n, _ in variants if n.startswith("stem"))
    for n in (a, bb, c):
        v = t[n]
        extra = f"  {flop / (med[n] * 1e-3) / 1e12:6.1f} TFLOP/s" if n != c else f"  {(n_in + n_out) / (med[n] * 1e-3) / 1e9:7.1f} GB/s"
        say(f"  {n:56s} {med[n] * 1e3:10.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
    spread = max(t[bb]) - min(t[bb])
    verdict = "fused by default" if med[bb] - med[a] > spread else "NOT fused by default (the kernel stays reachable with stem=True)"
    say(f"  (b) / (a) = {med[bb] / med[a]:.2f};  (a) / (c) = {med[a] / med[c]:.2f};  (b) - (a) = {(med[bb] - med[a]) * 1e3:.1f} us against a spread of "
        f"(b)'s rounds of {spread * 1e3:.1f} us: {verdict}")
    say()
    say("== the stand-in network under autocast(bfloat16)")
    base = med["network, eager"]
    for n, _ in variants:
        if n.startswith("network"):
            v = t[n]
            say(f"  {n:62s} {med[n]:8.2f} ms  ({min(v):.2f} .. {max(v):.2f})  {(med[n] / base - 1) * 100:+6.1f} % of eager")
    network_error(say, dev, "FusedStemNet (stem and both stages)", lambda net: S.FusedStemNet(net, stem=True, stages=D.STAGES),
                  "FusedDecoderNet (both stages)", lambda net: D.FusedDecoderNet(net, stages=D.STAGES))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
