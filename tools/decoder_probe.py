"""Measures the fused decoder stages (pvnet_amd/decoder.py, libpvnet_decoder.so) -> profiles/decoder_probe.txt.

    python tools/decoder_probe.py [--out FILE] [--rounds N] [--b B]

One MI355X, b = 32, 480 x 640 network shapes (conv4s at 120 x 160, conv2s at 240 x 320), in one process, device events on one stream, the
variants alternating, medians over the rounds with min and max.  Per stage
  (a) ``fused_stage``, bfloat16 in, bfloat16 out, into a preallocated output;
  (b) the eager stage of the stand-in network (tools/e2e_amd.py) in eval(): ``convNs(cat([up(lo), skip], 1))`` under
      ``torch.autocast(bfloat16)`` on the same inputs -- the yardstick;
  (c) a bare device pass over the bytes of (a): the inputs are larger than the output, so as many bytes copied as the output has and
      the rest of the inputs' bytes read by a float32 sum.
Then the stand-in network whole under autocast(bfloat16): eager, ``FusedTailNet``, ``FusedDecoderNet`` with every stage fused and with
its default stages.  No time is fixed in advance.  The rule the report applies per stage: the stage belongs in ``FusedDecoderNet``'s
default ``stages`` when (a) is below (b) by more than the spread (max - min) of (b)'s rounds.  Then, at the size of the device tests'
network case, what the eager network under autocast differs from the eager float32 network by (e) and what the fused network does.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pvnet_amd import decoder as D  # noqa: E402
from pvnet_amd import tail as T  # noqa: E402
from head_metrics_probe import H, W, network_error, time_ms  # noqa: E402
import e2e_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_probe.txt"))
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
    say(f"decoder_probe: {torch.cuda.get_device_name(0)}, b={b}, network input {H}x{W}; times are means of device-event windows, median over "
        f"{args.rounds} alternating rounds (min..max)")
    variants, facts = [], {}
    for stage, div in (("conv4s", 4), ("conv2s", 2)):
        P = D.StageParams.from_network(net, stage)
        h, w = H // div, W // div
        lo = torch.nn.functional.leaky_relu(torch.randn((b, P.cl, h // 2, w // 2), generator=g, device=dev), 0.1).bfloat16()
        skip = torch.relu(torch.randn((b, P.cs, h, w), generator=g, device=dev)).bfloat16()
        out = torch.empty((b, P.co, h, w), dtype=torch.bfloat16, device=dev)
        n_in, n_out = (lo.numel() + skip.numel()) * 2, out.numel() * 2
        src, dst = torch.zeros(n_in // 4, dtype=torch.float32, device=dev), torch.empty(n_out // 4, dtype=torch.float32, device=dev)
        seq = getattr(net, stage)
        facts[stage] = (n_in, n_out, 2 * 9 * (P.cl + P.cs) * P.co * b * h * w)

        def path_a(_, lo=lo, skip=skip, P=P, out=out):
            D.fused_stage(lo, skip, P, out=out)

        def path_b(_, lo=lo, skip=skip, seq=seq):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                seq(torch.cat([net.up(lo), skip], 1))

        def path_c(_, src=src, dst=dst):   # the inputs are larger than the output: as many bytes copied as it has, the rest only read
            m = min(src.numel(), dst.numel())
            dst[:m].copy_(src[:m])
            if dst.numel() > m:
                dst[m:].zero_()
            if src.numel() > m:
                src[m:].sum()

        variants += [(f"{stage} (a) fused_stage bf16 in / bf16 out", path_a), (f"{stage} (b) eager stage, autocast(bfloat16)", path_b),
                     (f"{stage} (c) device pass over the bytes of (a)", path_c)]
    im = torch.randn((b, 3, H, W), generator=g, device=dev)
    nets = {"eager": net, "FusedTailNet": T.FusedTailNet(net), "FusedDecoderNet, both stages": D.FusedDecoderNet(net, stages=D.STAGES),
            f"FusedDecoderNet, default stages {D.DEFAULT_STAGES}": D.FusedDecoderNet(net)}
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
    for stage in ("conv4s", "conv2s"):
        n_in, n_out, flop = facts[stage]
        say()
        say(f"== {stage}: (a) moves {(n_in + n_out) / 1e6:.0f} MB per batch ({n_in / 1e6:.0f} MB in, {n_out / 1e6:.0f} MB out) and computes {flop / 1e9:.0f} GFLOP")
        a, bb, c = (n for n, _ in variants if n.startswith(stage))
        for n in (a, bb, c):
            v = t[n]
            extra = f"  {flop / (med[n] * 1e-3) / 1e12:6.1f} TFLOP/s" if n != c else f"  {(n_in + n_out) / (med[n] * 1e-3) / 1e9:7.1f} GB/s"
            say(f"  {n:52s} {med[n] * 1e3:10.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
        spread = max(t[bb]) - min(t[bb])
        verdict = "fused by default" if med[bb] - med[a] > spread else "NOT fused by default (the kernel stays reachable by naming the stage)"
        say(f"  (b) / (a) = {med[bb] / med[a]:.2f};  (a) / (c) = {med[a] / med[c]:.2f};  (b) - (a) = {(med[bb] - med[a]) * 1e3:.1f} us against a spread of "
            f"(b)'s rounds of {spread * 1e3:.1f} us: {verdict}")
    say()
    say("== the stand-in network under autocast(bfloat16)")
    base = med["network, eager"]
    for n, _ in variants:
        if n.startswith("network"):
            v = t[n]
            say(f"  {n:62s} {med[n]:8.2f} ms  ({min(v):.2f} .. {max(v):.2f})  {(med[n] / base - 1) * 100:+6.1f} % of eager")
    network_error(say, dev, "FusedDecoderNet (both stages)", lambda net: D.FusedDecoderNet(net, stages=D.STAGES),
                  "FusedTailNet", T.FusedTailNet)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
