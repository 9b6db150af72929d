"""Measures the fused trunk convolution (pvnet_amd/trunk.py, libpvnet_trunk.so) -> profiles/trunk_probe.txt.

    python tools/trunk_probe.py [--out FILE] [--rounds N] [--b B]

One MI355X, b = 32, 480 x 640 network shapes (the pooled tensor at 120 x 160, the features at stride 8 at 60 x 80), in one process,
device events on one stream, the variants alternating, medians over the rounds with min and max.  For each piece of the trunk --
``layer1 .. layer4``, ``fc``, ``conv8s`` of the stand-in network (tools/e2e_amd.py) in eval(), under ``torch.autocast(bfloat16)``, on
bfloat16 features of the piece's own shape --
  (a) the fused piece: ``FusedBasicBlock``s (two launches each, a 1 x 1 downsample under PyTorch) or one ``fused_conv3x3``;
  (b) the eager piece: the network's own modules (``conv8s`` with its ``torch.cat``) -- the yardstick, with the spread of its rounds;
  (c) a bare device pass over the bytes (a) has to move at least: every launch's inputs once and its output once;
  and the MFMA-rate floor: the piece's 3 x 3 flops at 2.5 PFLOP/s.
Then the stand-in network whole under autocast(bfloat16): eager, ``FusedStemNet`` (the path without this library), ``FusedTrunkNet``
with every piece fused, with the pieces the rule selects, and with its default.  No time is fixed in advance.  The rule the report
applies: ``DEFAULT_LAYERS`` holds exactly the pieces whose (a) is below (b) by more than the spread (max - min) of (b)'s rounds.  Then,
at the size of the device tests' network case, what the eager network under autocast differs from the eager float32 network by (e) and
what the fused network does.
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
from pvnet_amd import trunk as T  # noqa: E402
from head_metrics_probe import H, W, network_error, time_ms  # noqa: E402
import e2e_amd  # noqa: E402

PEAK = 2.5e15   # bfloat16 matrix peak, dense, FLOP/s


def conv_work(p, b, h, w):
    """(flops, bytes moved at least, output sides) of one launch on bfloat16 tensors: inputs once, output once, packed weights once"""
    ho, wo = T.out_sizes(h, w, p.stride)
    return 2 * 9 * p.cin * p.co * b * ho * wo, 2 * (b * p.cin * h * w + b * p.co * ho * wo + 9 * p.cin * p.co), (ho, wo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trunk_probe.txt"))
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
    say(f"trunk_probe: {torch.cuda.get_device_name(0)}, b={b}, network input {H}x{W}; times are means of device-event windows, median over "
        f"{args.rounds} alternating rounds (min..max)")
    everything = T.FusedTrunkNet(net, layers=T.LAYERS, stem=True)
    h4, w4 = S.out_sizes(H, W)[2:]                 # the pooled tensor's sides
    h8, w8 = T.out_sizes(h4, w4, 2)

    def feat(c, h, w):
        return torch.relu(torch.randn((b, c, h, w), generator=g, device=dev)).to(torch.bfloat16)

    x8s = feat(128, h8, w8)
    # name -> (input, eager, fused, [(ConvParams, h, w) of every launch], residual tensors read)
    pieces = {}
    sides = {"layer1": (64, h4, w4), "layer2": (64, h4, w4), "layer3": (128, h8, w8), "layer4": (256, h8, w8)}
    for k, name in enumerate(T.LAYERS[:4]):
        c, h, w = sides[name]
        seq, blocks, launches = everything.parts.layers[k], everything.blocks[name], []
        for blk in blocks:
            launches.append((blk.conv1, h, w))
            h, w = T.out_sizes(h, w, blk.conv1.stride)
            launches.append((blk.conv2, h, w))

        def fused(x, blocks=blocks):
            for blk in blocks:
                x = blk(x)
            return x
        pieces[name] = (feat(c, *sides[name][1:]), seq, fused, launches, 2 * len(blocks))
    pieces["fc"] = (feat(512, h8, w8), net.fc, lambda x: T.fused_conv3x3(x, everything.fc_params), [(everything.fc_params, h8, w8)], 0)
    pieces["conv8s"] = (feat(256, h8, w8), lambda x: net.conv8s(torch.cat([x, x8s], 1)),
                        lambda x: T.fused_conv3x3(x, everything.conv8s_params, src2=x8s), [(everything.conv8s_params, h8, w8)], 0)

    variants, work = [], {}
    for name, (x, eager, fused, launches, nres) in pieces.items():
        flop = sum(conv_work(p, b, h, w)[0] for p, h, w in launches)
        nbytes = sum(conv_work(p, b, h, w)[1] for p, h, w in launches)
        if nres:   # a block's second launch reads its residual too
            nbytes += sum(2 * b * p.co * h * w for p, h, w in launches[1::2])
        work[name] = (flop, nbytes)
        src = torch.zeros(nbytes // 8, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)

        def path_a(_, x=x, fused=fused):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                fused(x)

        def path_b(_, x=x, eager=eager):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                eager(x)

        def path_c(_, src=src, dst=dst):   # half the bytes read and half written: a copy
            dst.copy_(src)
        variants += [(f"{name} (a) fused", path_a), (f"{name} (b) eager, autocast(bfloat16)", path_b), (f"{name} (c) device pass over the bytes", path_c)]

    im = torch.randn((b, 3, H, W), generator=g, device=dev)
    nets = {"eager": net, "FusedStemNet (default)": S.FusedStemNet(net), "FusedTrunkNet, all six pieces": everything,
            f"FusedTrunkNet, default (layers={T.DEFAULT_LAYERS})": T.FusedTrunkNet(net)}
    one = [None]
    for _, fn in variants:   # warm-up (and the convolution library's search)
        time_ms(fn, one, 2)
    t = {n: [] for n, _ in variants}
    for _ in range(args.rounds):
        for n, fn in variants:
            t[n].append(time_ms(fn, one, 2))
    med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
    selected = []
    for name in pieces:
        flop, nbytes = work[name]
        a, bb, c = (n for n, _ in variants if n.startswith(name + " "))
        say()
        say(f"== {name}: {len(pieces[name][3])} launches, {flop / 1e9:.0f} GFLOP per batch (MFMA-rate floor {flop / PEAK * 1e6:.0f} us), at least "
            f"{nbytes / 1e6:.0f} MB moved")
        for n in (a, bb, c):
            v = t[n]
            extra = f"  {flop / (med[n] * 1e-3) / 1e12:6.1f} TFLOP/s" if n != c else f"  {nbytes / (med[n] * 1e-3) / 1e9:7.1f} GB/s"
            say(f"  {n:48s} {med[n] * 1e3:10.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
        spread = max(t[bb]) - min(t[bb])
        ok = med[bb] - med[a] > spread
        selected += [name] if ok else []
        say(f"  (b) / (a) = {med[bb] / med[a]:.2f};  (a) / floor = {med[a] * 1e-3 / (flop / PEAK):.1f};  (a) / (c) = {med[a] / med[c]:.1f};  (b) - (a) = "
            f"{(med[bb] - med[a]) * 1e3:.1f} us against a spread of (b)'s rounds of {spread * 1e3:.1f} us: "
            f"{'fused by default' if ok else 'NOT fused by default (the piece stays reachable by naming it)'}")
    say()
    say(f"== the rule selects layers = {tuple(selected)};  pvnet_amd.trunk.DEFAULT_LAYERS = {T.DEFAULT_LAYERS}")
    nets[f"FusedTrunkNet, the selected pieces {tuple(selected)}"] = T.FusedTrunkNet(net, layers=tuple(selected))
    nvariants = []
    for name, m in nets.items():
        def run_net(_, m=m):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                m(im)
        nvariants.append((f"network, {name}", run_net))
    for _, fn in nvariants:
        time_ms(fn, one, 2)
    tn = {n: [] for n, _ in nvariants}
    for _ in range(args.rounds):
        for n, fn in nvariants:
            tn[n].append(time_ms(fn, one, 2))
    say()
    say("== the stand-in network under autocast(bfloat16)")
    base = sorted(tn["network, eager"])[args.rounds // 2]
    for n, _ in nvariants:
        v = tn[n]
        m = sorted(v)[len(v) // 2]
        say(f"  {n:90s} {m:8.2f} ms  ({min(v):.2f} .. {max(v):.2f})  {(m / base - 1) * 100:+6.1f} % of eager")
    network_error(say, dev, "FusedTrunkNet (all six pieces, stem and both stages)",
                  lambda net: T.FusedTrunkNet(net, layers=T.LAYERS, stem=True, stages=D.STAGES),
                  "FusedStemNet", lambda net: S.FusedStemNet(net, stem=True, stages=D.STAGES))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
