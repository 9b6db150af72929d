"""Measures the fused head-metrics pass (pvnet_amd/validation.py, pvnet_head_metrics) on the GPU -> profiles/head_metrics_probe.txt.

    python tools/head_metrics_probe.py [--out FILE] [--rounds N]      # needs tools/ubench_hbm_read.bin (see that file's head)

For b = 1, 8, 32 at 480 x 640, vn = 9, float32 and bfloat16 predictions, int64 masks, with enough DISTINCT input sets cycled that
more than the 256 MiB Infinity Cache lies between two uses of a set:
  (a) the fused call: time (device events) and achieved GB/s over the bytes it must read (164 B per pixel with float32 predictions);
  (b) the torch composition of the three lines of the reference's NetWrapper.forward (cross-entropy, smooth-L1, precision / recall)
      on the same inputs in the same run, the variants alternating: what a user has today;
  (c) a bare read of the same number of bytes (tools/ubench_hbm_read.bin BYTES): the ceiling.
And the A/B of which loads are non-temporal (default: targets, weights and mask; none; all), for the head alone and for head + the
vote that reads the same predictions next.
"""
import argparse
import math
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvnet_amd import validation as V  # noqa: E402
from pvnet_amd import voting  # noqa: E402

H, W, VN, HN = 480, 640, 9, 512
CACHE = 256 << 20


def make_set(b, dtype, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    c = torch.rand((b, 2), generator=g, device=dev) * torch.tensor([W - 200.0, H - 200.0], device=dev) + 100.0
    mask = (((xx[None] - c[:, 0, None, None]) ** 2 + (yy[None] - c[:, 1, None, None]) ** 2) < 40.0 ** 2)
    kp = c[:, None, :] + (torch.rand((b, VN, 2), generator=g, device=dev) - 0.5) * 120.0
    dx = kp[:, :, 0, None, None] - xx[None, None]
    dy = kp[:, :, 1, None, None] - yy[None, None]
    n = torch.sqrt(dx * dx + dy * dy).clamp_min(1e-6)
    vertex = (torch.stack([dx / n, dy / n], 2).reshape(b, 2 * VN, H, W) * mask[:, None]).contiguous()
    vertex_pred = (vertex + 0.05 * torch.randn(vertex.shape, generator=g, device=dev)).to(dtype)
    seg_pred = torch.randn((b, 2, H, W), generator=g, device=dev)
    seg_pred[:, 1] += mask.float() * 6.0 - 3.0
    return (seg_pred.to(dtype), vertex_pred, mask.to(torch.int64), vertex, mask.float()[:, None].contiguous())


def torch_head(seg_pred, vertex_pred, mask, vertex, vertex_weights, criterion):
    """the torch composition a user runs today: cross-entropy per image, weighted smooth-L1 (sigma 1), precision and recall"""
    b = seg_pred.shape[0]
    loss_seg = criterion(seg_pred, mask).view(b, -1).mean(1)
    diff = vertex_weights * (vertex_pred - vertex)
    a = diff.abs()
    near = (a < 1.0).float()
    in_loss = diff.pow(2) * 0.5 * near + (a - 0.5) * (1.0 - near)
    loss_vertex = in_loss.view(b, -1).sum(1) / (vertex_pred.shape[1] * vertex_weights.view(b, -1).sum(1) + 1e-3)
    pred = torch.argmax(seg_pred, 1).float()
    tgt = mask.float()
    tp = (pred * tgt).view(b, -1).sum(1)
    fp = (pred * (1 - tgt)).view(b, -1).sum(1)
    fn = ((1 - pred) * tgt).view(b, -1).sum(1)
    return loss_seg, loss_vertex, (tp + 1) / (tp + fp + 1), (tp + 1) / (tp + fn + 1)


def time_ms(fn, sets, reps):
    """mean device time of fn over reps passes through the cycled sets (events around the whole window)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for r in range(reps):
        for s in sets:
            fn(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * len(sets))


def network_error(say, dev, label, make, other_label, make_other):
    """the fused network probes' last lines: the seeded stand-in under ``make(net)`` and ``make_other(net)`` against the eager float32
    network, under autocast(bfloat16)"""
    from tests import tail_cases as TC
    net, x = TC.standin()
    net, x = net.to(dev), x.to(dev)
    with torch.no_grad():
        ref = torch.cat(net(x), 1).double()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            eager = torch.cat(net(x), 1).double()
            fused = torch.cat(make(net)(x), 1).double()
            other = torch.cat(make_other(net)(x), 1).double()
    e, d = float((eager - ref).abs().max()), float((fused - ref).abs().max())
    say()
    say("== the seeded stand-in of tests/tail_cases.py, 1 x 3 x 32 x 48, autocast(bfloat16): largest difference to the eager float32 network")
    say(f"  eager e = {e:.4e};  {label} {d:.4e} = {d / e:.2f} e (the test's bar is 2 e);  {other_label} {float((other - ref).abs().max()):.4e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_metrics_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"head_metrics_probe: {torch.cuda.get_device_name(0)}, {H}x{W}, vn={VN}, C=2, int64 masks, sigma=1; times are means of device-event "
        f"windows, median over {args.rounds} alternating rounds (min..max)")
    criterion = torch.nn.CrossEntropyLoss(reduction="none")
    ubench = os.path.join(ROOT, "tools", "ubench_hbm_read.bin")
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
        esz = 2 if dtype == torch.bfloat16 else 4
        bpp = 2 * esz + 2 * VN * esz + 2 * VN * 4 + 4 + 8
        for b in (1, 8, 32):
            nbytes = b * H * W * bpp
            nsets = max(2, math.ceil(1.25 * CACHE / nbytes) + 1)
            sets = [make_set(b, dtype, dev, 1000 * b + k) for k in range(nsets)]
            ws = torch.empty(V.head_metrics_workspace_bytes(b, H, W), dtype=torch.uint8, device=dev)
            out = (torch.empty((b, 4), dtype=torch.float64, device=dev), torch.empty((b, 3), dtype=torch.int64, device=dev),
                   torch.empty((b,), dtype=torch.int32, device=dev))
            L = voting.vote_layout(b, H, W, VN, HN, 30000)
            vws = torch.empty(L.total_bytes, dtype=torch.uint8, device=dev)
            kp = torch.empty((b, VN, 2), device=dev)

            def fused(flags):
                return lambda s: V.head_metrics_device(*s, out=out, workspace=ws, flags=flags)

            def vote(s):
                voting.ransac_voting_layer_v3_from_logits(s[0], voting._field_view(s[1]), HN, inlier_thresh=0.99, seed=7, workspace=vws,
                                                          out=kp, concurrent=False)

            def with_vote(flags):
                f = fused(flags)

                def run(s):
                    f(s)
                    vote(s)
                return run

            variants = [("fused (targets nt)", fused(0)), ("fused (no nt)", fused(V.HEAD_F_NT_NONE)), ("fused (all nt)", fused(V.HEAD_F_NT_ALL)),
                        ("torch composition", lambda s: torch_head(*s, criterion)), ("vote alone", vote),
                        ("fused (targets nt) + vote", with_vote(0)), ("fused (no nt) + vote", with_vote(V.HEAD_F_NT_NONE)),
                        ("fused (all nt) + vote", with_vote(V.HEAD_F_NT_ALL))]
            # the two agree before either is timed
            got = V.head_metrics_device(*sets[0])[0].float()
            want = torch.stack(torch_head(*sets[0], criterion), 1).float()
            agree = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
            reps = max(1, 64 // (b * nsets))
            for _, fn in variants:   # warm-up: every shape, every variant
                time_ms(fn, sets, 1)
            t = {n: [] for n, _ in variants}
            for _ in range(args.rounds):
                for n, fn in variants:
                    t[n].append(time_ms(fn, sets, reps))
            med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
            r = subprocess.run([ubench, str(nbytes)], capture_output=True, text=True, timeout=300)
            bare = next((ln for ln in r.stdout.splitlines() if ln.startswith("bare_read")), None)
            assert r.returncode == 0 and bare, (r.returncode, r.stdout[-500:], r.stderr[-500:])
            bare_us = float(bare.split("avg_us")[1].split()[0])
            say()
            say(f"== {name} predictions, b = {b}: {bpp} B/pixel, {nbytes / 1e6:.1f} MB per call, {nsets} input sets cycled "
                f"({nsets * nbytes / 1e6:.0f} MB), fused vs torch max relative difference {agree:.1e}")
            for n, _ in variants:
                v = t[n]
                extra = f"  {nbytes / (med[n] * 1e-3) / 1e9:7.0f} GB/s over the compulsory bytes" if "vote" not in n else ""
                say(f"  {n:28s} {med[n] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
            say(f"  {'(c) bare read, same bytes':28s} {bare_us:9.1f} us  {nbytes / (bare_us * 1e-6) / 1e9:7.0f} GB/s   [{bare.strip()}]")
            a, bt = med["fused (targets nt)"], med["torch composition"]
            say(f"  (a)/(b) fused / torch = {a / bt:.3f} (torch / fused = {bt / a:.1f}x);  (a)/(c) fused / bare read = {a * 1e3 / bare_us:.2f}")
            del sets, vws, ws
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
