"""Measures the colour jitter on the device (pvnet_amd/color.py) -> profiles/color_probe.txt.

    python tools/color_probe.py [--out FILE] [--rounds N] [--b B]

At b = 32, 480 x 640 -> 480 x 640, vn = 9, uint8 masks in and out, float32 and bfloat16 images, the default configurations, with enough
DISTINCT input sets cycled that more than the 256 MiB Infinity Cache lies between two uses of a set, in one process, device events on
one stream, the variants alternating:
  (a) ``augment_batch`` at this commit, into preallocated outputs (uniforms packed beforehand);
  (b) ``augment_jitter_batch``, likewise (the plan, the warp to uint8, the statistics, the apply);
  (c) ``jitter_batch`` alone on the source image (the statistics, the apply);
  (d) a bare device pass over the bytes that (c) moves: 3 B per pixel read twice, the image's bytes written (flat buffers: two
      copies of the source's bytes, a fill of the rest).
No threshold: (b) - (a) and (c) / (d) are reported.
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pvnet_amd import augment as A  # noqa: E402
from pvnet_amd import color as K  # noqa: E402
from augment_probe import make_set  # noqa: E402
from head_metrics_probe import H, W, VN, CACHE, time_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_probe.txt"))
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
    cfg, jcfg = A.AugmentConfig(), K.ColorJitterConfig()
    say(f"color_probe: {torch.cuda.get_device_name(0)}, b={b}, {H}x{W} -> {H}x{W}, vn={VN}, uint8 masks, default configurations; times "
        f"are means of device-event windows, median over {args.rounds} alternating rounds (min..max)")
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
        esz = 2 if dtype == torch.bfloat16 else 4
        nbytes_a = b * H * W * (4 + 3 * esz + 1)       # what (a) moves
        nbytes_c = b * H * W * (3 + 3 + 3 * esz)       # what (c) moves: the source twice, the image once
        nsets = max(2, math.ceil(1.25 * CACHE / nbytes_a) + 1)
        sets = []
        for k in range(nsets):
            rgb, mask, hc = make_set(b, dev, 1000 * b + k)
            packed = A.pack_uniforms(A.draw_uniforms(b, torch.Generator().manual_seed(k)), cfg, dev)
            ju = K.draw_jitter_uniforms(b, torch.Generator().manual_seed(100 + k)).to(dev)
            sets.append((rgb, mask, hc, packed, ju))
        out = (torch.empty((b, 3, H, W), dtype=dtype, device=dev), torch.empty((b, H, W), dtype=torch.uint8, device=dev),
               torch.empty((b, VN, 3), dtype=torch.float64, device=dev), torch.empty((b,), dtype=torch.int32, device=dev))
        ws_a = torch.empty(A.augment_workspace_bytes(b), dtype=torch.uint8, device=dev)
        ws_b = torch.empty(K.color_workspace_bytes(b, H, W), dtype=torch.uint8, device=dev)
        ws_c = torch.empty(K.color_workspace_bytes(b), dtype=torch.uint8, device=dev)
        src_flat = torch.empty(b * H * W * 3, dtype=torch.uint8, device=dev)
        dst_flat = torch.empty(b * H * W * 3 * esz, dtype=torch.uint8, device=dev)

        def path_a(s):
            A.augment_batch(s[0], s[1], s[2], H, W, cfg, s[3], 7, out_dtype=dtype, out=out, workspace=ws_a)

        def path_b(s):
            K.augment_jitter_batch(s[0], s[1], s[2], H, W, cfg, jcfg, s[3], s[4], 7, out_dtype=dtype, out=out, workspace=ws_b)

        def path_c(s):
            K.jitter_batch(s[0], jcfg, s[4], out_dtype=dtype, out=out[0], workspace=ws_c)

        def path_d(s):   # the source's bytes read twice and written twice, the rest of the image's bytes filled
            n = src_flat.numel()
            dst_flat[:n].copy_(src_flat)
            dst_flat[n:2 * n].copy_(src_flat)
            dst_flat[2 * n:].zero_()

        variants = [("(a) augment_batch", path_a), ("(b) augment_jitter_batch", path_b), ("(c) jitter_batch", path_c),
                    ("(d) device pass over the bytes of (c)", path_d)]
        reps = max(1, 64 // (b * nsets))
        for _, fn in variants:   # warm-up: every shape, every variant
            time_ms(fn, sets, 1)
        t = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, fn in variants:
                t[n].append(time_ms(fn, sets, reps))
        med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
        say()
        say(f"== {name} image: (a) moves {nbytes_a / 1e6:.0f} MB per batch, (c) {nbytes_c / 1e6:.0f} MB; {nsets} input sets cycled; status of the "
            f"last batch: {sorted(set(out[3].tolist()))}")
        sizes = {"(a) augment_batch": nbytes_a, "(c) jitter_batch": nbytes_c, "(d) device pass over the bytes of (c)": nbytes_c}
        for n, _ in variants:
            v = t[n]
            extra = f"  {sizes[n] / (med[n] * 1e-3) / 1e9:7.1f} GB/s, {sizes[n] / 1e6:.0f} MB" if n in sizes else ""
            say(f"  {n:42s} {med[n] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
        a, bb, c, d = (v[0] for v in variants)
        say(f"  (b) - (a) = {(med[bb] - med[a]) * 1e3:.1f} us ({(med[bb] / med[a] - 1) * 100:+.1f} %);  (c) / (d) = {med[c] / med[d]:.2f};  "
            f"spread of (b) {(max(t[bb]) - min(t[bb])) / med[bb] * 100:.1f} %")
        del sets, out, ws_a, ws_b, ws_c, src_flat, dst_flat
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
