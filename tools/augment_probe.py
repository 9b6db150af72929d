"""Measures the augmentation on the device (pvnet_amd/augment.py: augment_batch) -> profiles/augment_probe.txt.

    python tools/augment_probe.py [--out FILE] [--rounds N] [--b B]

At b = 32, 480 x 640 -> 480 x 640, vn = 9, uint8 masks in and out, float32 and bfloat16 images, default configuration, with enough
DISTINCT input sets cycled that more than the 256 MiB Infinity Cache lies between two uses of a set, in one process, device events on
one stream, the variants alternating:
  (a) ``augment_batch`` into preallocated outputs (uniforms packed beforehand: the call is the two launches);
  (b) a bare device pass over the same bytes: 4 B per pixel copied, the rest of the output's bytes filled (flat buffers);
  (c) the eager torch composition of ONE composed map: ``affine_grid`` + ``grid_sample`` (bilinear image, nearest mask) + normalise
      -- without the planning, the rectangle or the key-points, so it is charged less than (a) does;
  (d) the host-to-device copy (pinned memory) of what the reference's loader ships, a float32 image and an int64 mask, against the
      uint8 image and mask that (a) takes.
No threshold: the ratio (a)/(b) is reported.
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
from head_metrics_probe import H, W, VN, CACHE, time_ms  # noqa: E402


def make_set(b, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    c = torch.rand((b, 2), generator=g, device=dev) * torch.tensor([W - 200.0, H - 200.0], device=dev) + 100.0
    mask = (((xx[None] - c[:, 0, None, None]) ** 2 + (yy[None] - c[:, 1, None, None]) ** 2) < 40.0 ** 2).to(torch.uint8)
    rgb = torch.randint(0, 256, (b, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    hc = torch.cat([c[:, None, :].double() + (torch.rand((b, VN, 2), generator=g, device=dev, dtype=torch.float64) - 0.5) * 120.0,
                    torch.ones((b, VN, 1), dtype=torch.float64, device=dev)], 2)
    return rgb, mask, hc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_probe.txt"))
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
    cfg = A.AugmentConfig()
    say(f"augment_probe: {torch.cuda.get_device_name(0)}, b={b}, {H}x{W} -> {H}x{W}, vn={VN}, uint8 masks, default configuration; times "
        f"are means of device-event windows, median over {args.rounds} alternating rounds (min..max)")
    mean = torch.tensor(A.MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(A.STD, device=dev).view(1, 3, 1, 1)
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
        esz = 2 if dtype == torch.bfloat16 else 4
        read_b, write_b = 4, 3 * esz + 1
        nbytes = b * H * W * (read_b + write_b)
        nsets = max(2, math.ceil(1.25 * CACHE / nbytes) + 1)
        sets = []
        for k in range(nsets):
            rgb, mask, hc = make_set(b, dev, 1000 * b + k)
            packed = A.pack_uniforms(A.draw_uniforms(b, torch.Generator().manual_seed(k)), cfg, dev)
            ang = (torch.rand(b, device=dev) - 0.5) * (math.pi / 3)
            theta = torch.stack([torch.stack([ang.cos() * 0.8, -ang.sin() * 0.8, torch.zeros_like(ang)], 1),
                                 torch.stack([ang.sin() * 0.8, ang.cos() * 0.8, torch.zeros_like(ang)], 1)], 1)
            sets.append((rgb, mask, hc, packed, theta))
        out = (torch.empty((b, 3, H, W), dtype=dtype, device=dev), torch.empty((b, H, W), dtype=torch.uint8, device=dev),
               torch.empty((b, VN, 3), dtype=torch.float64, device=dev), torch.empty((b,), dtype=torch.int32, device=dev))
        ws = torch.empty(A.augment_workspace_bytes(b), dtype=torch.uint8, device=dev)
        src_flat = torch.empty(b * H * W * read_b, dtype=torch.uint8, device=dev)
        dst_flat = torch.empty(b * H * W * write_b, dtype=torch.uint8, device=dev)
        host_ref = (torch.empty((b, 3, H, W), dtype=torch.float32).pin_memory(), torch.empty((b, H, W), dtype=torch.int64).pin_memory())
        host_u8 = (torch.empty((b, H, W, 3), dtype=torch.uint8).pin_memory(), torch.empty((b, H, W), dtype=torch.uint8).pin_memory())
        dev_ref = tuple(torch.empty_like(t, device=dev) for t in host_ref)
        dev_u8 = tuple(torch.empty_like(t, device=dev) for t in host_u8)

        def path_a(s):
            A.augment_batch(s[0], s[1], s[2], H, W, cfg, s[3], 7, out_dtype=dtype, out=out, workspace=ws)

        def path_b(s):   # read_b bytes per pixel read and written by a copy, the rest of the write_b written by a fill
            dst_flat[:src_flat.numel()].copy_(src_flat)
            dst_flat[src_flat.numel():].zero_()

        def path_c(s):
            grid = torch.nn.functional.affine_grid(s[4], (b, 3, H, W), align_corners=False)
            img = torch.nn.functional.grid_sample(s[0].permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            m = torch.nn.functional.grid_sample(s[1][:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=False)
            out[0].copy_((img.round() / 255.0 - mean) / std)
            out[1].copy_(m[:, 0])

        def copy_ref(s):
            dev_ref[0].copy_(host_ref[0], non_blocking=True)
            dev_ref[1].copy_(host_ref[1], non_blocking=True)

        def copy_u8(s):
            dev_u8[0].copy_(host_u8[0], non_blocking=True)
            dev_u8[1].copy_(host_u8[1], non_blocking=True)

        variants = [("(a) augment_batch", path_a), ("(b) device copy of the same bytes", path_b),
                    ("(c) eager affine_grid + grid_sample + normalise", path_c),
                    ("(d) host-to-device: float32 image + int64 mask", copy_ref), ("(d) host-to-device: uint8 image + uint8 mask", copy_u8)]
        reps = max(1, 64 // (b * nsets))
        for _, fn in variants:   # warm-up: every shape, every variant
            time_ms(fn, sets, 1)
        t = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, fn in variants:
                t[n].append(time_ms(fn, sets, reps))
        med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
        say()
        say(f"== {name} image: {read_b} B/pixel read, {write_b} B/pixel written, {nbytes / 1e6:.0f} MB per batch; {nsets} input sets cycled; "
            f"status of the last batch: {sorted(set(out[3].tolist()))}")
        sizes = {"(d) host-to-device: float32 image + int64 mask": sum(x.numel() * x.element_size() for x in host_ref),
                 "(d) host-to-device: uint8 image + uint8 mask": sum(x.numel() * x.element_size() for x in host_u8),
                 "(a) augment_batch": nbytes, "(b) device copy of the same bytes": nbytes}
        for n, _ in variants:
            v = t[n]
            extra = f"  {sizes[n] / (med[n] * 1e-3) / 1e9:7.1f} GB/s, {sizes[n] / 1e6:.0f} MB" if n in sizes else ""
            say(f"  {n:50s} {med[n] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
        a, bb, c = variants[0][0], variants[1][0], variants[2][0]
        say(f"  (a) / (b) = {med[a] / med[bb]:.2f};  (c) / (a) = {med[c] / med[a]:.2f};  spread of (a) {(max(t[a]) - min(t[a])) / med[a] * 100:.1f} %")
        del sets, out, ws, src_flat, dst_flat, host_ref, host_u8, dev_ref, dev_u8
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
