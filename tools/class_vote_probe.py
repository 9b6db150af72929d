"""Measures the per-class vote (voting.ransac_voting_layer_v2) -> profiles/class_vote_probe.txt.

    python tools/class_vote_probe.py [--out FILE] [--rounds N] [--b B]

One MI355X, b = 32, 480 x 640, vn = 9, hn = 1024, thresh 0.99, int64 labels: three discs of R = 40 per image (labels 1, 2, 3), voted
with class_num = 4 and with class_num = 14 (the same discs: classes 4 .. 13 are empty virtual images).  Four copies of the labels are
cycled (more than the 256 MiB Infinity Cache between two uses of one), device events on one stream, the variants alternating, medians of the
rounds:
  (a) ``ransac_voting_layer_v2`` (the class split, then the layer's other launches over B = b (class_num - 1) virtual images);
  (b) ``ransac_voting_layer_v3`` on the materialised batch, INCLUDING building its B masks (one comparison kernel); its field,
      every image's repeated class_num - 1 times, is built beforehand and not timed;
  (c) class_num - 1 calls of ``ransac_voting_layer_v3`` on ``labels == k + 1``, building each mask included;
  (d) ``pvnet_class_split`` alone; and, back to back on ONE copy of the labels, next to the mask kernel of ``ransac_voting_layer_v3``
      on the same label bytes (b images, a binary int64 mask: ``stage_repeat_ms``, which re-launches on one mask).
Per stage: ``stage_times`` of (b)'s call -- its compaction, hypothesis, scoring and refinement launches are the launches (a) runs.
No threshold: the figures are reported as they come.
"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pvnet_amd import _abi, voting  # noqa: E402
from head_metrics_probe import H, W, VN, time_ms  # noqa: E402

HN, THRESH, R = 1024, 0.99, 40.0


def make_labels_and_field(b, dev, seed):
    """labels [b,H,W] int64 with three discs of radius R (labels 1, 2, 3) and the field [b,H,W,VN,2] whose disc pixels point
    at their class's key-points (N(0, 0.05) added), planar in memory as a backbone emits it"""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    labels = torch.zeros((b, H, W), dtype=torch.int64, device=dev)
    planar = torch.zeros((b, 2 * VN, H, W), device=dev)
    for k in range(3):   # three columns of the image, one disc in each: no overlap
        cx = torch.rand((b,), generator=g, device=dev) * (W / 3 - 2 * R - 2) + R + 1 + k * W / 3
        cy = torch.rand((b,), generator=g, device=dev) * (H - 2 * R - 2) + R + 1
        disc = ((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2) < R * R
        labels[disc] = k + 1
        kp = torch.stack([cx, cy], 1)[:, None, :] + (torch.rand((b, VN, 2), generator=g, device=dev) - 0.5) * 120.0
        dx, dy = kp[:, :, 0, None, None] - xx[None, None], kp[:, :, 1, None, None] - yy[None, None]
        n = torch.sqrt(dx * dx + dy * dy).clamp_min(1e-6)
        planar += torch.stack([dx / n, dy / n], 2).reshape(b, 2 * VN, H, W) * disc[:, None]
    planar += 0.05 * torch.randn(planar.shape, generator=g, device=dev)
    return labels, planar.permute(0, 2, 3, 1).view(b, H, W, VN, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_vote_probe.txt"))
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
    say(f"class_vote_probe: {torch.cuda.get_device_name(0)}, b={b}, {H}x{W}, vn={VN}, hn={HN}, thresh {THRESH}, int64 labels, three discs of "
        f"R={R:.0f}; times are means of device-event windows, median over {args.rounds} alternating rounds (min..max)")
    labels, vertex = make_labels_and_field(b, dev, 500)
    sets = [labels] + [labels.clone() for _ in range(3)]   # the same images at four addresses
    kw = dict(inlier_thresh=THRESH, seed=3)
    clib = _abi.load_classes_library()
    for cn in (4, 14):
        nk = cn - 1
        B = b * nk
        L = voting.vote_layout(B, H, W, VN, HN, 30000)
        ws = torch.empty(L.total_bytes, dtype=torch.uint8, device=dev)
        ws1 = torch.empty(voting.vote_layout(b, H, W, VN, HN, 30000).total_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((b, nk, VN, 2), device=dev)
        out1 = torch.empty((b, VN, 2), device=dev)
        rep = vertex.repeat_interleave(nk, dim=0)                       # (b)'s field: not timed
        ks = torch.arange(1, cn, device=dev).view(1, nk, 1, 1)

        def path_a(labels):
            voting.ransac_voting_layer_v2(labels, vertex, cn, HN, workspace=ws, out=out, **kw)

        def path_b(labels):
            masks = (labels[:, None] == ks).view(B, H, W)
            voting.ransac_voting_layer_v3(masks, rep, HN, workspace=ws, out=out.view(B, VN, 2), concurrent=False, **kw)

        def path_c(labels):
            for k in range(nk):
                voting.ransac_voting_layer_v3(labels == k + 1, vertex, HN, workspace=ws1, out=out1, concurrent=False, **kw)

        base = ws.data_ptr()
        tail = [cn, b, H, W, 30000, C.c_uint64(3), 0, C.c_void_p(base + L.off_bits), C.c_void_p(base + L.off_seg + 4 * B * L.nseg),
                C.c_void_p(base + L.off_seg + (8 * B * L.nseg + 15) // 16 * 16), None]

        def path_d(labels):
            tail[-1] = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = clib.pvnet_class_split(*voting._mask_part(labels), *tail)
            assert rc == 0, rc

        variants = [("(a) ransac_voting_layer_v2", path_a), ("(b) v3, materialised batch + its masks", path_b),
                    (f"(c) {nk} x v3 on labels == k + 1", path_c), ("(d) pvnet_class_split alone", path_d)]
        for _, fn in variants:
            time_ms(fn, sets, 1)
        path_a(sets[-1])
        ref = out.clone()
        out.zero_()
        path_b(sets[-1])
        torch.cuda.synchronize()
        same = torch.equal(ref, out)
        t = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, fn in variants:
                t[n].append(time_ms(fn, sets, 2))
        med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
        say()
        say(f"== class_num = {cn}: B = {B} virtual images, workspace {L.total_bytes / 1e6:.0f} MB, labels {b * H * W * 8 / 1e6:.1f} MB per batch; "
            f"(a) equals (b) bit for bit on the last set: {same}")
        for n, _ in variants:
            v = t[n]
            say(f"  {n:44s} {med[n] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
        a, bb, c, d = (v[0] for v in variants)
        say(f"  (a) / (b) = {med[a] / med[bb]:.3f};  (a) / (c) = {med[a] / med[c]:.3f};  (a) < (b): {med[a] < med[bb]};  (a) < (c): {med[a] < med[c]}")
        k1 = voting.stage_repeat_ms((sets[0] != 0).to(torch.int64), vertex, HN, THRESH, stage="mask_bits", repeats=50)
        warm = sorted(time_ms(path_d, sets[:1], 50) for _ in range(args.rounds))[args.rounds // 2]
        say(f"  (d) next to the mask kernel of v3 on the same bytes (b = {b}, a binary int64 mask), both as 50 back-to-back launches on ONE "
            f"copy of the labels (78.6 MB stay in the Infinity Cache): {warm * 1e3:.1f} us against {k1 * 1e3:.1f} us; (d) above reads cycled copies")
        masks = (sets[0][:, None] == ks).view(B, H, W)
        _, st = voting.ransac_voting_layer_v3(masks, rep, HN, workspace=ws, stage_times=True, concurrent=False, **kw)
        _, st1 = voting.ransac_voting_layer_v3(sets[0] == 1, vertex, HN, workspace=ws1, stage_times=True, concurrent=False, **kw)
        say("  per stage, one profiled call (events between the launches), us:  " +
            "  ".join(f"{n} {st[n] * 1e3:.1f}" for n in voting.STAGE_NAMES if n != "subsample"))
        say(f"  the same for ONE class (b = {b}, labels == 1):                      " +
            "  ".join(f"{n} {st1[n] * 1e3:.1f}" for n in voting.STAGE_NAMES if n != "subsample"))
        del ws, ws1, rep, masks, out, out1
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
