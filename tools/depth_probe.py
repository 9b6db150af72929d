"""Measures the z-buffered mesh renderer (pvnet_amd/depth.py, libpvnet_depth.so) on one GPU and writes profiles/depth_probe.txt.

    python tools/depth_probe.py [--out profiles/depth_probe.txt] [--rounds 7] [--reps 20]

b = 32 images of 480 x 640, icospheres of 5 subdivisions (20 480 faces) each filling about a tenth of the frame at full size, m = 1, 3
and 13 instances per image (the workload of tools/raster_probe.py).  Medians over ``--rounds`` rounds in which the candidates alternate
(every round times every candidate once, ``--reps`` back-to-back calls between two events), all in one process:
  (a) render_depth (depth and labels, caller-owned outputs and workspace)
  (b) render_labels at the same m: painter's composition, what the z-buffer replaces
  (c) a bare device pass that clears 8 B and writes 5 B per pixel (three ``fill_``)
  (d) where the time of (a) goes by kernel, from one profiled stretch per m
  (e) from the workspace, the triangles that took the cooperative path
and, once, the numpy restatement on one image at m = 3 (for scale, and equality with the device's)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pvnet_amd import depth, render  # noqa: E402
from raster_probe import make_poses, timed  # noqa: E402
from tests import depth_restatement as DR  # noqa: E402

B, H, W = 32, 480, 640
MS = (1, 3, 13)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    v, f = render.icosphere(5, 0.09)   # at z = 0.6: a disc of radius 86 px
    scales = np.linspace(0.5, 0.8, 13)
    meshes = [(v, f)] + [(v * s, f) for s in scales]   # mesh 0 for m = 1, meshes 1 .. 13 for m = 3 and 13, as tools/raster_probe.py
    table = render.DeviceMeshes(meshes)
    Kd = torch.from_numpy(K).to(dev)
    d_out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    l_out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    p_out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    zbuf = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    setup = {}
    for m in MS:
        poses = torch.from_numpy(make_poses(rng, B * m, 0.12 if m == 1 else 0.2).reshape(B, m, 3, 4)).to(dev)
        ids = [0] if m == 1 else list(range(1, m + 1))
        setup[m] = (poses, ids, list(range(1, m + 1)),
                    torch.empty(depth.depth_workspace_bytes(B * m, B, H, W, table), dtype=torch.uint8, device=dev),
                    torch.empty(render.raster_workspace_bytes(B * m, H, W, table, B), dtype=torch.uint8, device=dev))
    cands = {}
    for m in MS:
        poses, ids, labels, ws_d, ws_r = setup[m]
        cands[f"(a) render_depth m = {m}"] = lambda p=poses, i=ids, lb=labels, ws=ws_d: depth.render_depth(
            table, i, lb, p, Kd, H, W, out_depth=d_out, out_labels=l_out, workspace=ws)
        cands[f"(b) render_labels m = {m}"] = lambda p=poses, i=ids, lb=labels, ws=ws_r: render.render_labels(
            table, i, lb, p, Kd, H, W, out=p_out, workspace=ws)
    cands["(c) bare pass: clear 8 B, write 5 B per pixel"] = lambda: (zbuf.fill_(-1), d_out.fill_(0.0), l_out.fill_(0))
    for fn in cands.values():   # warm up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
    lines = [f"depth_probe: b = {B}, {H} x {W}, icospheres of {len(f)} faces, medians of {args.rounds} alternating rounds of {args.reps} "
             f"calls, {torch.cuda.get_device_name(0)}"]
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in med.items():
        lines.append(f"  {k:46s} {t:9.1f} us   (min {min(times[k]):.1f}, max {max(times[k]):.1f})")
    bare = med["(c) bare pass: clear 8 B, write 5 B per pixel"]
    for m in MS:
        a, b = med[f"(a) render_depth m = {m}"], med[f"(b) render_labels m = {m}"]
        lines.append(f"  m = {m:2d}: (a) / (b) = {a / b:.2f}   (a) / (c) = {a / bare:.2f}")
    for m in MS:
        poses, ids, labels, ws_d, _ = setup[m]
        _, lab, visible = depth.render_depth(table, ids, labels, poses, Kd, H, W, out_depth=d_out, out_labels=l_out, workspace=ws_d,
                                             return_visible=True)
        torch.cuda.synchronize()
        coop = int(ws_d[:4].view(torch.int32).cpu()[0])
        painted = render.render_labels(table, ids, labels, poses, Kd, H, W)
        lines.append(f"  (e) m = {m:2d}: triangles on the cooperative path: {coop} of {B * m * len(f)}; {100.0 * float((lab != 0).float().mean()):.1f} % "
                     f"of the frame covered, {int(visible.sum())} visible pixels; {int((painted != lab).sum())} pixels differ from "
                     f"render_labels under centroid order")
    try:
        from torch.profiler import ProfilerActivity, profile
        for m in MS:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(5):
                    cands[f"(a) render_depth m = {m}"]()
                torch.cuda.synchronize()
            for e in prof.key_averages():
                if "depth_" in e.key:
                    lines.append(f"  (d) m = {m:2d}: {e.key[:64]:64s} {e.device_time_total / max(e.count, 1):9.1f} us per launch "
                                 f"({e.count} launches)")
    except Exception as ex:   # the profiler is an aid, not the measurement
        lines.append(f"  (d) by kernel: profiler unavailable ({type(ex).__name__})")
    poses, ids, labels, ws_d, _ = setup[3]
    got = depth.render_depth(table, ids, labels, poses[:1], Kd, H, W, return_visible=True, return_status=True)
    t0 = time.perf_counter()
    p0 = poses[0].cpu().numpy()
    want = DR.render(meshes, [(ids[j], p0[j], K, 0, labels[j]) for j in range(3)], 1, H, W)
    equal = all(np.array_equal(a.cpu().numpy().reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))
                for a, b in zip(got, want))
    lines.append(f"  numpy restatement, one image at m = 3 {(time.perf_counter() - t0) * 1e6:9.0f} us   (equal to the device's, bit for bit: {equal})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
