"""Measures the mesh rasteriser (pvnet_amd/render.py, libpvnet_raster.so) on one GPU and writes profiles/raster_probe.txt.

    python tools/raster_probe.py [--out profiles/raster_probe.txt] [--rounds 7] [--reps 20]

b = 32 images of 480 x 640, an icosphere of 5 subdivisions (20 480 faces) filling about a tenth of the frame.  Medians over
``--rounds`` rounds in which the candidates alternate (every round times every candidate once, ``--reps`` back-to-back calls between
two events):
  (a) render_masks                      (b) a bare device pass writing the same 9.8 MB (``out.fill_``)
  (c) stage R alone on resident triangles (rasterize_triangles)
  (d) the numpy restatement on one image, for scale only (once)
  (e) render_labels with m = 3 and m = 13
and, from one profiled call of (a), where the time goes by kernel; from the workspace, the share of triangles that took the
cooperative path."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvnet_amd import render  # noqa: E402
from tests import raster_restatement as RS  # noqa: E402
from tests.render_cases import rotation  # noqa: E402

B, H, W = 32, 480, 640


def make_poses(rng, n, spread=0.12):
    out = []
    for _ in range(n):
        t = np.array([rng.uniform(-spread, spread), rng.uniform(-spread * 0.7, spread * 0.7), rng.uniform(0.55, 0.65)])
        out.append(np.concatenate([rotation(rng.normal(size=3), rng.uniform(0, np.pi)), t[:, None]], 1))
    return np.stack(out)


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1000.0 / reps   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    v, f = render.icosphere(5, 0.09)   # at z = 0.6: a disc of radius 86 px, 23 000 of 307 200 pixels
    table = render.DeviceMeshes([(v, f)])
    many = render.DeviceMeshes([(v * s, f) for s in np.linspace(0.5, 0.8, 13)])
    poses = torch.from_numpy(make_poses(rng, B)).to(dev)
    Kd = torch.from_numpy(K).to(dev)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    ws = torch.empty(render.raster_workspace_bytes(B, H, W, table), dtype=torch.uint8, device=dev)
    tri = render.project_triangles(table, 0, poses, Kd)
    lab = {}
    for m in (3, 13):
        lab[m] = (torch.from_numpy(make_poses(rng, B * m, 0.2).reshape(B, m, 3, 4)).to(dev),
                  torch.empty(render.raster_workspace_bytes(B * m, H, W, many, B), dtype=torch.uint8, device=dev))
    cands = {
        "(a) render_masks": lambda: render.render_masks(table, 0, poses, Kd, H, W, out=out, workspace=ws),
        "(b) bare pass writing 9.8 MB": lambda: out.fill_(1),
        "(c) stage R on resident triangles": lambda: render.rasterize_triangles(tri, H, W, out=out, workspace=ws),
        "(e) render_labels m = 3": lambda: render.render_labels(many, list(range(3)), list(range(1, 4)), lab[3][0], Kd, H, W, out=out,
                                                                workspace=lab[3][1]),
        "(e) render_labels m = 13": lambda: render.render_labels(many, list(range(13)), list(range(1, 14)), lab[13][0], Kd, H, W, out=out,
                                                                 workspace=lab[13][1]),
    }
    for fn in cands.values():   # warm up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
    lines = [f"raster_probe: b = {B}, {H} x {W}, icosphere of {len(f)} faces, medians of {args.rounds} alternating rounds of {args.reps} calls, "
             f"{torch.cuda.get_device_name(0)}"]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, t in med.items():
        lines.append(f"  {k:36s} {t:9.1f} us   (min {min(times[k]):.1f}, max {max(times[k]):.1f})")
    lines.append(f"  (a) / (b) = {med['(a) render_masks'] / med['(b) bare pass writing 9.8 MB']:.2f}")
    cands["(a) render_masks"]()
    torch.cuda.synchronize()
    coop = int(ws[:4].view(torch.int32).cpu()[0])
    covered = float(out.float().mean())
    lines.append(f"  triangles on the cooperative path: {coop} of {B * len(f)} ({100.0 * coop / (B * len(f)):.3f} %); the silhouettes cover "
                 f"{100.0 * covered:.1f} % of the frame")
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                cands["(a) render_masks"]()
            torch.cuda.synchronize()
        for e in prof.key_averages():
            if "kernel" in e.key and ("pvd" in e.key or "raster" in e.key or "setup" in e.key or "expand" in e.key or "triangle" in e.key
                                      or "clear" in e.key):
                lines.append(f"  by kernel: {e.key[:70]:70s} {e.device_time_total / max(e.count, 1):9.1f} us per launch ({e.count} launches)")
    except Exception as ex:   # the profiler is an aid, not the measurement
        lines.append(f"  by kernel: profiler unavailable ({type(ex).__name__})")
    t0 = time.perf_counter()
    want = RS.render([(v, f)], [(0, poses[0].cpu().numpy(), K, 0, 1)], 1, H, W)[0]
    lines.append(f"  (d) numpy restatement, one image      {(time.perf_counter() - t0) * 1e6:9.0f} us   (equal to the device's: "
                 f"{bool(np.array_equal(want[0], out[0].cpu().numpy()))})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
