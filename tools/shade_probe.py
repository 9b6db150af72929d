"""Measures the shaded vertex-colour renderer (pvnet_amd/shade.py, libpvnet_shade.so) on one GPU and writes profiles/shade_probe.txt.

    python tools/shade_probe.py [--out profiles/shade_probe.txt] [--rounds 7] [--reps 20]

b = 32 images of 480 x 640, icospheres of 5 subdivisions (20 480 faces) each filling about a tenth of the frame at full size, m = 1, 3
and 13 instances per image (the workload of tools/depth_probe.py).  Medians over ``--rounds`` rounds in which the candidates alternate
(every round times every candidate once, ``--reps`` back-to-back calls between two events), all in one process:
  (a) render_color, flat, over a background image (rgb, depth and labels, caller-owned outputs and workspace)
  (b) render_depth on the same inputs
  (c) a bare device pass that clears 8 B and writes 8 B per pixel (three ``fill_``)
  (d) where the time of (a) goes by kernel, from one profiled stretch per m
  (e) from the workspace, the triangles that took the cooperative path; the covered share of the frame
and, once, the numpy restatement on one image at m = 3 (for scale, and equality with the device's), and the restatement's largest
difference to the float64 ray caster of tests/test_shade_cpu.py on that test's scenes."""
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

from pvnet_amd import depth, shade  # noqa: E402
from pvnet_amd import render  # noqa: E402
from raster_probe import make_poses, timed  # noqa: E402
from tests import shade_restatement as SR  # noqa: E402

B, H, W = 32, 480, 640
MS = (1, 3, 13)
BARE = "(c) bare pass: clear 8 B, write 8 B per pixel"


def colours(v):
    s = v / np.abs(v).max()
    return np.round(127.5 + 87.5 * np.stack([np.sin(2.1 * s[:, 0] + 0.3), np.sin(1.7 * s[:, 1] - 0.8), np.cos(2.4 * s[:, 2] + 0.5)], 1)).astype(np.uint8)


def oracle_lines():
    """the ray-caster comparison of tests/test_shade_cpu.py, on the CPU: the figures its docstring records"""
    from tests import test_shade_cpu as TS
    lines = []
    variants = (("the shaders as written", {}), ("light from the hit point", dict(vertex_light=False)),
                ("three-vector normal", dict(normal_w=False)), ("both terms removed", dict(vertex_light=False, normal_w=False)))
    for name, ((v, f, col, nrm), p) in sorted(TS.ORACLE_SCENES.items()):
        _, owner, _ = SR.instance_layers(v, f, p, TS.ORACLE_K, TS.ORACLE_H, TS.ORACLE_W)
        hits = TS.ray_hits(v, f, p, TS.ORACLE_K, TS.ORACLE_H, TS.ORACLE_W)
        geometry = (owner, hits, TS.interior_pixels(hits[0]))
        for shading in ("flat", "phong"):
            for what, switches in variants:
                for ambient, diff in TS.oracle_differences(name, shading, geometry, **switches).items():
                    lines.append(f"  restatement against the GLSL ray caster ({what:24s}), {name:6s} {shading:5s} ambient {ambient}: largest "
                                 f"difference {diff.max():6.3f} grey levels, mean {diff.mean():.3f}, 99.9 % below {np.quantile(diff, 0.999):6.3f}, "
                                 f"{int(geometry[2].sum())} of {int(hits[0].sum())} covered pixels compared")
            lines.append(f"  the test's bars, {name} {shading}: {TS.MEASURED_ORACLE[(name, shading)] + 1.0:.3f} grey levels against the shaders as "
                         f"written (the largest difference plus one), {TS.ROUNDING_BAR:.2f} with both terms removed")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    v, f = render.icosphere(5, 0.09)   # at z = 0.6: a disc of radius 86 px
    scales = np.linspace(0.5, 0.8, 13)
    col, nrm = colours(v), v / np.linalg.norm(v, axis=1, keepdims=True)
    meshes = [(v, f, col, nrm)] + [(v * s, f, col, nrm) for s in scales]   # mesh 0 for m = 1, meshes 1 .. 13 for m = 3 and 13
    table = shade.ColorMeshes(meshes)
    Kd = torch.from_numpy(K).to(dev)
    rgb_out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    d_out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    l_out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    zbuf = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    bare_out = torch.empty((B, H, W, 2), dtype=torch.float32, device=dev)
    background = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    setup = {}
    for m in MS:
        poses = torch.from_numpy(make_poses(rng, B * m, 0.12 if m == 1 else 0.2).reshape(B, m, 3, 4)).to(dev)
        ids = [0] if m == 1 else list(range(1, m + 1))
        setup[m] = (poses, ids, list(range(1, m + 1)),
                    torch.empty(shade.shade_workspace_bytes(B * m, B, H, W, table), dtype=torch.uint8, device=dev),
                    torch.empty(depth.depth_workspace_bytes(B * m, B, H, W, table), dtype=torch.uint8, device=dev))
    cands = {}
    for m in MS:
        poses, ids, labels, ws_s, ws_d = setup[m]
        cands[f"(a) render_color flat m = {m}"] = lambda p=poses, i=ids, lb=labels, ws=ws_s: shade.render_color(
            table, i, lb, p, Kd, H, W, shading="flat", background=background, out_rgb=rgb_out, out_depth=d_out, out_labels=l_out, workspace=ws)
        cands[f"(b) render_depth m = {m}"] = lambda p=poses, i=ids, lb=labels, ws=ws_d: depth.render_depth(
            table, i, lb, p, Kd, H, W, out_depth=d_out, out_labels=l_out, workspace=ws)
    cands[BARE] = lambda: (zbuf.fill_(-1), bare_out.fill_(0.0))
    for fn in cands.values():   # warm up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
    lines = [f"shade_probe: b = {B}, {H} x {W}, icospheres of {len(f)} faces, medians of {args.rounds} alternating rounds of {args.reps} "
             f"calls, {torch.cuda.get_device_name(0)}"]
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in med.items():
        lines.append(f"  {k:46s} {t:9.1f} us   (min {min(times[k]):.1f}, max {max(times[k]):.1f})")
    for m in MS:
        a, b = med[f"(a) render_color flat m = {m}"], med[f"(b) render_depth m = {m}"]
        lines.append(f"  m = {m:2d}: (a) / (b) = {a / b:.2f}   (a) - (b) = {a - b:.1f} us   (a) / (c) = {a / med[BARE]:.2f}")
    for m in MS:
        poses, ids, labels, ws_s, _ = setup[m]
        _, _, lab, visible = shade.render_color(table, ids, labels, poses, Kd, H, W, background=background, out_rgb=rgb_out, out_depth=d_out,
                                                out_labels=l_out, workspace=ws_s, return_visible=True)
        torch.cuda.synchronize()
        coop = int(ws_s[:4].view(torch.int32).cpu()[0])
        lines.append(f"  (e) m = {m:2d}: triangles on the cooperative path: {coop} of {B * m * len(f)}; "
                     f"{100.0 * float((lab != 0).float().mean()):.1f} % of the frame covered, {int(visible.sum())} visible pixels")
    try:
        from torch.profiler import ProfilerActivity, profile
        for m in MS:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(5):
                    cands[f"(a) render_color flat m = {m}"]()
                torch.cuda.synchronize()
            per = {e.key: e.device_time_total / max(e.count, 1) for e in prof.key_averages() if "shade_" in e.key}
            total = sum(per.values())
            for key, t in per.items():
                lines.append(f"  (d) m = {m:2d}: {key[:64]:64s} {t:9.1f} us per launch ({100.0 * t / total:4.1f} % of the kernels' time)")
    except Exception as ex:   # the profiler is an aid, not the measurement
        lines.append(f"  (d) by kernel: profiler unavailable ({type(ex).__name__})")
    poses, ids, labels, _, _ = setup[3]
    got = shade.render_color(table, ids, labels, poses[:1], Kd, H, W, background=background[:1], return_visible=True, return_status=True)
    t0 = time.perf_counter()
    p0 = poses[0].cpu().numpy()
    want = SR.render([table.mesh(k) for k in range(table.count)], [(ids[j], p0[j], K, 0, labels[j]) for j in range(3)], 1, H, W,
                     shading="flat", background=background[:1].cpu().numpy())
    equal = all(np.array_equal(a.cpu().numpy().reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))
                for a, b in zip(got, want))
    lines.append(f"  numpy restatement, one image at m = 3 {(time.perf_counter() - t0) * 1e6:9.0f} us   (equal to the device's, bit for bit: {equal})")
    lines += oracle_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
