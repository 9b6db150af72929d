"""Measures the textured renderer (pvnet_amd/texture.py, libpvnet_texture.so) on one GPU and writes profiles/texture_probe.txt.

    python tools/texture_probe.py [--out profiles/texture_probe.txt] [--rounds 7] [--reps 20] [--cpu-only]

The workload of tools/shade_probe.py: b = 32 images of 480 x 640, icospheres of 5 subdivisions (20 480 faces), m = 1, 3 and 13 instances
per image, flat shading over a background image; every mesh with spherical uv and a 512 x 512 texture.  Medians over ``--rounds`` rounds
in which the candidates alternate (``--reps`` back-to-back calls between two events), all in one process:
  (a) render_textured, nearest     (b) render_textured, bilinear     (c) render_textured on the same meshes without their textures
  (d) shade.render_color on the same inputs
so (a) - (c) and (b) - (c) are what the texel fetches cost beside the float64 divisions the resolve kernel makes anyway, and (c) - (d)
what the copied kernels cost beside the originals;
  (e) where the time of (a) and (b) goes by kernel, from one profiled stretch per m
and, once, the numpy restatement on one image at m = 3 (equality with the device's), and on the CPU the restatement's largest
difference to the float64 ray caster of tests/test_texture_cpu.py on that test's scenes (``--cpu-only``: these lines alone)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, H, W = 32, 480, 640
MS = (1, 3, 13)
TEX = 512


def oracle_lines():
    """the ray-caster comparison of tests/test_texture_cpu.py, on the CPU: the figures its docstring records"""
    from tests import render_cases as RC
    from tests import shade_restatement as SR
    from tests import test_shade_cpu as TS
    from tests import test_texture_cpu as TT
    from tests import texture_restatement as TR
    from pvnet_amd import shade
    lines = [f"  ray caster: smooth {TT.TEXTURE64.shape[0]} x {TT.TEXTURE64.shape[1]} texture, largest texel-to-texel step {TT.TEXEL_STEP:.0f} grey "
             f"levels, bilinear filter, {TS.ORACLE_H} x {TS.ORACLE_W}, interior pixels"]
    (sv, sf, _, snrm), sp = TS.ORACLE_SCENES["sphere"]
    bv, bf, buv = TT.atlas_box(0.3, 0.22, 0.26)
    scenes = {"sphere": ((sv, sf, snrm, RC.spherical_uv(sv)), sp), "box": ((bv, bf, shade.vertex_normals(bv, bf), buv), TS.ORACLE_SCENES["box"][1])}
    for name, ((v, f, nrm, uv), p) in sorted(scenes.items()):
        _, owner, _ = SR.instance_layers(v, f, p, TS.ORACLE_K, TS.ORACLE_H, TS.ORACLE_W)
        hits = TS.ray_hits(v, f, p, TS.ORACLE_K, TS.ORACLE_H, TS.ORACLE_W)
        interior = TS.interior_pixels(hits[0])
        ys, xs = np.nonzero(interior)
        corners = np.asarray(f, np.int64)[hits[1][ys, xs]]
        true_uv = (np.asarray(uv, np.float32).astype(np.float64)[corners] * hits[2][ys, xs][..., None]).sum(1)
        texel = TT.gl_bilinear(TT.TEXTURE64, true_uv[:, 0], true_uv[:, 1])
        white = np.full((len(v), 3), 255, np.uint8)
        for shading in ("none", "flat", "phong"):
            for ambient in TS.ORACLE_AMBIENTS:
                light = np.ones(len(ys))
                if shading != "none":
                    light = TS.glsl_shade(hits, v, f, white, nrm, p, TS.ORACLE_K, shading, (ambient,), vertex_light=False,
                                          normal_w=False)[ambient][ys, xs, 0] / 255.0
                args = (v, f, white, nrm, uv, TT.TEXTURE64, p, TS.ORACLE_K, owner[ys, xs], xs, ys, TR.SHADING[shading], ambient)
                got = TR.shade_pixels(*args, filter=TR.BILINEAR).astype(np.float64)
                _, got_uv = TR.shade_pixels(*args, filter=TR.BILINEAR, rounded=False)
                shift = np.abs(got_uv - true_uv) * (TT.TEXTURE64.shape[1], TT.TEXTURE64.shape[0])
                diff = np.abs(got - light[:, None] * texel)
                lines.append(f"  restatement against the textured ray caster, {name:6s} {shading:5s} ambient {ambient}: largest |du| tw "
                             f"{shift[:, 0].max():.3e}, |dv| th {shift[:, 1].max():.3e}; largest difference {diff.max():.3f} grey levels, mean "
                             f"{diff.mean():.3f}; {int(interior.sum())} of {int(hits[0].sum())} covered pixels compared")
        lines.append(f"  the test's bar, {name}: 0.5 + {TT.MEASURED_SHIFT[name]:.1e} x {TT.TEXEL_STEP:.0f} + 0.01 = {TT.oracle_bar(name):.5f} grey levels")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    lines = []
    if not args.cpu_only:
        lines += device_lines(args)
    lines += oracle_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


def device_lines(args):
    import torch
    from pvnet_amd import render, shade, texture
    from raster_probe import make_poses, timed
    from shade_probe import colours
    from tests import texture_restatement as TR
    from tests.render_cases import spherical_uv
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    v, f = render.icosphere(5, 0.09)   # at z = 0.6: a disc of radius 86 px
    scales = np.linspace(0.5, 0.8, 13)
    col, nrm, uv = colours(v), v / np.linalg.norm(v, axis=1, keepdims=True), spherical_uv(v)
    tex = rng.integers(0, 256, (TEX, TEX, 3), dtype=np.uint8)
    shapes = [v] + [v * s for s in scales]   # mesh 0 for m = 1, meshes 1 .. 13 for m = 3 and 13
    textured = texture.TexturedMeshes([(x, f, col, nrm, uv, tex) for x in shapes])
    bare = texture.TexturedMeshes([(x, f, col, nrm, None, None) for x in shapes])
    coloured = shade.ColorMeshes([(x, f, col, nrm) for x in shapes])
    Kd = torch.from_numpy(K).to(dev)
    rgb_out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    d_out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    l_out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    background = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    out = dict(background=background, out_rgb=rgb_out, out_depth=d_out, out_labels=l_out)
    cands, setup = {}, {}
    for m in MS:
        poses = torch.from_numpy(make_poses(rng, B * m, 0.12 if m == 1 else 0.2).reshape(B, m, 3, 4)).to(dev)
        ids, labels = ([0] if m == 1 else list(range(1, m + 1))), list(range(1, m + 1))
        ws = torch.empty(texture.texture_workspace_bytes(B * m, B, H, W, textured), dtype=torch.uint8, device=dev)
        setup[m] = (poses, ids, labels, ws)
        for tag, table, filt in (("(a) render_textured nearest ", textured, "nearest"), ("(b) render_textured bilinear", textured, "bilinear"),
                                 ("(c) render_textured, no textures", bare, "nearest")):
            cands[f"{tag} m = {m}"] = lambda p=poses, i=ids, lb=labels, w_=ws, t=table, fl=filt: texture.render_textured(
                t, i, lb, p, Kd, H, W, shading="flat", filter=fl, workspace=w_, **out)
        cands[f"(d) shade.render_color m = {m}"] = lambda p=poses, i=ids, lb=labels, w_=ws: shade.render_color(
            coloured, i, lb, p, Kd, H, W, shading="flat", workspace=w_, **out)
    for fn in cands.values():   # warm up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
    lines = [f"texture_probe: b = {B}, {H} x {W}, icospheres of {len(f)} faces, a {TEX} x {TEX} texture per mesh, medians of {args.rounds} "
             f"alternating rounds of {args.reps} calls, {torch.cuda.get_device_name(0)}"]
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in med.items():
        lines.append(f"  {k:46s} {t:9.1f} us   (min {min(times[k]):.1f}, max {max(times[k]):.1f})")
    for m in MS:
        a, b, c, d = (med[f"{tag} m = {m}"] for tag in ("(a) render_textured nearest ", "(b) render_textured bilinear",
                                                        "(c) render_textured, no textures", "(d) shade.render_color"))
        lines.append(f"  m = {m:2d}: the texel fetches, nearest (a) - (c) = {a - c:6.1f} us, bilinear (b) - (c) = {b - c:6.1f} us; the copied "
                     f"kernels beside the originals (c) - (d) = {c - d:6.1f} us; (a) / (d) = {a / d:.2f}, (b) / (d) = {b / d:.2f}")
    try:
        from torch.profiler import ProfilerActivity, profile
        for m in MS:
            for tag in ("(a) render_textured nearest ", "(b) render_textured bilinear"):
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for _ in range(5):
                        cands[f"{tag} m = {m}"]()
                    torch.cuda.synchronize()
                per = {e.key: e.device_time_total / max(e.count, 1) for e in prof.key_averages() if "texture_" in e.key}
                total = sum(per.values())
                for key, t in per.items():
                    lines.append(f"  (e) {tag[4:].strip():26s} m = {m:2d}: {key[:56]:56s} {t:9.1f} us per launch ({100.0 * t / total:4.1f} %)")
    except Exception as ex:   # the profiler is an aid, not the measurement
        lines.append(f"  (e) by kernel: profiler unavailable ({type(ex).__name__})")
    poses, ids, labels, _ = setup[3]
    p0 = poses[0].cpu().numpy()
    rmeshes = [textured.mesh(k) for k in range(textured.count)]
    layers = {}   # the instances' depth and face images: once for both filters
    for filt in ("nearest", "bilinear"):
        got = texture.render_textured(textured, ids, labels, poses[:1], Kd, H, W, filter=filt, background=background[:1], return_visible=True,
                                      return_status=True)
        want = TR.render(rmeshes, [(ids[j], p0[j], K, 0, labels[j]) for j in range(3)], 1, H, W, shading="flat", filter=filt,
                         background=background[:1].cpu().numpy(), layers=layers)
        equal = all(np.array_equal(a.cpu().numpy().reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))
                    for a, b in zip(got, want))
        lines.append(f"  numpy restatement, one image at m = 3, {filt}: equal to the device's, bit for bit: {equal}")
    return lines


if __name__ == "__main__":
    main()
