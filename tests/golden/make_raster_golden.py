"""Regenerates tests/golden/raster.npz: what the REFERENCE's own ``mesh_binary_rasterization``
(lib/utils/extend_utils/src/mesh_rasterization.cpp:43-71) and ``Projector.project_K`` (lib/utils/base_utils.py:290-294) return for small
meshes, degenerate triangles, random triangle soups and triangles whose mask a contracted evaluation of the predicate changes.

    python tests/golden/make_raster_golden.py <root of a zju3dv/pvnet checkout>

CPU only.  The reference's C++ file is compiled as it stands (``g++ -O2 -shared``) into a temporary directory outside this repository
and called through ctypes with the argument list of extend_utils.py:15-18; its ``Projector`` is imported unchanged (tools/refshim.py
serves the third-party packages its module names).  The file written holds data only:

* ``mesh.<name>.vertices / .faces`` -- meshes made HERE (pvnet_amd.render.icosphere / box_mesh / l_prism_mesh);
* render cases ``r.<name>.mesh / .pose / .K / .size / .tri / .mask``: the reference's float32 triangles (project_K, then
  np.ascontiguousarray(..., np.float32) as extend_utils.py:13) and its mask;
* triangle cases ``t.<name>.tri / .size / .mask`` in three groups: ``degenerate``, ``soup`` and ``contract`` -- the last found by
  also evaluating tests/raster_restatement.py with ``contracted=True`` and keeping triangles whose masks differ.
"""
import ctypes
import importlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "raster.npz")

DEGENERATE = {   # name -> triangle: the consequences of the loop bounds and `>=` that belong to the definition
    "point": [(5.5, 7.5), (5.5, 7.5), (5.5, 7.5)],
    "collinear": [(2, 2), (6, 6), (10, 10)],
    "outside_corner": [(-3, -3), (-1, -1), (-0.5, -0.5)],
    "point_last_column_row": [(22.5, 18.5), (22.5, 18.5), (22.5, 18.5)],
    "denormal_products": [(0, 0), (1e-14, 0), (0, 1e-14)],
    "left_of_frame_collinear": [(-1.75, 3), (-1.75, 9), (-1.75, 5)],
    "right_of_frame_collinear": [(23.5, 3), (23.5, 9), (23.5, 5)],
    "covers_frame": [(-50, -10), (90, -10), (10, 80)],
    "sliver": [(-50, 10), (80, 10), (10, 11)],
}
SOUP_SIZE = (20, 24)


def build_reference(reference_root, tmp):
    src = os.path.join(reference_root, "lib", "utils", "extend_utils", "src", "mesh_rasterization.cpp")
    so = os.path.join(tmp, "ref_mesh_rasterization.so")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-O2", "-std=c++11", "-fPIC", "-shared", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.mesh_binary_rasterization.restype = None
    lib.mesh_binary_rasterization.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]

    def rasterize(triangles_2d, h, w):   # extend_utils.py:7-20
        tn = triangles_2d.shape[0]
        mask = np.ascontiguousarray(np.zeros([h, w], np.uint8))
        triangles_2d = np.ascontiguousarray(triangles_2d, np.float32)
        lib.mesh_binary_rasterization(triangles_2d.ctypes.data, mask.ctypes.data, tn, h, w)
        return mask

    return rasterize


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose_at(rng, t):
    R = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], 1)


def camera(h, w):
    return np.array([[0.95 * w, 0.0, w / 2.0 + 0.37], [0.0, 0.97 * w, h / 2.0 - 0.21], [0.0, 0.0, 1.0]])


def contract_candidates(rng, n):
    """triangles with an edge through a pixel centre and non-dyadic vertices: where one rounding more or less flips the sign"""
    out = []
    for _ in range(n):
        p = rng.integers(2, 18, 2).astype(np.float64)
        d = rng.normal(size=2)
        a, b = p - rng.uniform(0.5, 6) * d, p + rng.uniform(0.5, 6) * d
        c = p + rng.normal(size=2) * 5
        out.append(np.asarray([a, b, c], np.float32))
    return out


def main(reference_root):
    import refshim
    refshim.install(reference_root)
    refshim.pin_overlay(reference_root)
    cwd = os.getcwd()
    os.chdir(reference_root)   # lib/utils/config.py opens its files relatively
    try:
        base_utils = importlib.import_module("lib.utils.base_utils")
    finally:
        os.chdir(cwd)
    assert os.path.abspath(base_utils.__file__).startswith(os.path.abspath(reference_root) + os.sep), base_utils.__file__
    from pvnet_amd import render
    from tests import raster_restatement as RS
    tmp = tempfile.mkdtemp(prefix="raster_golden_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        ref_rasterize = build_reference(reference_root, tmp)
        rng = np.random.default_rng(20261018)
        arrays = {}
        meshes = {"ico1": render.icosphere(1, 0.1), "ico2": render.icosphere(2, 0.1), "ico3": render.icosphere(3, 0.1),
                  "box": render.box_mesh(0.15, 0.1, 0.2), "lprism": render.l_prism_mesh(0.2, 0.08)}
        for name, (v, f) in meshes.items():
            arrays[f"mesh.{name}.vertices"], arrays[f"mesh.{name}.faces"] = v, f
        rcases = []
        for h, w in ((60, 80), (33, 47)):
            K = camera(h, w)
            for name in ("ico1", "ico2", "ico3"):
                # inside the frame (twice), cut by the left border, cut by the bottom-right corner
                for k, t in enumerate(((0.0, 0.0, 0.55), (0.05, -0.03, 0.4), (-0.27, 0.02, 0.5), (0.21, 0.16, 0.45))):
                    rcases.append((f"{name}_{h}x{w}_{k}", name, pose_at(rng, t), K, (h, w)))
        for name in ("box", "lprism"):
            for k, t in enumerate(((0.0, 0.0, 0.5), (0.12, -0.1, 0.35))):
                rcases.append((f"{name}_60x80_{k}", name, pose_at(rng, t), camera(60, 80), (60, 80)))
        for cname, mname, pose, K, (h, w) in rcases:
            v, f = meshes[mname]
            pts = base_utils.Projector.project_K(v, pose, K)                       # the reference's projection (float64)
            tri = np.ascontiguousarray(pts[f.reshape(-1)].reshape(-1, 3, 2), np.float32)   # extend_utils.py:13
            mask = ref_rasterize(tri, h, w)
            arrays[f"r.{cname}.mesh"], arrays[f"r.{cname}.pose"], arrays[f"r.{cname}.K"] = np.array(mname), pose, K
            arrays[f"r.{cname}.size"], arrays[f"r.{cname}.tri"], arrays[f"r.{cname}.mask"] = np.array([h, w]), tri, mask
            print(f"render {cname:20s} {len(f):5d} faces -> {int(mask.sum()):5d} pixels")
        arrays["render_cases"] = np.array([c[0] for c in rcases])

        tcases = []   # (name, group, tri [tn,3,2], (h, w))
        for name, t in DEGENERATE.items():
            tcases.append((name, "degenerate", np.asarray([t], np.float32), SOUP_SIZE))
        tcases.append(("degenerate_all", "degenerate", np.asarray(list(DEGENERATE.values()), np.float32), SOUP_SIZE))
        for k in range(40):   # integer vertices (the sign of zero, edges through pixel centres), half of them with quarter-pixel offsets
            t = rng.integers(-4, 31, (50, 3, 2)).astype(np.float32)
            if k >= 20:
                t += rng.integers(0, 4, (50, 3, 2)).astype(np.float32) * np.float32(0.25)
            tcases.append((f"soup{k:02d}", "soup", t, SOUP_SIZE))
        found = 0
        for t in contract_candidates(rng, 4000):
            plain, _ = RS.rasterize(t[None], *SOUP_SIZE)
            fused, _ = RS.rasterize(t[None], *SOUP_SIZE, contracted=True)
            if not np.array_equal(plain, fused):
                tcases.append((f"contract{found:02d}", "contract", t[None], SOUP_SIZE))
                found += 1
                if found == 24:
                    break
        assert found >= 20, found
        for name, group, tri, (h, w) in tcases:
            mask = ref_rasterize(tri, h, w)
            arrays[f"t.{name}.tri"], arrays[f"t.{name}.size"], arrays[f"t.{name}.mask"] = tri, np.array([h, w]), mask
            arrays[f"t.{name}.group"] = np.array(group)
            mine, _ = RS.rasterize(tri, h, w)
            print(f"triangles {name:26s} {group:10s} {len(tri):3d} -> {int(mask.sum()):4d} pixels"
                  f"{'' if np.array_equal(mine, mask) else '   RESTATEMENT DIFFERS'}")
        arrays["triangle_cases"] = np.array([c[0] for c in tcases])
        np.savez_compressed(OUT, **arrays)
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
