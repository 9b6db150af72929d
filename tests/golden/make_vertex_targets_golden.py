"""Regenerates tests/golden/vertex_targets.npz: small masks and key-points with what the REFERENCE's own ``compute_vertex_hcoords``
(lib/datasets/linemod_dataset.py:68-81) returns for them, with ``use_motion`` off and on.

    python tests/golden/make_vertex_targets_golden.py <root of a zju3dv/pvnet checkout>

CPU only.  The reference's module is imported unchanged, with its repository root as the working directory and the shims of
tools/run_reference.py (tools/refshim.py) for the third-party packages its imports name but this function never touches.

The file holds data only: per case ``mask [h,w]`` uint8, ``hcoords [vn,3]`` (float64, or float32 where the case is about that) and
the reference's ``ref [h,w,2vn]`` / ``ref_motion [h,w,2vn]`` float32 exactly as returned (the loader's ``permute(2, 0, 1)`` makes
them ``[2vn,h,w]``).  The cases cover: mask values 0 / 1 / 2; a key-point exactly on a foreground pixel (n = 0); one 5e-4 beside a
foreground pixel (0 < n < 1e-3); hz = 0, hz != 1, hz < 0; key-points outside the image; no foreground; h w not a multiple of 8;
float32 key-points.
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "vertex_targets.npz")


def blob(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r).astype(np.uint8)


def cases():
    rng = np.random.default_rng(20241017)
    out = {}
    m = blob(12, 16, 6, 8, 4.5)
    m[0:2, 0:5] = 2            # not a target pixel, but weight 2
    m[11, 15] = 1              # a target pixel in the last row and column
    assert m[6, 8] == 1 and m[5, 9] == 1
    out["values_012_near_keypoints"] = (m, np.array([[8.0, 6.0, 1.0],           # exactly on the foreground pixel (8, 6): n = 0
                                                     [9.0005, 5.0, 1.0],        # 5e-4 beside the foreground pixel (9, 5)
                                                     [8.0, 6.0007, 1.0],        # 7e-4 beside (8, 6), along y
                                                     [-40.25, 300.5, 1.0],      # far outside the image
                                                     [15.0, 11.0, 1.0]]))       # on the corner pixel
    m = blob(10, 16, 5, 7, 3.6)
    out["homogeneous_scales"] = (m, np.array([[3.5, -2.25, 0.0],                # hz = 0: a direction, the same for every pixel
                                              [17.5, 12.5, 2.5],                # hz != 1: the point (7, 5), a foreground pixel, scaled
                                              [-3.0, -2.0, -0.5],               # hz < 0
                                              [0.0, 0.0, 0.0],                  # the zero vector: n = 0 everywhere
                                              [1e-4, -2e-4, 0.0],               # 0 < n < 1e-3 everywhere
                                              [7.3, 4.9, 1.0]]))
    out["no_foreground"] = (np.zeros((8, 8), np.uint8), rng.uniform(-5.0, 12.0, (2, 3)))
    m = blob(7, 9, 3, 4, 2.7)   # 63 pixels
    hc = np.concatenate([rng.uniform(-20.0, 30.0, (9, 2)), rng.uniform(0.5, 2.0, (9, 1))], 1)
    out["odd_size_nine_keypoints"] = (m, hc)
    m = blob(9, 8, 4, 4, 3.0)
    m[m == 0] = (rng.random((9, 8)) < 0.2).astype(np.uint8)[m == 0] * 2
    out["float32_keypoints"] = (m, np.concatenate([rng.uniform(-3.0, 11.0, (4, 2)), np.ones((4, 1))], 1).astype(np.float32))
    return out


def main(reference_root):
    import refshim
    refshim.install(reference_root)
    refshim.pin_overlay(reference_root)
    cwd = os.getcwd()
    os.chdir(reference_root)   # lib/utils/config.py opens its files relatively
    try:
        ref = importlib.import_module("lib.datasets.linemod_dataset")
    finally:
        os.chdir(cwd)
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference_root) + os.sep), ref.__file__
    arrays, names = {}, []
    for name, (mask, hc) in cases().items():
        names.append(name)
        arrays[f"{name}.mask"] = mask
        arrays[f"{name}.hcoords"] = hc
        for key, motion in (("ref", False), ("ref_motion", True)):
            with np.errstate(all="ignore"):
                got = ref.compute_vertex_hcoords(mask.copy(), hc.copy(), use_motion=motion)
            assert got.dtype == np.float32 and got.shape == mask.shape + (2 * hc.shape[0],)
            arrays[f"{name}.{key}"] = got
        print(f"{name:28s} {mask.shape} vn={hc.shape[0]} target pixels {int((mask == 1).sum())}, other non-zero {int((mask > 1).sum())}")
    arrays["cases"] = np.array(names)
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
