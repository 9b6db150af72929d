"""Regenerates tests/golden/augment.npz: small samples with what the REFERENCE's own ``LineModDatasetRealAug.augmentation``
(lib/datasets/linemod_dataset.py:254-290, lib/datasets/augmentation.py) returns for them.

    python tests/golden/make_augment_golden.py <root of a zju3dv/pvnet checkout>

CPU only.  The reference's modules are imported unchanged (tools/refshim.py serves the third-party packages they name).  Two things are
put under them, and nothing of them is changed:

* ``cv2`` is a stand-in of ours: ``getRotationMatrix2D`` by its formula, ``warpAffine`` / ``resize`` by the samplers of
  tests/augment_restatement.py (INTER_NEAREST and INTER_LINEAR).  cv2 itself is not installed here, so its fixed-point bilinear weights
  are not what the images below were made with; the key-points and the masks' geometry do not depend on them.
* ``np.random.random`` / ``uniform`` / ``randint`` consume one row of twelve uniforms per sample under the mapping of
  include/pvnet_augment.h (u0 mask-out gate, u1 u2 its sides, u3 u4 its place, u5 the angle, u6 the resize gate, u7 the ratio, u8 hbeg,
  u9 wbeg, u10 the flip gate); which draw a call is, is read from the reference's source line that makes it.  The rectangle's fill is the
  counter-based one.

The file holds data only: per case the inputs (``rgb [48,64,3]`` uint8, ``mask [48,64]`` uint8, ``hcoords [vn,3]`` float64,
``uniforms [12]``, the target size, the seed, the configuration overrides as JSON), the reference's float64 ``hcoords`` (before the
loader casts them to float32), and its uint8 image and its mask.  Without rotation and without resize -- flip, crop, pad and mask-out
are pure numpy in the reference -- these are the reference's own numbers.  With them they are what the reference's own code chains
together (``rotate_instance``, ``crop_resize_instance_v2``, crop or pad, flip: its order, offsets and conventions) over the two stand-in
samplers: interpolated twice and rounded to uint8 twice, where the product interpolates once.  The mask is a chain of integer maps
and must be the product's exactly; the image is an oracle to within the two roundings wherever no tap of the second interpolation
reaches a canvas pixel already blended with the zero border.  ``ramp_cases`` lists the cases whose picture is the ramp
``(4x, 5y, 2x + 2y)``, which has a closed form; their ``rgb`` is not stored: it is ``tests/augment_cases.ramp(48, 64)``.
"""
import importlib
import io
import json
import linecache
import math
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "augment.npz")
H, W = 48, 64


def blob(cy, cx, r, h=H, w=W):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r).astype(np.uint8)


def picture(rng, h=H, w=W):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 3 + yy, 255 - yy * 4, (xx * yy) % 256], -1)
    return np.clip(base + rng.integers(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)


def cases():
    """name -> (mask, vn, target (height, width), configuration overrides, uniforms)"""
    rng = np.random.default_rng(20241018)
    U = dict(maskout=0, xs=1, ys=2, xl=3, yl=4, ang=5, resize=6, ratio=7, hbeg=8, wbeg=9, flip=10, mul=11)

    def row(**kw):
        u = rng.uniform(0.05, 0.95, 12)
        for k, v in kw.items():
            u[U[k]] = v
        return u

    grow = dict(resize_hmin=24, resize_hmax=44, resize_wmin=24, resize_wmax=44)     # ratios above 1 for a blob of radius 10
    shrink = dict(resize_hmin=5, resize_hmax=8, resize_wmin=5, resize_wmax=8)       # ratios below 0.45: smaller than the target
    still = dict(rotation=False)
    out = {
        "all_open": (blob(24, 30, 10.3), 9, (32, 40), grow, row(maskout=0.2, resize=0.3, flip=0.1, xs=0.9, ys=0.9)),
        "all_closed": (blob(20, 36, 10.3), 9, (32, 40), grow, row(maskout=0.7, resize=0.9, flip=0.8)),
        "odd_target": (blob(26, 28, 9.2), 4, (31, 37), grow, row(maskout=0.1, resize=0.5, flip=0.3, ang=0.93)),
        "resized_smaller_than_target": (blob(24, 32, 10.3), 3, (32, 40), shrink, row(maskout=0.9, resize=0.1, flip=0.9)),
        "flip_crop_only": (blob(22, 30, 8.5), 5, (32, 40), still, row(maskout=0.6, resize=0.85, flip=0.2)),
        "maskout_crop": (blob(24, 34, 11.1), 5, (32, 40), still, row(maskout=0.3, resize=0.95, flip=0.7, xs=0.95, ys=0.8)),
        "pad_both": (blob(24, 32, 9.0), 2, (56, 72), still, row(maskout=0.8, resize=0.99, flip=0.4)),
        "pad_rows_crop_columns": (blob(30, 20, 7.0), 2, (56, 40), still, row(maskout=0.25, resize=0.81, flip=0.6, xs=0.99, ys=0.99)),
        "negative_start": (blob(24, 6, 9.5), 3, (32, 40), still, row(maskout=0.4, resize=0.9, flip=0.9, xl=0.01, xs=0.9, ys=0.9)),
        "empty_mask": (np.zeros((H, W), np.uint8), 3, (32, 40), {}, row(maskout=0.9, resize=0.2, flip=0.3)),
        "same_size": (blob(24, 32, 10.3), 9, (48, 64), {}, row(maskout=0.45, resize=0.5, flip=0.45, xs=0.5)),
    }
    for name, (mask, vn, size, over, u) in out.items():
        hc = np.concatenate([rng.uniform(-10.0, 70.0, (vn, 2)), np.ones((vn, 1))], 1)
        hc[0] = (31.5, 24.25, 1.0)
        if vn > 2:
            hc[2] *= 1.75   # a key-point whose homogeneous scale is not 1
        out[name] = (picture(rng), mask, hc, size, over, u)
    # appended after every draw above, so the earlier cases stay what they were: ramp pictures, rotated, the mask-out gate closed
    from tests.augment_cases import ramp as ramp_picture
    ramp = ramp_picture(H, W)
    mixed = dict(resize_hmin=12, resize_hmax=30, resize_wmin=12, resize_wmax=30)
    more = {
        "ramp_rotation_only": (blob(22, 34, 9.4), (32, 40), grow, dict(maskout=0.7, resize=0.9, flip=0.8, ang=0.08)),
        "ramp_rotation_grow": (blob(25, 29, 9.1), (24, 32), grow, dict(maskout=0.6, resize=0.2, flip=0.7, ang=0.9)),
        "ramp_rotation_shrink": (blob(23, 33, 10.2), (32, 40), shrink, dict(maskout=0.8, resize=0.4, flip=0.9, ang=0.2)),
        "ramp_rotation_resize_flip": (blob(21, 30, 8.7), (24, 32), mixed, dict(maskout=0.9, resize=0.5, flip=0.3, ang=0.75)),
        "ramp_rotation_resize_odd_target": (blob(26, 35, 9.8), (31, 37), mixed, dict(maskout=0.55, resize=0.1, flip=0.6, ang=0.97)),
    }
    for name, (mask, size, over, kw) in more.items():
        u = row(**kw)
        hc = np.concatenate([rng.uniform(-10.0, 70.0, (4, 2)), np.ones((4, 1))], 1)
        out[name] = (ramp.copy(), mask, hc, size, over, u)
    return out


class Draws:
    """the three np.random functions the reference's augmentation calls, on one row of uniforms"""

    def __init__(self, u, seed, image_index):
        self.u, self.seed, self.image_index = [float(x) for x in u], seed, image_index
        self.used = set()

    def _which(self, table, depth=2):
        f = sys._getframe(depth)
        line = linecache.getline(f.f_code.co_filename, f.f_lineno)
        for fn, key, k in table:
            if f.f_code.co_name == fn and key in line:
                assert k not in self.used, (fn, line)
                self.used.add(k)
                return self.u[k]
        raise AssertionError(f"unmapped draw in {f.f_code.co_name}: {line!r}")

    def random(self):
        return self._which((("augmentation", "cfg['mask']", 0), ("crop_resize_instance_v2", "random()<0.8", 6),
                            ("augmentation", "cfg['flip']", 10)))

    def uniform(self, lo, hi):
        from tests import augment_restatement as RS
        u = self._which((("mask_out_instance", "x_side=", 1), ("mask_out_instance", "y_side=", 2), ("rotate_instance", "degree=", 5),
                         ("crop_resize_instance_v2", "resize_ratio=", 7)))
        return RS.uniform(lo, hi, u)

    def randint(self, lo, hi, size=None):
        from tests import augment_restatement as RS
        if size is not None:   # the rectangle's fill (mask_out_instance, augmentation.py:199-200)
            f = sys._getframe(1)
            assert f.f_code.co_name == "mask_out_instance" and (lo, hi) == (0, 255)
            L = f.f_locals
            if 0 in size:
                return np.zeros(size, np.int64)
            h, w = L["img"].shape[:2]   # the pixels of the reference's own slices
            rows = np.arange(h)[L["y_loc"] - L["y_side"]:L["y_loc"] + L["y_side"]]
            cols = np.arange(w)[L["x_loc"] - L["x_side"]:L["x_loc"] + L["x_side"]]
            assert (len(rows), len(cols), 3) == tuple(size)
            ys, xs = np.meshgrid(rows, cols, indexing="ij")
            return RS.fill_values(self.seed, self.image_index, w, ys, xs)
        u = self._which((("mask_out_instance", "x_loc=", 3), ("mask_out_instance", "y_loc=", 4),
                         ("crop_or_padding_to_fixed_size_instance", "hbeg=0 if hpad", 8),
                         ("crop_or_padding_to_fixed_size_instance", "wbeg=0 if wpad", 9),
                         ("crop_or_padding_to_fixed_size", "hbeg=0 if hpad", 8), ("crop_or_padding_to_fixed_size", "wbeg=0 if wpad", 9)))
        status = [0]
        v = RS.randint(int(lo), int(hi), u, status)
        assert status[0] == 0, "the reference raises where hi <= lo: not a golden case"
        return v


def install_cv2():
    import cv2
    from tests import augment_restatement as RS
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = 0, 1, 0

    def getRotationMatrix2D(center, angle, scale):
        assert scale == 1
        ang = float(angle) * math.pi / 180.0   # (the host side of the product computes the pair the same way: augment.pack_uniforms)
        return RS.rotation_matrix(float(center[0]), float(center[1]), math.cos(ang), math.sin(ang))

    def warpAffine(src, M, dsize, flags=1, borderMode=0, borderValue=0):
        assert borderMode == 0 and borderValue == 0
        return RS.warp_nearest(src, M, dsize) if flags == 0 else RS.warp_linear(src, M, dsize)

    def resize(src, dsize, interpolation=1):
        return RS.resize_nearest(src, dsize) if interpolation == 0 else RS.resize_linear(src, dsize)

    cv2.getRotationMatrix2D, cv2.warpAffine, cv2.resize = getRotationMatrix2D, warpAffine, resize


def main(reference_root):
    import refshim
    refshim.install(reference_root)
    refshim.pin_overlay(reference_root)
    install_cv2()
    cwd = os.getcwd()
    os.chdir(reference_root)   # lib/utils/config.py opens its files relatively
    try:
        ref = importlib.import_module("lib.datasets.linemod_dataset")
    finally:
        os.chdir(cwd)
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference_root) + os.sep), ref.__file__
    from tests import augment_restatement as RS
    base = dict(ref.default_aug_cfg)
    arrays, names = {}, []
    saved = np.random.random, np.random.uniform, np.random.randint
    for k, (name, (rgb, mask, hc, (height, width), over, u)) in enumerate(cases().items()):
        cfg = {**base, **over}
        seed = 1000 + k
        draws = Draws(u, seed, 0)
        np.random.random, np.random.uniform, np.random.randint = draws.random, draws.uniform, draws.randint
        try:
            with np.errstate(all="raise"):
                img, m, out = ref.LineModDatasetRealAug.augmentation(types.SimpleNamespace(cfg=cfg), rgb.copy(), mask.astype(np.int32),
                                                                     hc.copy(), height, width)
        finally:
            np.random.random, np.random.uniform, np.random.randint = saved
        assert out.dtype == np.float64 and img.shape == (height, width, 3) and m.shape == (height, width)
        names.append(name)
        arrays[f"{name}.mask"], arrays[f"{name}.hcoords"] = mask, hc
        if not name.startswith("ramp_"):   # the ramp is a formula (tests/augment_cases.ramp); interleaved it does not deflate
            arrays[f"{name}.rgb"] = rgb
        arrays[f"{name}.uniforms"], arrays[f"{name}.size"], arrays[f"{name}.seed"] = u, np.array([height, width]), np.array(seed)
        arrays[f"{name}.cfg"] = np.array(json.dumps(over))
        arrays[f"{name}.ref_hcoords"] = out
        integer_only = not (5 in draws.used or 7 in draws.used)
        assert img.dtype == np.uint8 and int(m.min()) >= 0 and int(m.max()) <= 255
        arrays[f"{name}.ref_image"] = np.ascontiguousarray(img)
        arrays[f"{name}.ref_mask"] = np.ascontiguousarray(m).astype(np.uint8)
        print(f"{name:34s} vn={hc.shape[0]} -> {(height, width)} draws {sorted(draws.used)} foreground {int((m != 0).sum())}"
              f"{' (pure numpy in the reference)' if integer_only else ' (the chain over the stand-in samplers)'}")
    arrays["cases"] = np.array(names)
    arrays["ramp_cases"] = np.array([n for n in names if n.startswith("ramp_")])
    # np.savez_compressed's container without the zip64 fields it adds to every entry: most of the entries are a few bytes
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, value in arrays.items():
            data = io.BytesIO()
            np.lib.format.write_array(data, np.asanyarray(value), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0)), data.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
