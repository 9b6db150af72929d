"""Seeded inputs and a closed-form oracle for the training warp (include/pvnet_augment.h), shared by tests/test_augment_cpu.py,
tests/test_augment_device.py and tests/test_color_device.py.  A plain module: no fixtures, no device, no reference tree.

THE RAMP ORACLE.  Bilinear interpolation reproduces an affine function of position exactly, so for a source image
``I_c(x, y) = p_c x + q_c y`` (uint8, nothing clipped) the header's one-pass pixel is ``rint(I_c(sx, sy))`` wherever the four taps lie
inside the source and the resize's clamp is idle: one rounding and nothing else, hence ``|v - I_c(sx, sy)| <= 0.5``.  The source point
is NOT taken from the backward formulas of the header: ``source_points`` composes the FORWARD maps of pixel centres as 3 x 3 matrices

    R  the rotation (getRotationMatrix2D at scale 1, the plan's matrix),
    S  the resize:  X = (x + 0.5) w2 / w - 0.5, rows likewise,
    C  the crop or pad:  a translation by (woff - wbeg, hoff - hbeg),
    F  the flip:  X -> width - 1 - X,

and inverts the product with ``np.linalg.inv`` in float64.  The plan's scalars come from the restatement; they are held to the
reference through the key-points.  ``RAMP_BAR`` = 0.5 (the one rint) + 1e-6 (float64 map error times the slope is about 1e-12).

THE SETS.  ``ramp_set()`` is the seeded set that holds the image to this closed form (mask-out gate closed, three
resize ranges x four targets, status 0 only: a draw whose restatement status is not 0 is drawn again, which the restatement decides
and no device does); ``ramp_maskout_case()`` has the gate open, ``ramp_odd_source()`` a 37 x 53 source.  ``sweep_calls()`` is the
seeded sweep for device == restatement: all twelve uniforms over [0, 1), blobs of every kind.  Everything is computed once per
process and must not be written to.
"""
import functools

import numpy as np

from tests import augment_restatement as RS

RAMP_BAR = 0.5 + 1e-6
SLOPES = {(48, 64): ((4, 0), (0, 5), (2, 2)), (37, 53): ((4, 0), (0, 6), (2, 3))}   # (p_c, q_c) per channel: at most 252 / 235 / 220, 208 / 216 / 212
GROW = dict(resize_hmin=24, resize_hmax=44, resize_wmin=24, resize_wmax=44)
SHRINK = dict(resize_hmin=5, resize_hmax=8, resize_wmin=5, resize_wmax=8)
MIXED = dict(resize_hmin=12, resize_hmax=30, resize_wmin=12, resize_wmax=30)
RANGES = dict(grow=GROW, shrink=SHRINK, mixed=MIXED)
TARGETS = ((32, 40), (31, 37), (56, 72), (48, 64))
RAMP_PER_GROUP = 25            # 12 groups: 300 samples
# interior pixels of ramp_set(), asserted from the restatement's plans (tests/test_augment_cpu.py): at least 140 in every sample (the
# fewest measured there is 146, a sample shrunk to a third and padded), 503 372 in all against the 200 000 asked for
RAMP_MIN_INTERIOR_PER_SAMPLE = 140
RAMP_MIN_INTERIOR_TOTAL = 200000
DEFECTS = ("resize_without_half_pixel", "flip_about_width", "rotation_sign", "hoff_hbeg_swapped")


def ramp(h, w):
    """[h,w,3] uint8 with channel c = p_c x + q_c y"""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([p * xx + q * yy for p, q in SLOPES[(h, w)]], -1)
    assert img.max() <= 255 and max(p for p, _ in SLOPES[(h, w)]) >= 3 and max(q for _, q in SLOPES[(h, w)]) >= 3   # grey levels per px
    return img.astype(np.uint8)


def blob(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r).astype(np.uint8)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def forward_matrices(plan, h, w, width, defect=None):
    """(R, F C S) as 3 x 3 float64: source pixel centre -> canvas, canvas -> output.  ``defect`` plants one of DEFECTS."""
    R = np.vstack([np.asarray(plan["R"], np.float64), [0.0, 0.0, 1.0]])
    if defect == "rotation_sign":
        R[0, 1], R[1, 0] = -R[0, 1], -R[1, 0]
    kx, ky = plan["w2"] / w, plan["h2"] / h
    S = np.array([[kx, 0.0, 0.5 * kx - 0.5], [0.0, ky, 0.5 * ky - 0.5], [0.0, 0.0, 1.0]])
    if defect == "resize_without_half_pixel":
        S[0, 2] = S[1, 2] = 0.0
    dy = plan["hoff"] - plan["hbeg"]
    C = np.array([[1.0, 0.0, plan["woff"] - plan["wbeg"]], [0.0, 1.0, -dy if defect == "hoff_hbeg_swapped" else dy], [0.0, 0.0, 1.0]])
    F = np.eye(3)
    if plan["flip"]:
        F[0, 0], F[0, 2] = -1.0, (width if defect == "flip_about_width" else width - 1)
    return R, F @ C @ S


def source_points(plan, h, w, height, width, defect=None):
    """per output pixel [height,width]: the source point (sx, sy) and the canvas point (cx, cy)"""
    R, FCS = forward_matrices(plan, h, w, width, defect)
    Y, X = np.mgrid[0:height, 0:width]
    P = np.stack([X, Y, np.ones_like(X)]).reshape(3, -1).astype(np.float64)
    s = np.linalg.inv(FCS @ R) @ P
    c = np.linalg.inv(FCS) @ P
    assert np.allclose(s[2], 1.0, atol=1e-12) and np.allclose(c[2], 1.0, atol=1e-12)
    shape = (height, width)
    return s[0].reshape(shape), s[1].reshape(shape), c[0].reshape(shape), c[1].reshape(shape)


def interior(sx, sy, cx, cy, h, w, margin=0.0):
    """the four taps inside the source (``margin`` px inside its border) and the canvas point inside the canvas (the clamp idle)"""
    return ((sx >= margin) & (sx <= w - 1 - margin) & (sy >= margin) & (sy <= h - 1 - margin)
            & (cx >= 0) & (cx <= w - 1) & (cy >= 0) & (cy <= h - 1))


def maskout_rectangle(mask, cfg, u):
    """step 1 of the header for a sample whose gate is open: the (rows, cols) the fill covers, under numpy's slice rule"""
    cfg = {**RS.DEFAULTS, **cfg}
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    xmin, xmax, ymin, ymax = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    x_side = int(np.floor(float(xmax - xmin) * RS.uniform(cfg["min_mask"], cfg["max_mask"], float(u[1])) / 2.0))
    y_side = int(np.floor(float(ymax - ymin) * RS.uniform(cfg["min_mask"], cfg["max_mask"], float(u[2])) / 2.0))
    status = [0]
    x_loc, y_loc = RS.randint(xmin, xmax, float(u[3]), status), RS.randint(ymin, ymax, float(u[4]), status)
    return np.arange(h)[y_loc - y_side:y_loc + y_side], np.arange(w)[x_loc - x_side:x_loc + x_side]


def recover_uint8(image):
    """[...,3,H,W] float32 normalised image -> the integers it was made from; they must round-trip exactly"""
    image = np.asarray(image)
    assert image.dtype == np.float32
    mean, std = RS.MEAN.reshape(3, 1, 1), RS.STD.reshape(3, 1, 1)
    v = np.rint((image * std + mean) * np.float32(255.0))
    assert v.min() >= 0 and v.max() <= 255
    assert np.array_equal((v.astype(np.float32) / np.float32(255.0) - mean) / std, image), "not a normalised uint8 image"
    return v.astype(np.int64)


def ramp_errors(v, plan, h, w, defect=None, rectangle=None):
    """v [3,height,width] integers of one sample -> (|v - I(sx, sy)| on the interior pixels [n,3], interior [height,width] bool,
    number of pixels left out for a tap inside ``rectangle``)"""
    height, width = v.shape[1:]
    sx, sy, cx, cy = source_points(plan, h, w, height, width, defect)
    inside = interior(sx, sy, cx, cy, h, w)
    left_out = 0
    if rectangle is not None:
        rows, cols = rectangle
        rect = np.zeros((h + 1, w + 1), bool)
        if len(rows) and len(cols):
            rect[np.ix_(rows, cols)] = True
        x0, y0 = np.clip(np.floor(sx).astype(np.int64), 0, w - 1), np.clip(np.floor(sy).astype(np.int64), 0, h - 1)
        tapped = rect[y0, x0] | rect[y0, x0 + 1] | rect[y0 + 1, x0] | rect[y0 + 1, x0 + 1]
        left_out = int((inside & tapped).sum())
        inside &= ~tapped
    exact = np.stack([p * sx + q * sy for p, q in SLOPES[(h, w)]])
    return np.abs(v - exact)[:, inside].T, inside, left_out


def ramp_check(images, group, defect=None):
    """images [n,3,height,width] float32 of one group -> (worst |v - I|, interior pixels per sample, pixels left out per sample)"""
    v = recover_uint8(images)
    h, w = group["rgb"].shape[1:3]
    worst, counts, left = 0.0, [], []
    for i, plan in enumerate(group["want"][4]):
        assert not plan["maskmul"]
        rect = maskout_rectangle(group["mask"][i], group["cfg"], group["U"][i]) if group.get("maskout") else None
        err, inside, out = ramp_errors(v[i], plan, h, w, defect, rect)
        worst = max(worst, float(err.max()) if err.size else 0.0)
        counts.append(int(inside.sum()))
        left.append(out)
    return worst, counts, left


# ---- the ramp sets ----------------------------------------------------------------------------------------------------------------
def _group(name, rng, n, h, w, size, cfg, seed, gate, accept_status0=True):
    """n samples of a ramp source h x w: blobs well inside, all uniforms over [0, 1) but the mask-out gate u0 (``gate``: open/closed)"""
    pic = ramp(h, w)
    masks, hcs, Us, outs = [], [], [], []
    while len(masks) < n:
        m = blob(h, w, rng.uniform(0.3 * h, 0.7 * h), rng.uniform(0.3 * w, 0.7 * w), rng.uniform(6.0, 11.0))
        hc = np.concatenate([rng.uniform(-5.0, w + 5.0, (3, 2)), np.ones((3, 1))], 1)
        u = rng.uniform(0.0, 1.0, 12)
        u[0] = 0.5 * u[0] + (0.0 if gate else 0.5)
        out = RS.augment_one(pic, m, hc, size[0], size[1], cfg, u, seed, len(masks))
        if accept_status0 and out[3] != 0:
            continue
        masks.append(m), hcs.append(hc), Us.append(u), outs.append(out)
    want = (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]),
            np.array([o[3] for o in outs], np.int32), [o[4] for o in outs])
    for a in want[:4]:
        a.setflags(write=False)
    return dict(name=name, rgb=np.ascontiguousarray(np.broadcast_to(pic, (n,) + pic.shape)), mask=np.stack(masks), hc=np.stack(hcs),
                size=size, cfg=dict(cfg), U=np.stack(Us), seed=seed, want=want, maskout=gate)


@functools.lru_cache(maxsize=None)
def ramp_set():
    """12 groups (three resize ranges x four targets) of RAMP_PER_GROUP samples from a 48 x 64 ramp, the mask-out gate closed"""
    rng = np.random.default_rng(20250117)
    return tuple(_group(f"{rname}->{size}", rng, RAMP_PER_GROUP, 48, 64, size, cfg, 300 + 10 * k + j, False)
                 for k, (rname, cfg) in enumerate(RANGES.items()) for j, size in enumerate(TARGETS))


@functools.lru_cache(maxsize=None)
def ramp_maskout_case():
    """the gate open: pixels with a tap inside the rectangle carry the random fill and are left out of the check"""
    return _group("maskout", np.random.default_rng(20250118), 12, 48, 64, (32, 40), dict(MIXED, min_mask=0.3, max_mask=0.8), 77, True)


@functools.lru_cache(maxsize=None)
def ramp_odd_source():
    """a 37 x 53 source (w no multiple of 8) to both store paths"""
    rng = np.random.default_rng(20250119)
    return tuple(_group(f"37x53->{size}", rng, 12, 37, 53, size, MIXED, 90 + j, False) for j, size in enumerate(((32, 40), (31, 37))))


def feature_counts(groups):
    """how many samples of the groups are rotated, resized up / down, padded, cropped with an offset, flipped"""
    n = dict(rotated=0, grow=0, shrink=0, row_pad=0, column_pad=0, hbeg=0, wbeg=0, flip=0)
    for g in groups:
        for p in g["want"][4]:
            n["rotated"] += p["rotated"] and p["R"][0, 1] != 0.0
            n["grow"] += p["resized"] and p["ratio"] > 1.0
            n["shrink"] += p["resized"] and p["ratio"] < 1.0
            n["row_pad"] += p["hoff"] > 0
            n["column_pad"] += p["woff"] > 0
            n["hbeg"] += p["hbeg"] > 0
            n["wbeg"] += p["wbeg"] > 0
            n["flip"] += p["flip"]
    return n


# ---- the sweep: device == restatement ---------------------------------------------------------------------------------------------
SWEEP_PER_CALL = 40
# (source, target, resize range, configuration on top, output type, mask_out type, mask input type, padded strides)
SWEEP_CALLS = (
    ((48, 64), (32, 40), "grow", dict(), "float32", "uint8", "uint8", False),
    ((48, 64), (31, 37), "mixed", dict(use_mask_out=True), "bfloat16", "uint8", "int32", True),
    ((37, 53), (56, 72), "shrink", dict(use_mask_out=True), "float16", "int64", "int64", False),
    ((37, 53), (48, 64), "grow", dict(use_mask_out=True, min_mask=1.2, max_mask=2.0), "float32", "uint8", "uint8", False),
    ((48, 64), (56, 40), "mixed", dict(), "float32", "int64", "int32", False),
    ((48, 64), (48, 64), "shrink", dict(use_mask_out=True, min_mask=1.2, max_mask=2.0), "bfloat16", "uint8", "int64", False),
    ((37, 53), (32, 40), "mixed", dict(use_mask_out=True), "float16", "uint8", "uint8", False),
)


def sweep_mask(rng, i, h, w):
    """the i-th mask of a call: empty, one row, one column, touching a border, or a blob anywhere; values 1 .. 3"""
    kind = i % 10
    m = np.zeros((h, w), np.uint8)
    if kind == 0:
        return m
    if kind == 1:
        x0 = int(rng.integers(0, w - 6))
        m[int(rng.integers(0, h)), x0:x0 + int(rng.integers(2, 7))] = 1
        return m
    if kind == 2:
        y0 = int(rng.integers(0, h - 6))
        m[y0:y0 + int(rng.integers(2, 7)), int(rng.integers(0, w))] = 1
        return m
    r = rng.uniform(2.0, 12.0)
    if kind == 3:   # over a border
        cy, cx = ((rng.choice([0.0, h - 1.0]), rng.uniform(0, w)) if rng.uniform() < 0.5 else (rng.uniform(0, h), rng.choice([0.0, w - 1.0])))
    else:
        cy, cx = rng.uniform(0.15 * h, 0.85 * h), rng.uniform(0.15 * w, 0.85 * w)
    return blob(h, w, cy, cx, r) * np.uint8(1 + i % 3)


@functools.lru_cache(maxsize=None)
def sweep_calls():
    """one dict per device call: inputs, how to call, and the restatement's output (``want``)"""
    rng = np.random.default_rng(20250120)
    calls = []
    for k, ((h, w), size, rname, over, out_dtype, mask_dtype, mask_in, pad) in enumerate(SWEEP_CALLS):
        n = SWEEP_PER_CALL
        rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        mask = np.stack([sweep_mask(rng, i, h, w) for i in range(n)])
        hc = np.concatenate([rng.uniform(-10.0, w + 10.0, (n, 3, 2)), rng.uniform(0.5, 2.0, (n, 3, 1))], 2)
        U = rng.uniform(0.0, 1.0, (n, 12))
        cfg = dict(RANGES[rname], **over)
        want = RS.augment_batch(rgb, mask, hc, size[0], size[1], cfg, U, 500 + k)
        calls.append(dict(rgb=rgb, mask=mask, hc=hc, size=size, cfg=cfg, U=U, seed=500 + k, out_dtype=out_dtype, mask_dtype=mask_dtype,
                          mask_in=mask_in, pad_strides=pad, want=want))
    return tuple(calls)


def sweep_coverage(calls):
    """what the sweep walks, from the restatement's plans and status"""
    status = np.concatenate([c["want"][3] for c in calls])
    plans = [p for c in calls for p in c["want"][4]]
    cover = {f"status_{b}": int((status & b != 0).sum()) for b in (RS.S_RANGE, RS.S_EMPTIED, RS.S_DEGENERATE, RS.S_NO_FOREGROUND)}
    for key in ("rotated", "resized", "flip", "maskmul"):
        cover[key] = sum(bool(p[key]) for p in plans)
        cover["not_" + key] = sum(not p[key] for p in plans)
    cover.update(row_pad=sum(p["hoff"] > 0 for p in plans), column_pad=sum(p["woff"] > 0 for p in plans),
                 row_crop=sum(p["hbeg"] > 0 for p in plans), column_crop=sum(p["wbeg"] > 0 for p in plans), samples=len(plans))
    return cover


# ---- tests/golden/augment.npz -----------------------------------------------------------------------------------------------------
def golden_rgb(g, n):
    """the picture of a recorded case: stored, or for the names under ``ramp_cases`` the 48 x 64 ramp"""
    return g[n + ".rgb"] if n + ".rgb" in g else ramp(48, 64)


def two_pass_difference(v, ref_image, plan, h, w):
    """v [3,height,width] one-pass integers, ref_image [height,width,3] the reference's chain -> (largest |v - ref| where the source
    point is at least 2 px inside the source and the canvas point inside the canvas, how many such pixels, largest |v - ref| anywhere)"""
    height, width = v.shape[1:]
    d = np.abs(v - ref_image.astype(np.int64).transpose(2, 0, 1))
    inside = interior(*source_points(plan, h, w, height, width), h, w, margin=2.0)
    return (int(d[:, inside].max()) if inside.any() else 0), int(inside.sum()), int(d.max())
