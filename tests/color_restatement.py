"""numpy restatement of THE DEFINITION of include/pvnet_color.h, written from the header alone: float32, float64 where the header
says so, and integers, one operation per step in the header's order.  The kernels of pvnet_amd/csrc/color_jitter.hip are held to it
bit for bit (tests/test_color_device.py); it is held to Pillow byte for byte, and its own properties are checked, on the CPU
(tests/test_color_cpu.py, tests/pillow_jitter_oracle.py)."""
import itertools

import numpy as np

F = np.float32
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
DEFAULTS = dict(brightness=0.1, contrast=0.1, saturation=0.1, hue=0.1)
B, C, S, H = 0, 1, 2, 3
ORDERS = list(itertools.permutations((B, C, S, H)))   # lexicographic


def range_factor(x, u):
    """float64, one operation per step, rounded once to float32"""
    x, u = float(x), float(u)
    a = 1.0 - x
    lo = a if a > 0.0 else 0.0
    hi = 1.0 + x
    d = hi - lo
    p = d * u
    return F(lo + p)


def hue_factor(hue, u):
    hue, u = float(hue), float(u)
    h2 = 2.0 * hue
    p = h2 * u
    return F(-hue + p)


def chain(cfg, u):
    """(fb, fc, fs, fh, the present steps in order) of one image from its five uniforms"""
    cfg = {**DEFAULTS, **cfg}
    fb, fc, fs = range_factor(cfg["brightness"], u[0]), range_factor(cfg["contrast"], u[1]), range_factor(cfg["saturation"], u[2])
    fh = hue_factor(cfg["hue"], u[3])
    k = min(int(np.floor(24.0 * float(u[4]))), 23)
    present = {B: cfg["brightness"] != 0, C: cfg["contrast"] != 0, S: cfg["saturation"] != 0, H: cfg["hue"] != 0}
    return fb, fc, fs, fh, [s for s in ORDERS[k] if present[s]]


def luma(img):
    """img [..., 3] integers -> L"""
    img = img.astype(np.int64)
    return (19595 * img[..., 0] + 38470 * img[..., 1] + 7471 * img[..., 2] + 32768) >> 16


def blend(d, x, f):
    """d, x integer arrays (broadcast), f float32 -> integers 0 .. 255"""
    d, x = np.asarray(d, np.int64), np.asarray(x, np.int64)
    t = F(f) * (x - d).astype(np.float32)
    r = d.astype(np.float32) + t
    assert t.dtype == np.float32 and r.dtype == np.float32
    return np.clip(r, F(0), F(255)).astype(np.int64)     # astype truncates


def mean_luma(img):
    n = img.shape[0] * img.shape[1]
    return (2 * int(luma(img).sum()) + n) // (2 * n)


def clip_rint(x):
    assert x.dtype == np.float32
    return np.clip(np.rint(x), F(0), F(255)).astype(np.int64)


def rgb_to_hsv(img, float32_only=False):
    """img [..., 3] integers -> (h, s, v), integers 0 .. 255: the forward conversion of step H.  float32_only: the hue as this
    project defined it before it was held to Pillow (every operation in float32), kept so that the tests can find the colours on
    which the two differ."""
    img = img.astype(np.int64)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    maxc, minc = img.max(-1), img.min(-1)
    v = maxc
    grey = minc == maxc
    cr = np.where(grey, 1, maxc - minc)                   # (grey pixels: any divisor, the result is discarded)
    fcr = cr.astype(np.float32)
    fmax = np.where(grey, 1, maxc).astype(np.float32)
    s = ((F(255) * fcr) / fmax).astype(np.int64)
    rc, gc, bc = ((maxc - ch).astype(np.float32) / fcr for ch in (r, g, b))
    assert rc.dtype == np.float32
    if float32_only:
        t = np.where(r == maxc, bc - gc, np.where(g == maxc, (F(2) + rc) - bc, (F(4) + gc) - rc))
        x = t / F(6) + F(1)
        hf = x - np.floor(x)
        h = (hf * F(255)).astype(np.int64)
        assert x.dtype == np.float32 and hf.dtype == np.float32
    else:
        D = np.float64
        rd, gd, bd = rc.astype(D), gc.astype(D), bc.astype(D)
        t = np.where(r == maxc, bc - gc, np.where(g == maxc, ((D(2) + rd) - bd).astype(np.float32), ((D(4) + gd) - rd).astype(np.float32)))
        assert t.dtype == np.float32
        x = t.astype(D) / D(6) + D(1)
        hf = (x - np.floor(x)).astype(np.float32)         # float64, rounded once
        h = (hf.astype(D) * D(255)).astype(np.int64)
    return np.where(grey, 0, h), np.where(grey, 0, s), v


def hue_shift(fh):
    """the float32 factor -> 0 .. 255: one float32 product, truncated toward zero, with a non-negative remainder"""
    return int(F(fh) * F(255)) % 256


def hsv_to_rgb(h, s, v):
    """integer arrays 0 .. 255 -> [..., 3]: the back conversion of step H"""
    h, s, v = (np.asarray(a, np.int64) for a in (h, s, v))
    i = (6 * h) // 255                                    # 0 .. 6
    f = (6 * h - 255 * i).astype(np.float32) / F(255)
    sg, fv = s.astype(np.float32) / F(255), v.astype(np.float32)
    p = clip_rint(fv * (F(1) - sg))
    q = clip_rint(fv * (F(1) - sg * f))
    t2 = clip_rint(fv * (F(1) - sg * (F(1) - f)))
    i = i % 6
    table = [(v, t2, p), (q, v, p), (p, v, t2), (p, q, v), (t2, p, v), (v, p, q)]
    out = np.empty(h.shape + (3,), np.int64)
    for c in range(3):
        out[..., c] = np.select([i == k for k in range(6)], [table[k][c] for k in range(6)])
    out[s == 0] = v[s == 0][:, None]
    return out


def hue_step(img, fh):
    h, s, v = rgb_to_hsv(img)
    return hsv_to_rgb((h + hue_shift(fh)) % 256, s, v)


def step(img, s, f):
    """one step of the chain on an integer image [h,w,3] with its float32 factor -> (the image, m of step C or None)"""
    if s == B:
        return blend(0, img, f), None
    if s == S:
        return blend(luma(img)[..., None], img, f), None
    if s == C:
        m = mean_luma(img)
        return blend(m, img, f), m
    return hue_step(img, f), None


def jitter_uint8(rgb, cfg, u):
    """one image [h,w,3] uint8 -> the jittered image, integers 0 .. 255 (int64), and the list of (step, m) applied"""
    fb, fc, fs, fh, steps = chain(cfg, u)
    img = rgb.astype(np.int64)
    trace = []
    for s in steps:
        img, m = step(img, s, {B: fb, C: fc, S: fs, H: fh}[s])
        trace.append((s, m))
    assert img.min() >= 0 and img.max() <= 255
    return img, trace


def normalize(img, mean=MEAN, std=STD):
    """[h,w,3] integers -> [3,h,w] float32"""
    x = (img.astype(np.float32) / F(255) - mean) / std
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def jitter_one(rgb, cfg, u, mask=None, maskmul=0):
    img, _ = jitter_uint8(rgb, cfg, u)
    x = normalize(img)
    if mask is not None and maskmul:
        x = x * mask.astype(np.float32)[None]
    return x


def jitter_batch(rgb, cfg, U, mask=None, maskmul=None):
    """rgb [b,h,w,3] uint8, U [b,5] -> [b,3,h,w] float32"""
    return np.stack([jitter_one(rgb[i], cfg, U[i], None if mask is None else mask[i], 0 if maskmul is None else int(maskmul[i]))
                     for i in range(len(rgb))])
