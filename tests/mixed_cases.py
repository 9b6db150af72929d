"""Inputs of the mixed-batch tests (tests/test_mixed_batches_cpu.py, tests/test_mixed_batches_device.py): batches in which live, empty,
below-min_num and few-pixel images stand side by side at layouts with culling buffers (768 <= hn <= 1024, b * vn >= 64, vn <= 32), and
label batches whose absent classes lie between the present ones.  numpy only; importable without a GPU.

All images are 96 x 128 = 12 288 pixels: three 4096-pixel segments, 192 words of 64 pixels, the last one full.  An image is of one KIND:

  empty                    no foreground
  below_min                3 pixels (min_num = 5)
  at_min                   exactly 5 pixels, clean field
  tile                     20 pixels (less than one 32-pixel tile), clean field
  item_m1, item, item_p1   255, 256, 257 pixels (one 256-pixel item less one / exactly / plus one): rectangles cut to the count, clean field
  clean                    disc of radius 30, ground-truth field, zero background
  noisy                    disc of radius 30, sigma 0.05 rad and 10 % outliers, N(0,1) background
  thinned                  the whole frame foreground, noisy, voted with max_num = 1500
  ties                     a clean disc whose key-points lie on integer coordinates (its hypotheses scatter over the four 1/8-pixel cells
                           that meet there, so the Hilbert order of a culled key-point is not the caller's), voted with explicit idxs: slots
                           0 .. 4 hold degenerate pairs, 40 slots spread over the hn hold ONE pixel pair -- identical hypotheses, equal counts
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import ransac_voting_oracle as O
from pvnet_amd import synth

H, W = 96, 128
MIN_NUM = 5
RADIUS = 30
THIN_MAX_NUM = 1500
PIXELS = {"empty": 0, "below_min": 3, "at_min": 5, "tile": 20, "item_m1": 255, "item": 256, "item_p1": 257}
DISC_KINDS = ("clean", "noisy", "ties")
KINDS = ("empty", "below_min", "at_min", "tile", "item_m1", "item", "item_p1", "clean", "noisy", "thinned", "ties")
DEAD_KINDS = ("empty", "below_min")
CLEAN_KINDS = ("at_min", "tile", "item_m1", "item", "item_p1", "clean", "ties")   # the field points at the key-points exactly
LABEL_KINDS = ("below_min", "at_min", "tile", "item_m1", "item", "item_p1", "clean", "noisy")   # what a class of a label image may be
TIE_SLOTS, TIE_FIRST = 40, 5

# ---- the cases of the device module: (b, h, w, vn, hn, max_num) of every call it makes ----------------------------------------------
V3_B, V3_VN = 8, 9
N_PERMUTATIONS = 12
HN_PADDED = 1000                      # padding columns inside the last tile of 32
HN_PERMUTATIONS = (2, 3)              # the permutations also run at hn = 1000
THRESH_PERMUTATIONS = (4, 9)          # ... and at thresh 0.9 and 0.999
HISTORY_PERMUTATION = 5
REF_KERNEL_PERMUTATION = 8
TIES_ORDER = ("empty", "ties", "at_min", "clean", "below_min", "tile", "item_p1", "noisy")   # the ties test's batch (seed TIES_SEED)
TIES_SEED = 77
V2_CASES = ((2, 14, 3), (1, 64, 2), (8, 4, 3))   # (b, class_num, vn); the last with every class present


def permutation(index: int) -> tuple:
    """eight of the eleven kinds, `empty` and `below_min` always among them; index 0 starts with a dead image, index 1 ends with one"""
    rng = np.random.default_rng([77, index])
    others = [k for k in KINDS if k not in DEAD_KINDS]
    chosen = [others[(4 * index + j) % len(others)] for j in range(V3_B - 2)]
    order = [str(k) for k in rng.permutation(chosen + list(DEAD_KINDS))]
    if index == 0 and order[0] not in DEAD_KINDS:
        j = order.index("empty")
        order[0], order[j] = order[j], order[0]
    if index == 1 and order[-1] not in DEAD_KINDS:
        j = order.index("below_min")
        order[-1], order[j] = order[j], order[-1]
    return tuple(order)


def batch_max_num(order) -> int:
    return THIN_MAX_NUM if "thinned" in order else 30000


def v3_shapes() -> list:
    """(b, h, w, vn, hn, max_num) of every v3 call of the device module"""
    out = []
    for i in range(N_PERMUTATIONS):
        mx = batch_max_num(permutation(i))
        out.append((V3_B, H, W, V3_VN, 1024, mx))
        if i in HN_PERMUTATIONS:
            out.append((V3_B, H, W, V3_VN, HN_PADDED, mx))
    out.append((V3_B, H, W, V3_VN, 1024, 30000))   # the batch of eight empty images, the ties batch
    return sorted(set(out))


def v2_shapes() -> list:
    """(B, h, w, vn, hn, max_num) of every per-class call of the device module: B = b (class_num - 1) virtual images"""
    return [(b * (cn - 1), H, W, vn, 1024, 30000) for b, cn, vn in V2_CASES]


# ---- one image -----------------------------------------------------------------------------------------------------------------------
def rectangle(n: int, x0: int, y0: int) -> np.ndarray:
    """the first n pixels, in raster order, of a rectangle min(16, ceil(sqrt(n))) wide at (x0, y0)"""
    fg = np.zeros((H, W), bool)
    if n == 0:
        return fg
    wd = min(16, int(np.ceil(np.sqrt(n))))
    i = np.arange(n)
    fg[y0 + i // wd, x0 + i % wd] = True
    assert int(fg.sum()) == n
    return fg


def region(kind: str, cx: int, cy: int) -> np.ndarray:
    """the foreground of a kind about (cx, cy); a rectangle's corner lies there"""
    if kind == "thinned":
        return np.ones((H, W), bool)
    if kind in DISC_KINDS:
        return synth.disk_mask(H, W, cx, cy, RADIUS)
    return rectangle(PIXELS[kind], cx, cy)


def keypoints(kind: str, fg: np.ndarray, vn: int, rng) -> np.ndarray:
    ys, xs = np.nonzero(fg)
    cx, cy = float(xs.mean()), float(ys.mean())
    if kind == "ties":   # integer coordinates on a ring outside the disc
        ang = 2 * np.pi * (np.arange(vn) + 0.25) / vn
        return np.stack([np.round(cx) + np.round(36 * np.cos(ang)), np.round(cy) + np.round(36 * np.sin(ang))], 1)
    r = 1.5 * RADIUS if kind in DISC_KINDS or kind == "thinned" else 20.0
    return np.stack([rng.uniform(cx - r, cx + r, vn), rng.uniform(cy - r, cy + r, vn)], 1)


def paint(planar: np.ndarray, kind: str, fg: np.ndarray, kp: np.ndarray, rng):
    """write the kind's field on its own pixels of planar [2vn,h,w]"""
    if not fg.any():
        return
    own = synth.field_from_keypoints(fg, kp)
    if kind in ("noisy", "thinned"):
        own = synth.add_noise(own, fg, rng, sigma_rad=0.05, outlier_frac=0.10)
    planar[:, fg] = own[:, fg]


def kept_pixels(fg: np.ndarray, seed: int, image: int, max_num: int) -> int:
    """tn: the pixels the layer keeps of an image with tn0 = fg.sum() pixels (thinning above max_num)"""
    tn0 = int(fg.sum())
    if tn0 <= max_num:
        return tn0
    return int((fg.reshape(-1) & O.subsample_keep(seed, image, H * W, max_num, tn0)).sum())


def tie_idxs(hn: int, vn: int, tn: int, rng) -> np.ndarray:
    """[hn,vn,2] for a `ties` image: random pairs, slots 0 .. TIE_FIRST-1 degenerate (a pixel with itself: the zero hypothesis), TIE_SLOTS
    slots from TIE_FIRST on, spread over the hn, all holding key-point k's one pair"""
    ix = rng.integers(0, tn, (hn, vn, 2)).astype(np.int32)
    ix[:TIE_FIRST, :, 1] = ix[:TIE_FIRST, :, 0]
    slots = tie_slots(hn)
    for k in range(vn):
        ix[slots, k] = (10 + 7 * k, tn - 11 - 5 * k)
    return ix


def tie_slots(hn: int) -> np.ndarray:
    return np.linspace(TIE_FIRST, hn - 4, TIE_SLOTS).astype(np.int64)


class MixedBatch(NamedTuple):
    mask: np.ndarray        # [b,96,128] uint8
    planar: np.ndarray      # [b,2vn,96,128] float32
    kinds: tuple
    kpts: np.ndarray        # [b,vn,2] the generating key-points (NaN for empty images)
    max_num: int
    call_seed: int          # the seed the batch is voted with (the thinning and the draws follow it)
    idxs: object            # None, or [b,hn,vn,2] int32 when the batch holds a `ties` image: the layer's own draws for every other image


def mixed_batch(order, vn: int = V3_VN, seed: int = 0, hn: int = 1024) -> MixedBatch:
    """one image per entry of `order`"""
    rng = np.random.default_rng(8800 + seed)
    b = len(order)
    mask = np.zeros((b, H, W), np.uint8)
    planar = np.zeros((b, 2 * vn, H, W), np.float32)
    kpts = np.full((b, vn, 2), np.nan)
    max_num, call_seed = batch_max_num(order), 1000 + seed
    for i, kind in enumerate(order):
        if kind in DISC_KINDS:
            cx, cy = 64 + int(rng.integers(-20, 21)), 48 + int(rng.integers(-10, 11))
        else:
            cx, cy = int(rng.integers(0, W - 16)), int(rng.integers(0, H - 17))
        fg = region(kind, cx, cy)
        if kind not in CLEAN_KINDS:
            planar[i] = rng.standard_normal((2 * vn, H, W)).astype(np.float32)
        if fg.any():
            kpts[i] = keypoints(kind, fg, vn, rng)
            paint(planar[i], kind, fg, kpts[i], rng)
        mask[i] = fg
    idxs = None
    if "ties" in order:
        idxs = np.zeros((b, hn, vn, 2), np.int32)
        for i, kind in enumerate(order):
            tn = kept_pixels(mask[i] != 0, call_seed, i, max_num)
            if kind == "ties":
                idxs[i] = tie_idxs(hn, vn, tn, rng)
            elif kind not in DEAD_KINDS:
                idxs[i] = O.draw_idxs(call_seed, i, hn, vn, tn)
    return MixedBatch(mask, planar, tuple(order), kpts, max_num, call_seed, idxs)


def rolled(batch: MixedBatch) -> MixedBatch:
    """the same images one slot further: every slot changes kind.  (Not for a batch with explicit idxs: an image's draws follow its slot.)"""
    assert batch.idxs is None
    r = lambda a: np.ascontiguousarray(np.roll(a, 1, axis=0))   # noqa: E731
    return MixedBatch(r(batch.mask), r(batch.planar), tuple(str(k) for k in np.roll(np.array(batch.kinds, object), 1)), r(batch.kpts),
                      batch.max_num, batch.call_seed, None)


# ---- label images ----------------------------------------------------------------------------------------------------------------------
DISC_SLOTS = ((31, 48), (96, 48))                                             # discs of radius 30: rows 18 .. 78
RECT_SLOTS = tuple((16 * j, y0) for y0 in (0, 79) for j in range(8))          # 16 x 17 pixels each: rows 0 .. 16 and 79 .. 95
STRAY_ROW = 17                                                                # between the upper rectangles and the discs: nobody's labels


class LabelBatch(NamedTuple):
    labels: np.ndarray      # [b,96,128] int64
    field: np.ndarray       # [b,96,128,vn,2] float32, contiguous
    kinds: np.ndarray       # [b,class_num-1] of str: `empty` for an absent class
    kpts: np.ndarray        # [b,class_num-1,vn,2], NaN for absent classes


def label_batch(b: int, class_num: int, vn: int, present, seed: int = 0) -> LabelBatch:
    """`present`: per image a dict {label: kind} with kinds of LABEL_KINDS (at most two discs and sixteen rectangles an image); the regions
    do not overlap, every other class is absent, and labels 0, -1, class_num and 255 lie on pixels that belong to nobody.  The field
    is N(0,1) where no class is."""
    assert len(present) == b
    rng = np.random.default_rng(9900 + seed)
    nk = class_num - 1
    labels = np.zeros((b, H, W), np.int64)
    planar = rng.standard_normal((b, 2 * vn, H, W)).astype(np.float32)
    kinds = np.full((b, nk), "empty", object)
    kpts = np.full((b, nk, vn, 2), np.nan)
    for i, classes in enumerate(present):
        discs, rects = list(DISC_SLOTS), [RECT_SLOTS[j] for j in rng.permutation(len(RECT_SLOTS))]
        for label in sorted(classes):
            kind = classes[label]
            assert kind in LABEL_KINDS and 1 <= label < class_num
            fg = region(kind, *(discs.pop(0) if kind in DISC_KINDS else rects.pop(0)))
            assert not (labels[i][fg] != 0).any()
            labels[i][fg] = label
            kinds[i, label - 1] = kind
            kpts[i, label - 1] = keypoints(kind, fg, vn, rng)
            paint(planar[i], kind, fg, kpts[i, label - 1], rng)
        labels[i, STRAY_ROW, 0:4] = (class_num, 255, -1, 0)
        labels[i, STRAY_ROW, W - 4:W] = (-1, class_num, 255, class_num + 1)
    field = np.ascontiguousarray(synth.planar_to_vertex_view(planar))
    return LabelBatch(labels, field, kinds, kpts)


def v2_present(case) -> list:
    """the classes of the device module's label batches"""
    b, cn, vn = case
    if (b, cn) == (2, 14):    # three live objects an image and one below min_num: ten of thirteen virtual images are dead, between the live ones
        return [{2: "clean", 6: "item_p1", 8: "below_min", 11: "tile"}, {1: "noisy", 4: "below_min", 7: "at_min", 13: "item"}]
    if (b, cn) == (1, 64):
        return [{1: "clean", 10: "below_min", 20: "item_m1", 33: "tile", 47: "noisy", 55: "item", 63: "at_min"}]
    small = ("item_m1", "item", "item_p1", "tile", "at_min")
    return [{1: ("clean", "noisy")[i % 2], 2: small[i % 5], 3: small[(i + 2) % 5]} for i in range(b)]   # every class present and live


def v2_present_changed() -> list:
    """(2, 14, 3) with class 6 of image 0 gone and class 3 there instead: one class vanishes, one appears"""
    p = v2_present((2, 14, 3))
    return [{2: "clean", 3: "item", 8: "below_min", 11: "tile"}, p[1]]


def materialised_masks(labels: np.ndarray, class_num: int) -> np.ndarray:
    """[b (class_num - 1), h, w] uint8: mask[i] == k + 1 in the order (i, k)"""
    return np.stack([(labels[i] == k + 1) for i in range(labels.shape[0]) for k in range(class_num - 1)]).astype(np.uint8)
