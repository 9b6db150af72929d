"""Label images and key-points per class shared by tests/test_class_targets_cpu.py and tests/test_class_targets_device.py.

Every builder returns int64 labels [b,h,w] for ``class_num`` classes (the background counted); ``as_dtype`` stores them as a tensor
type can hold them.  The builders: three discs (a lane's eight pixels mostly of one class), vertical stripes of period 3 and 5 (a
lane's eight pixels mix classes and cross class boundaries mid-lane, column 0 in class 1), a class that is absent, labels 0, -1,
class_num and 255 planted among the others, and a batch whose second image has no foreground."""
import numpy as np


def three_discs(b, h, w, class_num, seed=0):
    """three discs per image, of the classes 1 + (i + j) % nk, a later disc over an earlier one"""
    rng = np.random.default_rng(seed)
    nk = class_num - 1
    yy, xx = np.mgrid[:h, :w]
    labels = np.zeros((b, h, w), np.int64)
    for i in range(b):
        for j in range(3):
            cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
            r = 0.22 * max(min(h, w), 2)
            labels[i][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 1 + (i + j) % nk
    labels[:, 0, 0] = 1   # a target pixel in every image, the 1 x 1 one included
    return labels


def stripes(b, h, w, class_num, period):
    """vertical stripes `period` pixels wide through the labels 1, 2, .., nk, 0, 1, ..: column 0 of image 0 is of class 1, and image i
    is shifted by i classes"""
    x = np.arange(w)[None, None, :]
    i = np.arange(b)[:, None, None]
    return np.broadcast_to((x // period + 1 + i) % class_num, (b, h, w)).astype(np.int64).copy()


def absent_class(b, h, w, class_num, seed=1):
    """the discs without the last class (class_num >= 3), which its key-points must not touch; class_num == 2: no foreground at all"""
    labels = three_discs(b, h, w, class_num, seed)
    labels[labels == class_num - 1] = 0
    return labels


def planted(b, h, w, class_num, seed=2):
    """the stripes of period 5 with the labels 0, -1, class_num and 255 planted at random pixels (about one in sixteen each)"""
    rng = np.random.default_rng(seed)
    labels = stripes(b, h, w, class_num, 5)
    for value in (0, -1, class_num, 255):
        labels[rng.random((b, h, w)) < 1.0 / 16] = value
    if h * w > 4:
        labels.reshape(b, -1)[:, :4] = (0, -1, class_num, 255)   # each of them at least once
    return labels


def no_foreground(b, h, w, class_num, seed=3):
    """the discs with image 1 (or the only one) emptied"""
    labels = three_discs(b, h, w, class_num, seed)
    labels[min(1, b - 1)] = 0
    return labels


BUILDERS = {
    "discs": three_discs,
    "stripes3": lambda b, h, w, c: stripes(b, h, w, c, 3),
    "stripes5": lambda b, h, w, c: stripes(b, h, w, c, 5),
    "absent": absent_class,
    "planted": planted,
    "empty": no_foreground,
}


def as_dtype(labels, np_dtype):
    """the labels as `np_dtype` stores them: what it cannot hold (-1 in uint8, anything but 0 / 1 in bool) becomes a value of the same
    kind that it can (255: outside every class; True for a class only where class_num == 2 makes that the same label)"""
    if np_dtype == np.uint8:
        return np.where(labels < 0, 255, labels).astype(np.uint8)
    if np_dtype == np.bool_:
        return labels == 1
    return labels.astype(np_dtype)


def class_keypoints(labels, class_num, vn, seed, planted_points=True, minus_zero=False):
    """[b,nk,vn,3] float64 key-points, hz in [0.5, 2], all different between the classes.  With `planted_points`, per class that has
    pixels: key-point 0 exactly ON one of them (n = 0), key-point 1 5e-4 beside one (0 < n < 1e-3), both with hz = 1, and key-point 2
    with hz = 0.  With `minus_zero` the last key-point of class 1 is (-0.0, hy, 0): vx = -0.0 - x * 0 = -0.0 at every pixel, so that
    class's x target is -0.0, normalised or not."""
    rng = np.random.default_rng(seed)
    b, h, w = labels.shape
    nk = class_num - 1
    hz = rng.uniform(0.5, 2.0, (b, nk, vn, 1))
    hc = np.concatenate([rng.uniform(-0.5 * w, 1.5 * w, (b, nk, vn, 1)) * hz, rng.uniform(-0.5 * h, 1.5 * h, (b, nk, vn, 1)) * hz, hz], 3)
    if planted_points:
        for i in range(b):
            for k in range(nk):
                ys, xs = np.nonzero(labels[i] == k + 1)
                if len(ys) == 0:
                    continue
                j = rng.integers(len(ys), size=2)
                hc[i, k, 0] = (xs[j[0]], ys[j[0]], 1.0)
                if vn > 1:
                    hc[i, k, 1] = (xs[j[1]] + 5e-4, ys[j[1]], 1.0)
                if vn > 2:
                    hc[i, k, 2, 2] = 0.0
    if minus_zero:
        hc[:, 0, vn - 1] = (-0.0, 3.25, 0.0)
    return hc


def bits(a):
    """the bit patterns of a float32 array: -0.0 and +0.0 differ, a NaN equals itself"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)
