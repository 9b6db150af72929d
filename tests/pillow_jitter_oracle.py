"""The colour jitter as the reference's training loop computes it: torchvision 0.2.1's ``adjust_brightness``, ``adjust_contrast``,
``adjust_saturation`` and ``adjust_hue`` (transforms/functional.py of that release), restated with the Pillow calls they consist of
and nothing else.  An oracle this project's definition (include/pvnet_color.h, tests/color_restatement.py) is held to byte for byte;
tests/golden/color_pillow.npz records its results so that a machine without Pillow can compare with them.

It takes the project's float32 factors as ``color_restatement.chain`` gives them and does no arithmetic of its own beyond the hue
shift.  PIL is imported lazily: importing this module needs only numpy."""
import numpy as np

B, C, S, H = 0, 1, 2, 3   # color_restatement's step numbers


def pil_version():
    import PIL
    return PIL.__version__


def to_pil(rgb):
    from PIL import Image
    rgb = np.ascontiguousarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    return Image.fromarray(rgb)


def adjust_brightness(img, factor):
    from PIL import ImageEnhance
    return ImageEnhance.Brightness(img).enhance(factor)


def adjust_contrast(img, factor):
    from PIL import ImageEnhance
    return ImageEnhance.Contrast(img).enhance(factor)


def adjust_saturation(img, factor):
    from PIL import ImageEnhance
    return ImageEnhance.Color(img).enhance(factor)


def hue_shift(fh):
    """np.uint8(hue_factor * 255) as x86 computes it: a double product, truncated toward zero, with a non-negative remainder"""
    return int(float(fh) * 255.0) % 256


def adjust_hue(img, factor):
    from PIL import Image
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(hue_shift(factor))            # the wrapped uint8 add
    h = Image.fromarray(np_h)
    return Image.merge("HSV", (h, s, v)).convert("RGB")


def rgb_to_hsv(rgb):
    """[..., 3] uint8 -> Pillow's (h, s, v), uint8 arrays"""
    hsv = np.asarray(to_pil(rgb).convert("HSV"))
    return hsv[..., 0], hsv[..., 1], hsv[..., 2]


def hsv_to_rgb(h, s, v):
    """uint8 arrays [a, b] -> Pillow's RGB [a, b, 3]"""
    from PIL import Image
    planes = [Image.fromarray(np.ascontiguousarray(p, dtype=np.uint8)) for p in (h, s, v)]
    return np.asarray(Image.merge("HSV", planes).convert("RGB"))


STEPS = {B: adjust_brightness, C: adjust_contrast, S: adjust_saturation, H: adjust_hue}


def apply_chain(rgb, factors, steps):
    """rgb [h,w,3] uint8; factors (fb, fc, fs, fh), float32; steps: the present steps in order -> uint8 [h,w,3]"""
    fb, fc, fs, fh = factors
    img = to_pil(rgb)
    for s in steps:
        img = STEPS[s](img, float({B: fb, C: fc, S: fs, H: fh}[s]))
    return np.asarray(img).copy()


def jitter_uint8(rgb, cfg, u):
    """the counterpart of color_restatement.jitter_uint8: its factors and order, Pillow's arithmetic"""
    from tests import color_restatement as RS
    fb, fc, fs, fh, steps = RS.chain(cfg, u)
    return apply_chain(rgb, (fb, fc, fs, fh), steps)
