"""Writes tests/golden/color_pillow.npz: what Pillow gives for 48 chains of the colour jitter over one 32 x 40 image, recorded so
that a machine without Pillow can hold the kernels to Pillow's bytes (tests/test_color_cpu.py, tests/test_color_device.py).

    python tests/golden/make_color_golden.py

Needs Pillow (tests/pillow_jitter_oracle.py is the oracle); the version is stored in the file.

  image    [32,40,3] uint8.  Rows 0 .. 15: 640 colours on which a hue computed in float32 throughout differs from Pillow's (drawn from
           the exhaustive list over all 2^24 colours, a third from each maxc branch).  Rows 16 .. 31: random colours, a grey ramp, pure
           primaries and secondaries, and maxc == minc pixels.
  ranges   [48,4] float64: brightness, contrast, saturation, hue of each case (0: the step is absent).  Case 2 k: order k, all four
           steps, wide ranges.  Case 2 k + 1: order k, the reference's ranges, step (k mod 4) absent.
  uniforms [48,2,5] float64: two draws per case, the first with a negative hue factor, the second with a positive one.
  want     [48,2,32,40,3] uint8: Pillow's result.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import color_restatement as RS  # noqa: E402
from tests import pillow_jitter_oracle as PO  # noqa: E402

OUT = os.path.join(HERE, "color_pillow.npz")
H, W = 32, 40
KEYS = ("brightness", "contrast", "saturation", "hue")
WIDE = dict(brightness=0.6, contrast=0.7, saturation=0.8, hue=0.5)


def hard_colours():
    """every colour on which the float32-only hue and the definition's differ, [n,3] uint8 in lexicographic order"""
    out = []
    for r0 in range(0, 256, 16):
        r, g, b = np.meshgrid(np.arange(r0, r0 + 16), np.arange(256), np.arange(256), indexing="ij")
        img = np.stack([r, g, b], -1).reshape(-1, 3).astype(np.uint8)
        out.append(img[RS.rgb_to_hsv(img)[0] != RS.rgb_to_hsv(img, float32_only=True)[0]])
    return np.concatenate(out)


def branch(colours):
    """0: r == maxc, 1: g == maxc (and not r), 2: b alone"""
    c = colours.astype(np.int64)
    m = c.max(1)
    return np.where(c[:, 0] == m, 0, np.where(c[:, 1] == m, 1, 2))


def make_image(rng):
    hard = hard_colours()
    br = branch(hard)
    picks = [hard[br == k][rng.choice(int((br == k).sum()), n, replace=False)] for k, n in ((0, 213), (1, 213), (2, 214))]
    top = rng.permutation(np.concatenate(picks))
    ramp = np.repeat(np.linspace(0, 255, 3 * W).round().astype(np.uint8)[:, None], 3, 1)                  # 3 rows of grey
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
    prim = np.tile(prim, (W // 8, 1))                                                                     # 1 row
    flat = np.repeat(rng.integers(0, 256, (W, 1), dtype=np.uint8), 3, 1)                                  # 1 row of maxc == minc
    rand = rng.integers(0, 256, (11 * W, 3), dtype=np.uint8)
    image = np.concatenate([top, rand, ramp, prim, flat]).reshape(H, W, 3)
    return image, len(hard)


def make_cases(rng):
    ranges, uniforms = np.zeros((48, 4)), np.zeros((48, 2, 5))
    for k in range(24):
        for copy in range(2):
            cfg = dict(WIDE) if copy == 0 else dict(RS.DEFAULTS, **{KEYS[k % 4]: 0})
            ranges[2 * k + copy] = [cfg[key] for key in KEYS]
            u = rng.uniform(0.0, 1.0, (2, 5))
            u[0, 3], u[1, 3] = rng.uniform(0.05, 0.45), rng.uniform(0.55, 0.95)
            u[:, 4] = (k + 0.5) / 24
            uniforms[2 * k + copy] = u
    return ranges, uniforms


def main():
    rng = np.random.default_rng(20240)
    image, n_hard = make_image(rng)
    ranges, uniforms = make_cases(rng)
    want = np.zeros((48, 2, H, W, 3), np.uint8)
    for c in range(48):
        cfg = dict(zip(KEYS, ranges[c]))
        for j in range(2):
            assert (RS.hue_factor(cfg["hue"], uniforms[c, j, 3]) < 0) == (j == 0) or cfg["hue"] == 0
            want[c, j] = PO.jitter_uint8(image, cfg, uniforms[c, j])
    np.savez_compressed(OUT, image=image, ranges=ranges, uniforms=uniforms, want=want, pil_version=np.array(PO.pil_version()),
                        hard_colours=np.array(n_hard))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, Pillow {PO.pil_version()}, {n_hard} hard colours")


if __name__ == "__main__":
    main()
