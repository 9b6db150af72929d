"""Inputs shared by tests/test_stem_cpu.py and tests/test_stem_device.py: the shapes, seeded real data at a trained stem's scales, the
exact integer data, the one-hot weights, and the fixture's input.  All on the CPU, float32 unless said."""
import os

import torch

from tests.tail_cases import ROOT, standin  # noqa: F401  (the seeded stand-in network of fixture G9)

# (b, h, w) of the IMAGE.  The kernel's tile is 64 x 4 x2s pixels (pooled: 32 x 2).
SHAPES = [
    (1, 32, 48),     # the G9 size
    (2, 37, 53),     # odd sides: the last window's right and bottom padding differs; Ho = 19 and Wo = 27 are odd, so the pool's far edge
                     # has no padding; Ho = 19 crosses the 4-row tiles four times by 3
    (1, 1, 1),       # every tap but one is padding; Ho = Wo = Hp = Wp = 1
    (3, 18, 262),    # Wo = 131 crosses the 64-pixel tile twice by 3 (the third tile has one column block only), Ho = 9 the 4-row tile
                     # twice by 1, with b = 3
    (1, 70, 8),      # Ho = 35 spans nine row tiles (the last of 3 rows) with Wo = 4
]
FIXTURE = os.path.join(ROOT, "tests", "golden", "stem.npz")
FIXTURE_SHAPE = (1, 3, 37, 53)


def out_sizes(h, w):
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return ho, wo, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1


def seeded(b, h, w, seed):
    """(image [b,3,h,w], (w [64,3,7,7], bias [64])) at a trained stem's scales: a normalised image of order 1, weights of order
    1 / sqrt(147), so that pre-activations are of order 1 and of both signs"""
    g = torch.Generator().manual_seed(seed)
    image = torch.randn(b, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 7, 7, generator=g) * 147 ** -0.5
    bias = torch.randn(64, generator=g) * 0.2
    return image, (wt, bias)


INT_W, INT_X, INT_BIAS = 128, 4, 50   # the largest |w|, |x| and |bias| of the integer data: every partial sum below 147 * 128 * 4 + 50 < 2^24


def integers(b, h, w, seed):
    """Exact integer data: image integers in -4 .. 4, weights in -128 .. 128 (at most eight significant bits: exact in bfloat16), an
    integer bias in +-50.  Every partial sum in any order is an integer below 2^24, so the kernel must give THE integers' ReLU."""
    g = torch.Generator().manual_seed(seed)
    image = torch.randint(-INT_X, INT_X + 1, (b, 3, h, w), generator=g).float()
    wt = torch.randint(-INT_W, INT_W + 1, (64, 3, 7, 7), generator=g).float()
    bias = torch.randint(-INT_BIAS, INT_BIAS + 1, (64,), generator=g).float()
    return image, (wt, bias)


ONEHOT_SETS = 3   # 3 * 64 >= 147


def onehot(k):
    """(taps, w, bias) of set k < 3: output channel o takes the one (c, ky, kx) = taps[o] with flat index (64 k + o) mod 147, weight +1
    for even o and -1 for odd o, every other weight 0, bias 0.  Over the three sets each of the 147 taps occurs."""
    taps, wt = [], torch.zeros(64, 3, 7, 7)
    for o in range(64):
        t = (64 * k + o) % 147
        c, ky, kx = t // 49, (t % 49) // 7, t % 7
        taps.append((c, ky, kx))
        wt[o, c, ky, kx] = 1.0 if o % 2 == 0 else -1.0
    return taps, wt, torch.zeros(64)


def fixture_input():
    """the seeded input the fixture tests/golden/stem.npz was recorded on (tests/golden/make_stem_golden.py)"""
    return torch.randn(*FIXTURE_SHAPE, generator=torch.Generator().manual_seed(1234))
