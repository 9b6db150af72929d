"""Inputs shared by tests/test_trunk_cpu.py and tests/test_trunk_device.py: the geometries, widths and shapes, seeded real data at a
trained trunk's scales, the exact integer data and the one-hot weights.  All on the CPU, float32 unless said."""
import torch

GEOMETRIES = [(1, 1), (2, 1), (1, 2), (1, 4)]   # (stride, dilation): layer1 / fc / conv8s, layer2[0].conv1, layer3, layer4

# (c1, c2, co).  The kernel stages In in chunks of 32 channels and gives a workgroup a group of 128 output channels, 32 per wave:
#   (32, 0, 32)    one chunk, one wave at work
#   (64, 32, 96)   two sources, a chunk boundary inside src1 and the boundary between the sources; three waves at work
#   (32, 32, 160)  co crosses the group of 128 by a remainder of 32: a second group with one wave at work
SMALL_TRIPLES = [(32, 0, 32), (64, 32, 96), (32, 32, 160)]
# the widest a launch takes and conv8s' own two sources, once each at TINY: sixteen chunks x four groups, twelve chunks x one group
FULL_TRIPLES = [(512, 0, 512), (256, 128, 128)]
TINY = (1, 3, 5)

# (b, ho, wo) of the OUTPUT.  The kernel's tile is 32 x 8 output pixels:
#   (1, 1, 1)     one pixel: every off-centre tap is padding
#   (2, 3, 5)     sides below d = 4: at that dilation every off-centre tap is padding; two images
#   (1, 19, 27)   odd sides, three row tiles (8 + 8 + 3); from a 37 x 53 input under stride 2
#   (3, 9, 67)    b = 3; the width crosses the tile's 32 twice by a remainder of 3, the height crosses its 8 by 1
#   (1, 70, 5)    tall and narrow: nine row tiles of one column tile
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 19, 27), (3, 9, 67), (1, 70, 5)]


def in_sides(ho, wo, s, even=False):
    """the input sides an output of ho x wo is computed from under stride s: the odd ones (the last window's centre is the last pixel),
    or, with ``even``, one more (a last row and column that only the far taps reach)"""
    return (ho, wo) if s == 1 else (2 * ho - 1 + bool(even), 2 * wo - 1 + bool(even))


def seeded(b, ho, wo, triple, s, seed, even=False):
    """(src1 [b,c1,h,w], src2 [b,c2,h,w] or None, res [b,co,ho,wo], (w, bias)) at the scales of a trained trunk: activations of order 1
    behind a ReLU, weights of order 1 / sqrt(9 cin)"""
    c1, c2, co = triple
    h, w = in_sides(ho, wo, s, even)
    g = torch.Generator().manual_seed(seed)
    src1 = torch.relu(torch.randn(b, c1, h, w, generator=g))
    src2 = torch.relu(torch.randn(b, c2, h, w, generator=g)) if c2 else None
    res = torch.relu(torch.randn(b, co, ho, wo, generator=g))
    wt = torch.randn(co, c1 + c2, 3, 3, generator=g) * (9 * (c1 + c2)) ** -0.5
    bias = torch.randn(co, generator=g) * 0.2
    return src1, src2, res, (wt, bias)


INT_W, INT_X, INT_R = 128, 4, 50   # the largest |w|, |x| and |res| of the integer data
INT_BIAS = 1 << 20                  # above every |sum|, so that no pre-activation is negative


def integers(b, ho, wo, triple, s, seed):
    """Exact integer data: every operand a small integer that bfloat16 holds exactly, every partial sum in any order an integer below
    2^24, so the kernel must give THE integers, whatever its order of summation.
      src1, src2   integers in -4 .. 4, different at every pixel
      w            seeded integers in -128 .. 128 (at most eight significant bits: exact in bfloat16)
      bias         2^20 + a small integer: above every |sum| <= 9 * 192 * 128 * 4 < 2^20 at the small widths, so no pre-activation is
                   negative and ReLU leaves the integers alone
      res          integers in -50 .. 50; bias + |sum| + |res| < 2^21"""
    c1, c2, co = triple
    assert 9 * (c1 + c2) * INT_W * INT_X < INT_BIAS - 100
    h, w = in_sides(ho, wo, s)
    g = torch.Generator().manual_seed(seed)
    src1 = torch.randint(-INT_X, INT_X + 1, (b, c1, h, w), generator=g).float()
    src2 = torch.randint(-INT_X, INT_X + 1, (b, c2, h, w), generator=g).float() if c2 else None
    res = torch.randint(-INT_R, INT_R + 1, (b, co, ho, wo), generator=g).float()
    wt = torch.randint(-INT_W, INT_W + 1, (co, c1 + c2, 3, 3), generator=g).float()
    bias = (INT_BIAS + torch.randint(-50, 51, (co,), generator=g)).float()
    return src1, src2, res, (wt, bias)


def onehot(triple, seed):
    """(taps, w, bias): per output channel o one (c, ky, kx, sign) = taps[o], w[o][c][ky][kx] = sign = +-1 and every other weight 0,
    bias 0.  Over the output channels every tap occurs (o runs through a seeded order of the nine, again and again), the signs
    alternate every nine channels, and with two sources both alternate: a channel of src1 for even o, of src2 for odd o, seeded; the
    first and the last channel of each source are taken too (the chunk boundaries of the concatenation)."""
    c1, c2, co = triple
    g = torch.Generator().manual_seed(seed)
    order = torch.randperm(9, generator=g).tolist()
    fixed = {0: 0, 2: c1 - 1}
    if c2:
        fixed.update({1: c1, 3: c1 + c2 - 1})
    taps = []
    for o in range(co):
        if o in fixed:
            c = fixed[o]
        elif c2 and o % 2:
            c = c1 + int(torch.randint(0, c2, (1,), generator=g))
        else:
            c = int(torch.randint(0, c1, (1,), generator=g))
        t = order[o % 9]
        taps.append((c, t // 3, t % 3, -1.0 if (o // 9) % 2 else 1.0))
    assert {3 * ky + kx for _, ky, kx, _ in taps} == set(range(9)) and {sg for *_, sg in taps} == {1.0, -1.0}
    assert not c2 or {c < c1 for c, *_ in taps} == {True, False}
    wt = torch.zeros(co, c1 + c2, 3, 3)
    for o, (c, ky, kx, sg) in enumerate(taps):
        wt[o, c, ky, kx] = sg
    return taps, wt, torch.zeros(co)


FIXTURE_SHAPE = (1, 3, 64, 88)   # the pooled tensor is 16 x 22, the features at stride 8 are 8 x 11: odd width, sides above d = 4


def fixture_input():
    """the seeded input the fixture tests/golden/trunk.npz was recorded on (tests/golden/make_trunk_golden.py)"""
    return torch.randn(*FIXTURE_SHAPE, generator=torch.Generator().manual_seed(4321))


def standin():
    """the seeded stand-in of fixture G9 (tests/tail_cases.py makes it)"""
    from tests.tail_cases import standin as make
    return make()[0]
