"""Inputs shared by tests/test_decoder_cpu.py and tests/test_decoder_device.py: the shapes, seeded real data at a trained decoder's
scales, the exact integer data and the one-hot weights.  All on the CPU, float32 unless said."""
import torch

from tests.tail_cases import SHAPES, standin  # noqa: F401  ((b, h, w) of the OUTPUT: the G9 size, a width that is no multiple of 32, a
#          width that crosses a 64-pixel tile by 2 with b = 3, hin = win = 1, thin and wider than two tiles; the seeded stand-in network)

TRIPLES = [(64, 64, 32), (128, 64, 64)]   # (cl, cs, co): conv2s and conv4s of Resnet18_8s
STAGE_OF = {(64, 64, 32): "conv2s", (128, 64, 64): "conv4s"}


def seeded(b, h, w, triple, seed):
    """(lo [b,cl,h/2,w/2], skip [b,cs,h,w], (w, bias)) at the scales of a trained decoder, drawn as tests/tail_cases.py draws the
    tail's: activations of order 1 behind a LeakyReLU (the trunk's skip features behind a ReLU), weights of order 1 / sqrt(fan-in)"""
    cl, cs, co = triple
    g = torch.Generator().manual_seed(seed)
    lo = torch.nn.functional.leaky_relu(torch.randn(b, cl, h // 2, w // 2, generator=g), 0.1)
    skip = torch.relu(torch.randn(b, cs, h, w, generator=g))
    wt = torch.randn(co, cl + cs, 3, 3, generator=g) * (9 * (cl + cs)) ** -0.5
    bias = torch.randn(co, generator=g) * 0.2
    return lo, skip, (wt, bias)


INT_W, INT_X = 128, 4   # the largest |w| and |x| of the integer data
INT_BIAS = 1 << 20      # above every |sum|, so that no pre-activation is negative


def integers(b, h, w, triple, seed):
    """Exact integer data: every operand a small integer that bfloat16 holds exactly, every partial sum in any order an integer below
    2^24, so the kernel must give THE integers, whatever its order of summation.
      lo     per (image, channel) a constant plane from {0, +-1, +-2, +-4}: powers of two are what the float32 upsample reproduces
             exactly ((1 - l) v and l v are exact and fl((1 - l) + l) = 1), so In is integral
      skip   integers in -4 .. 4, different at every pixel
      w      seeded integers in -128 .. 128 (at most eight significant bits: exact in bfloat16), different at every (o, c, tap)
      bias   2^20 + a small integer: above every |sum| <= 1728 * 128 * 4 < 2^20, so no pre-activation is negative and the activation
             (whose 0.1f is not dyadic) leaves the integers alone; bias + |sum| < 2^21"""
    cl, cs, co = triple
    g = torch.Generator().manual_seed(seed)
    planes = torch.tensor([0., 1., -1., 2., -2., 4., -4.])
    lo = planes[torch.randint(0, 7, (b, cl, 1, 1), generator=g)].expand(b, cl, h // 2, w // 2).contiguous()
    skip = torch.randint(-INT_X, INT_X + 1, (b, cs, h, w), generator=g).float()
    wt = torch.randint(-INT_W, INT_W + 1, (co, cl + cs, 3, 3), generator=g).float()
    bias = (INT_BIAS + torch.randint(-50, 51, (co,), generator=g)).float()
    return lo, skip, (wt, bias)


def onehot(triple, seed):
    """(taps, w, bias): per output channel o one (c, ky, kx) = taps[o], w[o][c][ky][kx] = 1 and every other weight 0, bias 0.  Over the
    output channels every tap occurs (o runs through a seeded order of the nine, again and again) and both halves of In alternate:
    an upsampled channel for even o, a skip channel for odd o, seeded; among the upsampled ones the first and the last channel, and
    among skip's its first and last, are taken too (the chunk boundaries of the concatenation)."""
    cl, cs, co = triple
    g = torch.Generator().manual_seed(seed)
    order = torch.randperm(9, generator=g).tolist()
    fixed = {0: 0, 2: cl - 1, 1: cl, 3: cl + cs - 1}
    taps = []
    for o in range(co):
        c = fixed[o] if o in fixed else int(torch.randint(0, cl, (1,), generator=g)) if o % 2 == 0 else cl + int(torch.randint(0, cs, (1,), generator=g))
        t = order[o % 9]
        taps.append((c, t // 3, t % 3))
    assert {3 * ky + kx for _, ky, kx in taps} == set(range(9)) and {c < cl for c, _, _ in taps} == {True, False}
    wt = torch.zeros(co, cl + cs, 3, 3)
    for o, (c, ky, kx) in enumerate(taps):
        wt[o, c, ky, kx] = 1.0
    return taps, wt, torch.zeros(co)
