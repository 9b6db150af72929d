"""Inputs shared by tests/test_tail_cpu.py and tests/test_tail_device.py: seeded real data, the exact integer data, the identity
weights and the ramp of the known answer, and fixture G9 with the stand-in's features.  All on the CPU, float32 unless said."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 32, 48), (2, 40, 56), (3, 34, 66), (1, 2, 2), (1, 8, 130)]   # (b, h, w): the G9 size, a width that is no multiple of 32,
#                                             a width that crosses a 64-pixel tile by 2, hin = win = 1, thin and wider than two tiles
COUTS = [20, 1, 32, 18]


def seeded(b, h, w, cout, seed):
    """(fm [b,32,h/2,w/2], image [b,3,h,w], (w1, b1, w2, b2)) at the scales of a trained decoder: activations of order 1 behind a
    LeakyReLU, weights of order 1 / sqrt(fan-in)"""
    g = torch.Generator().manual_seed(seed)
    fm = torch.nn.functional.leaky_relu(torch.randn(b, 32, h // 2, w // 2, generator=g), 0.1)
    image = torch.randn(b, 3, h, w, generator=g)
    w1 = torch.randn(32, 35, 3, 3, generator=g) * 0.06
    b1 = torch.randn(32, generator=g) * 0.2
    w2 = torch.randn(cout, 32, generator=g) * 0.2
    b2 = torch.randn(cout, generator=g) * 0.1
    return fm, image, (w1, b1, w2, b2)


def integers(b, h, w, cout, seed, positive):
    """Exact integer data: every operand a small integer that bfloat16 holds exactly, every partial sum in any order an integer below
    2^24 (the tests assert it through A1 and A2), so both tiers must give THE integers, whatever their order of summation.
      fm     per (image, channel) a constant plane from {0, +-1, +-2, +-4}: powers of two are what the float32 upsample reproduces
             exactly ((1 - l) v and l v are exact and fl((1 - l) + l) = 1), so In is integral in the F32 tier too
      image  integers in -4 .. 4, different at every pixel
      w1     per raw channel its own permutation of 315 DISTINCT integers (-157 .. 157 without 0) over (column, tap): a swapped
             row / column map or a mis-ordered k changes almost every output
      w2     per output channel its own permutation of the 32 distinct integers -16 .. 16 without 0
      b1     `positive`: large enough that no pre-activation is negative, so the raw values stay integers for stage 2 (the
             activation's 0.1f is not dyadic); otherwise small, so that both branches of the activation occur in the raw output"""
    g = torch.Generator().manual_seed(seed)
    planes = torch.tensor([0., 1., -1., 2., -2., 4., -4.])
    fm = planes[torch.randint(0, 7, (b, 32, 1, 1), generator=g)].expand(b, 32, h // 2, w // 2).contiguous()
    image = torch.randint(-4, 5, (b, 3, h, w), generator=g).float()
    vals = torch.cat([torch.arange(-157, 0), torch.arange(1, 159)]).float()[:315]
    w1 = torch.stack([vals[torch.randperm(315, generator=g)] for _ in range(32)]).view(32, 35, 3, 3).contiguous()
    v2 = torch.cat([torch.arange(-16, 0), torch.arange(1, 17)]).float()
    w2 = torch.stack([v2[torch.randperm(32, generator=g)] for _ in range(cout)])
    b1 = torch.randint(-50, 51, (32,), generator=g).float() + (40000. if positive else 0.)
    b2 = torch.randint(-100, 101, (cout,), generator=g).float()
    return fm, image, (w1, b1, w2, b2)


def identity_weights(cout=20):
    """centre-tap identity: raw channel o is the activated upsampled channel o; the image and every other tap weigh 0"""
    w1 = torch.zeros(32, 35, 3, 3)
    w1[torch.arange(32), torch.arange(32), 1, 1] = 1.0
    return w1, torch.zeros(32), torch.zeros(cout, 32), torch.zeros(cout)


def ramp(b, hin, win):
    """fm[c] = p_c x + q_c y with non-negative dyadic slopes (exact in float32), the slopes, and the closed form of its upsampled value
    and magnitude at every output pixel in float64: p X (win - 1) / (w - 1) + q Y (hin - 1) / (h - 1)"""
    c = torch.arange(32)
    p, q = (c % 5).double() * 0.25, (c % 3).double() * 0.5
    x, y = torch.arange(win).double(), torch.arange(hin).double()
    fm = (p[:, None, None] * x[None, None, :] + q[:, None, None] * y[None, :, None]).float()[None].expand(b, 32, hin, win).contiguous()
    h, w = 2 * hin, 2 * win
    sx = torch.arange(w).double() * ((win - 1) / (w - 1) if w > 1 else 0.0)
    sy = torch.arange(h).double() * ((hin - 1) / (h - 1) if h > 1 else 0.0)
    closed = p[:, None, None] * sx[None, None, :] + q[:, None, None] * sy[None, :, None]
    return fm, closed[None].expand(b, 32, h, w).numpy()


FIXTURE = os.path.join(ROOT, "tests", "golden", "backbone_resnet18_8s.npz")


def standin():
    """the seeded stand-in of fixture G9 (tests/test_backbone_standin.py makes it the same way) and the fixture's input"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_amd
    torch.manual_seed(0)
    net = e2e_amd.StandInResnet18_8s(ver_dim=18, seg_dim=2).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    return net, torch.randn(1, 3, 32, 48)


def standin_features(net, x):
    """the stand-in's own modules up to conv2s"""
    with torch.no_grad():
        x2s = net.stem(x)
        x4s = net.l1(net.pool(x2s))
        x8s = net.l2(x4s)
        xfc = net.fc(net.l4(net.l3(x8s)))
        fm = net.up(net.conv8s(torch.cat([xfc, x8s], 1)))
        fm = net.up(net.conv4s(torch.cat([fm, x4s], 1)))
        return net.conv2s(torch.cat([fm, x2s], 1))


def g9():
    """(fm, x, params of the stand-in's tail, the fixture's seg and ver) of fixture G9, float32 on the CPU"""
    from pvnet_amd.tail import TailParams
    g = np.load(FIXTURE)
    net, x = standin()
    assert np.array_equal(x.numpy(), g["x"])
    P = TailParams.from_network(net)
    return standin_features(net, x), x, (P.w1, P.b1, P.w2, P.b2), g["seg"], g["ver"]
