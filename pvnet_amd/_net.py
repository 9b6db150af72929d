"""What the wrappers of the four fused network libraries share (tail.py, decoder.py, stem.py, trunk.py): the type codes, the BatchNorm
fold and its checks, the packed weight image, the parameter classes' base, the checks of inputs and outputs, and ``NetworkParts``, the
one place that knows the two spellings of the wrapped network.  Private: the public names stay in the four modules."""
from __future__ import annotations

import torch
from torch import nn

from ._abi import TAIL_T_BF16, TAIL_T_F16, TAIL_T_F32

TYPE_CODES = {torch.float32: TAIL_T_F32, torch.float16: TAIL_T_F16, torch.bfloat16: TAIL_T_BF16}   # (_abi: the four families are equal)
SLOPE = 0.1   # the LeakyReLU of the reference's decoder stages


def check_conv_bn(who, conv, bn):
    """refuses what no fold serves: a BatchNorm in training mode or without running statistics, a convolution with a bias"""
    if not (isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d)):
        raise ValueError(f"{who}: expected Conv2d, BatchNorm2d")
    if bn.training or bn.running_mean is None or bn.running_var is None:
        raise ValueError(f"{who}: the BatchNorm must be in eval() mode with running statistics (inference only)")
    if conv.bias is not None:
        raise ValueError(f"{who}: the reference's convolutions have no bias")
    if bn.num_features != conv.out_channels:
        raise ValueError(f"{who}: the BatchNorm's width is not the convolution's")


def fold_batchnorm(conv, bn):
    """the eval() BatchNorm folded into a bias-free convolution in float64: ``s = gamma / sqrt(var + eps)``, ``w = W * s``, ``bias =
    beta - mean * s``, each rounded once to float32; on the CPU"""
    with torch.no_grad():
        var, mean = bn.running_var.double(), bn.running_mean.double()
        gamma = bn.weight.double() if bn.weight is not None else torch.ones_like(var)
        beta = bn.bias.double() if bn.bias is not None else torch.zeros_like(var)
        s = gamma / torch.sqrt(var + bn.eps)
        return (conv.weight.double() * s[:, None, None, None]).float().cpu(), (beta - mean * s).float().cpu()


def is_plain_conv(conv, kernel, stride, padding, dilation):
    """whether ``conv`` is ``Conv2d(cin, cout, kernel, stride, padding, dilation)``, square, ungrouped and zero-padded"""
    got = (tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation), conv.groups)
    return got == ((kernel,) * 2, (stride,) * 2, (padding,) * 2, (dilation,) * 2, 1) and (padding == 0 or conv.padding_mode == "zeros")


def is_leaky(act):
    return isinstance(act, nn.LeakyReLU) and float(act.negative_slope) == SLOPE


def pack_weights(w):
    """``w [co,cin,3,3]`` float32 -> the bfloat16 image the decoder's (PVNET_DECODER_F_PACKED) and the trunk's library take,
    ``[cin/32, 9, 2, co/32, 64, 8]``: element (chunk, tap, half, m, lane, j) is
    ``bf16(w[32 m + (lane & 31)][32 chunk + 16 half + 8 (lane >> 5) + j][tap / 3][tap % 3])``, the rounding torch's round-to-nearest-even"""
    co, cin = int(w.shape[0]), int(w.shape[1])
    v = w.to(torch.bfloat16).reshape(co // 32, 32, cin // 32, 2, 2, 8, 9)   # m, r, chunk, half, hh, j, tap
    return v.permute(2, 6, 3, 0, 4, 1, 5).contiguous().reshape(cin // 32, 9, 2, co // 32, 64, 8)


class Params:
    """The base of the four parameter classes: ``DEVICE`` names the tensors ``on(device)`` gives (and keeps) the device's copies of."""
    DEVICE = ()

    @staticmethod
    def float32(*tensors):
        return tuple(torch.as_tensor(t).detach().to(torch.float32).contiguous() for t in tensors)

    def on(self, device):
        device, kept = torch.device(device), self.__dict__.setdefault("_on", {})
        if device not in kept:
            kept[device] = tuple(getattr(self, n).to(device) for n in self.DEVICE)
        return kept[device]


def check_input(name, t, channels=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.dtype in TYPE_CODES):
        raise RuntimeError(f"{name} must be a 4-D float32, float16 or bfloat16 CUDA tensor")
    if channels is not None and t.shape[1] != channels:
        raise RuntimeError(f"{name} must have {channels} channels (got {t.shape[1]})")


def new_or_checked_out(out, out_dtype, default_dtype, shape, dev, name="out"):
    """a new contiguous tensor of ``out_dtype`` (default ``default_dtype``), or ``out`` where it is one of that shape on that device
    and of ``out_dtype`` (default: its own)"""
    if out is None:
        dtype = out_dtype if out_dtype is not None else default_dtype
        if dtype not in TYPE_CODES:
            raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
        return torch.empty(shape, dtype=dtype, device=dev)
    want = out_dtype if out_dtype is not None else out.dtype if isinstance(out, torch.Tensor) else None
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == want and out.dtype in TYPE_CODES and
            tuple(out.shape) == shape and out.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous {want} CUDA tensor of shape {shape} on {dev}")
    return out


def presets_in_net(module, *names):
    """a module's ``__getattr__`` that resolves ``names`` in pvnet_amd/net.py on first use: net.py imports the four modules, so they
    cannot import it while they load"""
    def __getattr__(name):
        if name in names:
            from . import net
            return getattr(net, name)
        raise AttributeError(f"module {module!r} has no attribute {name!r}")
    return __getattr__


def conv_bn_act(net, name, who):
    """the ``Sequential`` of conv, bn, act that ``net`` has under ``name`` (the same in both spellings)"""
    seq = getattr(net, name, None)
    if not isinstance(seq, nn.Sequential) or len(seq) != 3:
        raise ValueError(f"{who}: the network has no `{name}` Sequential of conv, bn, act")
    return tuple(seq)


class NetworkParts:
    """The pieces of a wrapped ``Resnet18_8s`` under one set of names, whichever spelling it has -- the reference's (``resnet18_8s``
    with ``conv1, bn1, relu, maxpool, layer1 .. layer4, fc``; ``up8sto4s, up4sto2s, up2storaw``) or the stand-in's of tools/e2e_amd.py
    (``stem, pool, l1 .. l4, fc``; one ``up``):

    ``stem_triple`` (conv, bn, act), ``pool``, ``layers`` (four), ``fc``; and, None where the network lacks them, ``conv8s``, ``ups``
    (the upsample before conv4s, before conv2s and before convraw), ``stages`` (conv4s, conv2s) and ``convraw``, which both spell alike."""

    def __init__(self, net, who="NetworkParts"):
        self.whole = getattr(net, "resnet18_8s", None)   # the reference's trunk, which its network calls whole and FusedNet piecewise
        try:
            if self.whole is not None:
                t = self.whole
                self.stem_triple, self.pool, self.fc = (t.conv1, t.bn1, t.relu), t.maxpool, t.fc
                self.layers = (t.layer1, t.layer2, t.layer3, t.layer4)
                ups = ("up8sto4s", "up4sto2s", "up2storaw")
            else:
                self.stem_triple, self.pool, self.fc = tuple(net.stem), net.pool, net.fc
                self.layers = (net.l1, net.l2, net.l3, net.l4)
                ups = ("up",) * 3
            if len(self.stem_triple) != 3:
                raise TypeError
        except (AttributeError, TypeError):
            raise ValueError(f"{who}: neither the reference's `resnet18_8s` with `conv1, bn1, relu, maxpool, layer1 .. layer4, fc` nor "
                             "the stand-in's `stem` Sequential of conv, bn, act with `pool, l1 .. l4, fc`") from None
        self.ups = tuple(getattr(net, n, None) for n in ups)
        self.conv8s, self.convraw = getattr(net, "conv8s", None), getattr(net, "convraw", None)
        self.stages = (getattr(net, "conv4s", None), getattr(net, "conv2s", None))

    def require_fully_conv(self, who):
        """the reference's trunk, run piecewise, is its fully convolutional forward only"""
        if self.whole is not None and not (getattr(self.whole, "fully_conv", False) and getattr(self.whole, "remove_avg_pool_layer", False)):
            raise ValueError(f"{who}: the reference's trunk must be built with fully_conv=True, remove_avg_pool_layer=True")

    @staticmethod
    def basic_block(block):
        """(conv1, bn1, conv2, bn2, downsample) of the reference's ``BasicBlock`` or of the stand-in's ``B`` (tools/e2e_amd.py)"""
        for names in (("conv1", "bn1", "conv2", "bn2", "downsample"), ("c1", "b1", "c2", "b2", "down")):
            if all(hasattr(block, n) for n in names) and not hasattr(block, "conv3"):   # (conv3: the Bottleneck, which is not supported)
                return tuple(getattr(block, n) for n in names)
        raise ValueError("FusedBasicBlock: neither the reference's BasicBlock (conv1, bn1, conv2, bn2, downsample) nor the stand-in's "
                         "(c1, b1, c2, b2, down)")

    def stem_modules(self, x):
        conv, bn, act = self.stem_triple
        return act(bn(conv(x)))

    def eager_stem(self, x):
        x2s = self.stem_modules(x)
        return x2s, self.pool(x2s)

    def eager_conv8s(self, xfc, x8s):
        return self.conv8s(torch.cat([xfc, x8s], 1))

    def eager_stage(self, k, fm, skip):
        """stage k (0: conv4s, 1: conv2s) by the wrapped modules: the upsample in front of it, the concatenation, the stage"""
        return self.stages[k](torch.cat([self.ups[k](fm), skip], 1))
