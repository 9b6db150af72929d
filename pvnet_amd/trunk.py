"""The residual trunk's 3 x 3 convolutions on the device, one launch each (include/pvnet_trunk.h, libpvnet_trunk.so): the convolution
over one or two concatenated inputs with the eval() BatchNorm folded in, and the residual addition and the activation applied to its
own accumulators -- ``conv1`` + ``bn1`` + ``relu`` and ``conv2`` + ``bn2`` + add + ``relu`` of the reference's ``BasicBlock.forward``
(lib/networks/resnet.py:54-70), and ``fc`` and ``cat`` + ``conv8s`` of its ``Resnet18_8s`` (lib/networks/model_repository.py:17-33, 67).
Inference only: no autograd, ``eval()`` BatchNorm; training keeps the PyTorch trunk.

    params = ConvParams.from_modules(conv, bn, act)           # folds the BatchNorm in float64 and packs the weights, once
    y = fused_conv3x3(x, params, residual=r)                  # [b,co,ho,wo]; src2= concatenates a second input behind the first
    y = FusedBasicBlock(block)(x)                             # two launches; a 1 x 1 downsample is one F.conv2d with its BatchNorm folded
    seg_pred, ver_pred = FusedTrunkNet(net, layers=LAYERS)(image)   # pvnet_amd/net.py: FusedNet under its first name

There is one tier: operands rounded to bfloat16, float32 accumulation on the matrix pipe.  PyTorch is plumbing only.  There is NO CPU
fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ._abi import TRUNK_ACT_LEAKY, TRUNK_ACT_NONE, TRUNK_ACT_RELU, TRUNK_GEOMETRIES, TRUNK_MAX_WIDTH, _check, load_trunk_library
from ._marshal import ptr as _ptr, stream as _stream, strides as _strides
from ._net import (SLOPE, TYPE_CODES, NetworkParts, Params, check_conv_bn, check_input, fold_batchnorm, is_leaky, is_plain_conv,
                   new_or_checked_out, pack_weights, presets_in_net)

ACTS = {"none": TRUNK_ACT_NONE, "relu": TRUNK_ACT_RELU, "leaky": TRUNK_ACT_LEAKY}
LAYERS = ("layer1", "layer2", "layer3", "layer4", "fc", "conv8s")   # the reference's attribute names, in the order the network runs them
# the pieces FusedTrunkNet fuses unless told otherwise: those that tools/trunk_probe.py measured faster than the eager piece by more than
# the spread of the eager piece's rounds (profiles/trunk_probe.txt); every other piece stays reachable by naming it
DEFAULT_LAYERS = ("layer3", "fc", "conv8s")


def out_sizes(h, w, stride):
    """(ho, wo) of an h x w input: the header's integer divisions"""
    return (h - 1) // stride + 1, (w - 1) // stride + 1


class ConvParams(Params):
    """A convolution's weights as the library takes them: ``w [co,cin,3,3]`` and ``bias [co]`` (the 3 x 3 convolution with the
    BatchNorm folded in), float32 and contiguous, ``packed``, the same weights rounded to bfloat16 in the kernel's fragment order, and
    its ``stride``, ``dilation`` (one of (1,1), (2,1), (1,2), (1,4); the padding is the dilation) and ``act`` ("none", "relu" or
    "leaky").  ``on(device)`` gives (and keeps) the device's copies of ``bias`` and ``packed``."""

    DEVICE = ("bias", "packed")

    def __init__(self, w, bias, stride=1, dilation=1, act="none"):
        w, bias = self.float32(w, bias)
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or tuple(bias.shape) != (int(w.shape[0]),):
            raise ValueError(f"ConvParams: w must be [co,cin,3,3] and bias [co] (got {tuple(w.shape)}, {tuple(bias.shape)})")
        co, cin = int(w.shape[0]), int(w.shape[1])
        if co % 32 or cin % 32 or not 0 < co <= TRUNK_MAX_WIDTH or not 0 < cin <= TRUNK_MAX_WIDTH:
            raise ValueError(f"ConvParams: widths must be multiples of 32 up to {TRUNK_MAX_WIDTH} (got {cin} -> {co}): the ResNet-18 "
                             "trunk's shapes only")
        if (int(stride), int(dilation)) not in TRUNK_GEOMETRIES:
            raise ValueError(f"ConvParams: (stride, dilation) must be one of {TRUNK_GEOMETRIES} (got {(stride, dilation)})")
        if act not in ACTS:
            raise ValueError(f"ConvParams: act must be one of {tuple(ACTS)} (got {act!r})")
        self.w, self.bias = w, bias
        self.cin, self.co, self.stride, self.dilation, self.act = cin, co, int(stride), int(dilation), act
        self.packed = pack_weights(w)

    @classmethod
    def from_modules(cls, conv, bn, act=None):
        """Folds the ``eval()`` BatchNorm into the convolution in float64, with ``_net.fold_batchnorm``.  Refuses what
        the fused convolution does not compute: a BatchNorm in training mode or without running statistics, a convolution with a bias,
        a kernel other than 3 x 3, a padding that is not the dilation, groups, an activation (``act``: None, a module or one of
        "none", "relu", "leaky") other than ReLU and LeakyReLU(0.1), widths, strides and dilations outside the library's."""
        check_conv_bn("ConvParams", conv, bn)
        if isinstance(act, nn.ReLU):
            act = "relu"
        elif isinstance(act, nn.LeakyReLU):
            if not is_leaky(act):
                raise ValueError(f"ConvParams: the LeakyReLU slope must be {SLOPE} (got {act})")
            act = "leaky"
        elif act is None:
            act = "none"
        elif act not in ACTS:
            raise ValueError(f"ConvParams: the activation must be ReLU, LeakyReLU({SLOPE}) or none (got {act})")
        if tuple(conv.kernel_size) != (3, 3) or conv.groups != 1 or conv.padding_mode != "zeros":
            raise ValueError("ConvParams: expected Conv2d(cin, cout, 3, stride, d, d, groups=1, bias=False) with zero padding")
        if conv.stride[0] != conv.stride[1] or conv.dilation[0] != conv.dilation[1] or tuple(conv.padding) != tuple(conv.dilation):
            raise ValueError(f"ConvParams: the padding must be the dilation, both square (got stride {conv.stride}, padding "
                             f"{conv.padding}, dilation {conv.dilation})")
        return cls(*fold_batchnorm(conv, bn), stride=conv.stride[0], dilation=conv.dilation[0], act=act)


def fused_conv3x3(src1, params, *, src2=None, residual=None, out=None, out_dtype=None):
    """A 3 x 3 convolution of the trunk for a batch, on the current stream, without synchronising: one launch, no workspace.

    :param src1:      [b,c1,h,w] float32 / float16 / bfloat16 CUDA tensor, any strides
    :param params:    ``ConvParams``; its stride, dilation and activation are the launch's
    :param src2:      None or [b,c2,h,w] of the same three types (its own), any strides: the convolution reads ``cat([src1, src2], 1)``;
                      c1 + c2 is the parameters' ``cin``, each a multiple of 32
    :param residual:  None or [b,co,ho,wo] of the same three types, any strides: added in float32 before the activation
    :param out:       None or the tensor to write into and return: contiguous ``[b,co,ho,wo]``
    :param out_dtype: the type of a new ``out``: float32 / float16 / bfloat16; default ``src1``'s
    """
    if not isinstance(params, ConvParams):
        raise RuntimeError("params must be a ConvParams")
    for name, t in (("src1", src1), ("src2", src2), ("residual", residual)):
        if t is not None or name == "src1":
            check_input(name, t)
    dev = src1.device
    b, c1, h, w = (int(v) for v in src1.shape)
    c2 = 0 if src2 is None else int(src2.shape[1])
    if b < 1 or h < 1 or w < 1:
        raise RuntimeError("src1 must not be empty")
    if c1 % 32 or c2 % 32 or c1 < 1 or (src2 is not None and c2 < 1) or c1 + c2 != params.cin:
        raise RuntimeError(f"src1 and src2 must have multiples of 32 channels that add up to {params.cin} (got {c1} + {c2})")
    if src2 is not None and (src2.device != dev or tuple(src2.shape) != (b, c2, h, w)):
        raise RuntimeError(f"src2 must be {(b, c2, h, w)} on {dev} (got {tuple(src2.shape)} on {src2.device})")
    ho, wo = out_sizes(h, w, params.stride)
    shape = (b, params.co, ho, wo)
    if residual is not None and (residual.device != dev or tuple(residual.shape) != shape):
        raise RuntimeError(f"residual must be {shape} on {dev} (got {tuple(residual.shape)} on {residual.device})")
    out = new_or_checked_out(out, out_dtype, src1.dtype, shape, dev)
    bias, wpk = params.on(dev)
    lib = load_trunk_library()

    def triple(t):
        return (None, 0, None) if t is None else (_ptr(t), TYPE_CODES[t.dtype], _strides(t, 4))

    with torch.cuda.device(dev):
        _check(lib.pvnet_conv3x3_fused(*triple(src1), *triple(src2), *triple(residual), _ptr(wpk), _ptr(bias), b, h, w, c1, c2,
                                       params.co, params.stride, params.dilation, ACTS[params.act], _ptr(out), TYPE_CODES[out.dtype],
                                       _stream(dev)), "pvnet_conv3x3_fused")
    return out


class FusedBasicBlock(nn.Module):
    """A ``BasicBlock`` for inference in two launches: conv1 + bn1 + ReLU, then conv2 + bn2 + residual + ReLU.  The residual is the
    input, or, for a block with a 1 x 1 ``downsample`` (Conv2d, BatchNorm2d), one ``F.conv2d`` under PyTorch with the downsample's
    BatchNorm folded into its weight and bias (in float64, as ``ConvParams`` folds) -- one call where eager makes two."""

    def __init__(self, block):
        super().__init__()
        conv1, bn1, conv2, bn2, down = NetworkParts.basic_block(block)
        self.conv1 = ConvParams.from_modules(conv1, bn1, "relu")
        self.conv2 = ConvParams.from_modules(conv2, bn2, "relu")
        if (self.conv2.stride, self.conv2.cin) != (1, self.conv1.co):
            raise ValueError("FusedBasicBlock: conv2 must have stride 1 and conv1's width")
        self.down = None
        if down is not None:
            if not (isinstance(down, nn.Sequential) and len(down) == 2):
                raise ValueError("FusedBasicBlock: the downsample must be a Sequential of Conv2d, BatchNorm2d")
            check_conv_bn("FusedBasicBlock: downsample", down[0], down[1])
            if not is_plain_conv(down[0], 1, self.conv1.stride, 0, 1):
                raise ValueError("FusedBasicBlock: the downsample must be Conv2d(cin, cout, 1, stride) with conv1's stride")
            self.down = fold_batchnorm(down[0], down[1])
        elif self.conv1.stride != 1 or self.conv1.cin != self.conv2.co:
            raise ValueError("FusedBasicBlock: a block that changes its shape needs a downsample")
        self._down_on = {}

    def residual(self, x):
        """what conv2's launch adds: ``x``, or the folded downsample of it (in ``x``'s type)"""
        if self.down is None:
            return x
        key = (x.device, x.dtype)
        if key not in self._down_on:
            self._down_on[key] = tuple(t.to(device=x.device, dtype=x.dtype) for t in self.down)
        w, bias = self._down_on[key]
        return F.conv2d(x, w, bias, stride=self.conv1.stride)

    @torch.no_grad()
    def forward(self, x):
        y = fused_conv3x3(x, self.conv1)
        return fused_conv3x3(y, self.conv2, residual=self.residual(x))


__getattr__ = presets_in_net(__name__, "FusedTrunkNet")   # the network class: pvnet_amd/net.py, which imports this module
