"""The network's tail on the device in one launch (include/pvnet_tail.h, libpvnet_tail.so): bilinear 2x upsample of the last decoder
stage, concatenation with the image, 3 x 3 convolution with the eval() BatchNorm folded in, LeakyReLU(0.1) and the 1 x 1 convolution
to the seg / vertex channels -- ``up2storaw`` + ``cat`` + ``convraw`` of the reference's ``Resnet18_8s.forward``
(lib/networks/model_repository.py:51-58, 74-78).  Inference only: no autograd, ``eval()`` BatchNorm; training keeps the PyTorch tail.

    params = TailParams.from_network(net)              # folds the BatchNorm in float64, once
    out = fused_tail(fm, image, params)                # [b,cout,h,w]; fm [b,32,h/2,w/2] is the output of conv2s, image [b,3,h,w]
    seg_pred, ver_pred = FusedTailNet(net)(image)      # pvnet_amd/net.py: FusedNet with only this piece fused

``seg_pred`` / ``ver_pred`` are views of one tensor; ``voting.EvalWrapper`` / ``PoseEvalWrapper`` and the ``_from_logits`` entries take
them as they are.  PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise
``RuntimeError``.
"""
from __future__ import annotations

import torch
from torch import nn

from ._abi import TAIL_BF16, TAIL_F32, TAIL_F_RAW, TAIL_MAX_COUT, TAIL_WIDTH, _check, load_tail_library
from ._marshal import ptr as _ptr, stream as _stream, strides as _strides
from ._net import (SLOPE, TYPE_CODES, Params, check_conv_bn, check_input, fold_batchnorm, is_leaky, is_plain_conv, new_or_checked_out,
                   presets_in_net)

_PRECISIONS = {"bf16": TAIL_BF16, "f32": TAIL_F32}


class TailParams(Params):
    """The tail's weights as the library takes them, float32 and contiguous: ``w1 [32,35,3,3]`` and ``b1 [32]`` (the 3 x 3 convolution
    with the BatchNorm folded in), ``w2 [cout,32]`` and ``b2 [cout]`` (the 1 x 1 convolution).  ``on(device)`` gives (and keeps) their
    copies on a device."""
    DEVICE = ("w1", "b1", "w2", "b2")

    def __init__(self, w1, b1, w2, b2):
        w1, b1, w2, b2 = self.float32(w1, b1, w2, b2)
        cout = int(w2.shape[0]) if w2.dim() == 2 else -1
        if tuple(w1.shape) != (TAIL_WIDTH, TAIL_WIDTH + 3, 3, 3) or tuple(b1.shape) != (TAIL_WIDTH,):
            raise ValueError(f"TailParams: w1 must be [32,35,3,3] and b1 [32] (got {tuple(w1.shape)}, {tuple(b1.shape)}): the ResNet-18 widths only")
        if not 1 <= cout <= TAIL_MAX_COUT or tuple(w2.shape) != (cout, TAIL_WIDTH) or tuple(b2.shape) != (cout,):
            raise ValueError(f"TailParams: w2 must be [cout,32] and b2 [cout] with 1 <= cout <= 32 (got {tuple(w2.shape)}, {tuple(b2.shape)})")
        self.w1, self.b1, self.w2, self.b2 = w1, b1, w2, b2
        self.cout = cout

    @classmethod
    def from_modules(cls, conv3x3, bn, conv1x1, act=None):
        """Folds the ``eval()`` BatchNorm into the 3 x 3 convolution in float64: ``s = gamma / sqrt(var + eps)``, ``w1 = W * s``,
        ``b1 = beta - mean * s``, each rounded once to float32.  Refuses what the fused tail does not compute: a BatchNorm in training
        mode or without running statistics, a LeakyReLU slope other than 0.1 (``act``, where given), a 3 x 3 convolution with a bias or
        a 1 x 1 convolution without one, widths other than 32, strides, dilations, groups."""
        if not isinstance(conv1x1, nn.Conv2d):
            raise ValueError("TailParams: expected Conv2d, BatchNorm2d, Conv2d")
        check_conv_bn("TailParams", conv3x3, bn)
        if act is not None and not is_leaky(act):
            raise ValueError(f"TailParams: the activation must be LeakyReLU({SLOPE}) (got {act})")
        if conv1x1.bias is None:
            raise ValueError("TailParams: the reference's 1 x 1 convolution has a bias")
        if (conv3x3.in_channels, conv3x3.out_channels, conv1x1.in_channels) != (TAIL_WIDTH + 3, TAIL_WIDTH, TAIL_WIDTH):
            raise ValueError("TailParams: widths other than 35 -> 32 -> cout are not supported (the ResNet-18 network's shapes only)")
        if not 1 <= conv1x1.out_channels <= TAIL_MAX_COUT:
            raise ValueError("TailParams: 1 <= cout <= 32")
        if not (is_plain_conv(conv3x3, 3, 1, 1, 1) and is_plain_conv(conv1x1, 1, 1, 0, 1)):
            raise ValueError("TailParams: expected Conv2d(35, 32, 3, 1, 1) and Conv2d(32, cout, 1, 1)")
        return cls(*fold_batchnorm(conv3x3, bn), conv1x1.weight.detach().reshape(conv1x1.out_channels, TAIL_WIDTH).float().cpu(),
                   conv1x1.bias.detach().float().cpu())

    @classmethod
    def from_network(cls, net):
        """From a network with the reference's ``convraw``: its ``Resnet18_8s`` (a flat ``Sequential`` of conv, bn, act, conv) or the
        stand-in of tools/e2e_amd.py (``Sequential(Sequential(conv, bn, act), conv)``)."""
        convraw = getattr(net, "convraw", None)
        if not isinstance(convraw, nn.Sequential):
            raise ValueError("TailParams: the network has no `convraw` Sequential")
        mods = list(convraw)
        if len(mods) == 2 and isinstance(mods[0], nn.Sequential):
            mods = list(mods[0]) + mods[1:]
        if len(mods) != 4:
            raise ValueError("TailParams: `convraw` must be conv, bn, act, conv (flat, or the first three nested)")
        return cls.from_modules(mods[0], mods[1], mods[3], act=mods[2])


def fused_tail(fm, image, params, *, precision="bf16", out=None, out_dtype=None, raw=False):
    """The tail for a batch, on the current stream, without synchronising: one launch, no workspace.

    :param fm:        [b,32,hin,win] float32 / float16 / bfloat16 CUDA tensor, any strides: the output of ``conv2s``
    :param image:     [b,3,2 hin,2 win] of the same three types (its own), any strides, on the same device
    :param params:    ``TailParams``
    :param precision: ``"bf16"`` -- operands rounded to bfloat16, float32 accumulation on the matrix pipe (the hot path) -- or ``"f32"``
    :param out:       None or the tensor to write into and return: contiguous ``[b,cout,h,w]`` (with ``raw``: ``[b,32,h,w]`` float32)
    :param out_dtype: the type of a new ``out``: float32 / float16 / bfloat16; default ``fm``'s (with ``raw`` always float32)
    :param raw:       return the 32 channels behind the LeakyReLU, float32, before any rounding; the 1 x 1 convolution is skipped
    """
    if not isinstance(params, TailParams):
        raise RuntimeError("params must be a TailParams")
    if precision not in _PRECISIONS:
        raise RuntimeError('precision must be "bf16" or "f32"')
    check_input("fm", fm, TAIL_WIDTH)
    check_input("image", image, 3)
    dev = fm.device
    b, _, hin, win = (int(v) for v in fm.shape)
    h, w = 2 * hin, 2 * win
    if image.device != dev or tuple(image.shape) != (b, 3, h, w):
        raise RuntimeError(f"image must be [b,3,2 hin,2 win] = {(b, 3, h, w)} on {dev} (got {tuple(image.shape)} on {image.device})")
    if b < 1 or hin < 1 or win < 1:
        raise RuntimeError("fm must not be empty")
    shape = (b, TAIL_WIDTH if raw else params.cout, h, w)
    out = new_or_checked_out(out, torch.float32 if raw else out_dtype, fm.dtype, shape, dev)
    w1, b1, w2, b2 = params.on(dev)
    lib = load_tail_library()
    with torch.cuda.device(dev):
        _check(lib.pvnet_tail_forward(
            _ptr(fm), TYPE_CODES[fm.dtype], _strides(fm, 4), _ptr(image), TYPE_CODES[image.dtype], _strides(image, 4),
            _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), b, hin, win, h, w, TAIL_WIDTH, TAIL_WIDTH, params.cout, _PRECISIONS[precision],
            TAIL_F_RAW if raw else 0, _ptr(out), TYPE_CODES[out.dtype], _stream(dev)), "pvnet_tail_forward")
    return out


__getattr__ = presets_in_net(__name__, "FusedTailNet")   # the network class: pvnet_amd/net.py, which imports this module
