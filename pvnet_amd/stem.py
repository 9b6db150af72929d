"""The network's stem on the device in one launch (include/pvnet_stem.h, libpvnet_stem.so): 7 x 7 stride-2 convolution with the eval()
BatchNorm folded in, ReLU, and the 3 x 3 stride-2 max-pool behind it -- ``conv1`` + ``bn1`` + ``relu`` + ``maxpool`` of the reference's
``ResNet.forward`` (lib/networks/resnet.py:138-142, 200-204).  Inference only: no autograd, ``eval()`` BatchNorm; training keeps the
PyTorch stem.

    params = StemParams.from_network(net)                # folds the BatchNorm in float64, once
    x2s, pooled = fused_stem(image, params)              # [b,64,Ho,Wo] (the decoder's skip input) and [b,64,Hp,Wp] (what layer1 takes)
    seg_pred, ver_pred = FusedStemNet(net)(image)        # pvnet_amd/net.py: FusedNet with the stem, the stages and the tail fused

There is one tier: operands rounded to bfloat16, float32 accumulation on the matrix pipe.  PyTorch is plumbing only.  There is NO CPU
fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import torch
from torch import nn

from ._abi import STEM_CIN, STEM_COUT, _check, load_stem_library
from ._marshal import ptr as _ptr, stream as _stream, strides as _strides
from ._net import (TYPE_CODES, NetworkParts, Params, check_conv_bn, check_input, fold_batchnorm, is_plain_conv, new_or_checked_out,
                   presets_in_net)

# whether FusedStemNet fuses the stem unless told otherwise: tools/stem_probe.py measured fused_stem faster than the eager stem and pool
# by more than the spread of the eager rounds (profiles/stem_probe.txt) -- the rule decoder.DEFAULT_STAGES was set by
DEFAULT_STEM = True


def out_sizes(h, w):
    """(Ho, Wo, Hp, Wp) of an h x w image: the header's integer divisions"""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return ho, wo, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1


class StemParams(Params):
    """The stem's weights as the library takes them: ``w [64,3,7,7]`` and ``bias [64]`` (the 7 x 7 convolution with the BatchNorm folded
    in), float32 and contiguous.  ``on(device)`` gives (and keeps) their copies on a device."""

    DEVICE = ("w", "bias")

    def __init__(self, w, bias):
        w, bias = self.float32(w, bias)
        if tuple(w.shape) != (STEM_COUT, STEM_CIN, 7, 7) or tuple(bias.shape) != (STEM_COUT,):
            raise ValueError(f"StemParams: w must be [64,3,7,7] and bias [64] (got {tuple(w.shape)}, {tuple(bias.shape)}): "
                             "widths other than the ResNet stem's are not supported")
        self.w, self.bias = w, bias

    @classmethod
    def from_modules(cls, conv, bn, act=None, pool=None):
        """Folds the ``eval()`` BatchNorm into the convolution in float64, with ``_net.fold_batchnorm``: ``s = gamma /
        sqrt(var + eps)``, ``w = W * s``, ``bias = beta - mean * s``, each rounded once to float32.  Refuses what the fused stem does not
        compute: a BatchNorm in training mode or without running statistics, a convolution that is not ``Conv2d(3, 64, 7, 2, 3,
        bias=False)``, an activation (``act``, where given) that is not ``ReLU``, a pool (where given) that is not ``MaxPool2d(3, 2, 1)``
        with dilation 1 and ``ceil_mode=False``."""
        check_conv_bn("StemParams", conv, bn)
        if act is not None and not isinstance(act, nn.ReLU):
            raise ValueError(f"StemParams: the activation must be ReLU (got {act})")
        if pool is not None:
            def pair(v):
                return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
            if not isinstance(pool, nn.MaxPool2d) or (pair(pool.kernel_size), pair(pool.stride), pair(pool.padding), pair(pool.dilation),
                                                      bool(pool.ceil_mode)) != ((3, 3), (2, 2), (1, 1), (1, 1), False):
                raise ValueError(f"StemParams: the pool must be MaxPool2d(3, 2, 1) with dilation 1 and ceil_mode=False (got {pool})")
        if (conv.in_channels, conv.out_channels) != (STEM_CIN, STEM_COUT):
            raise ValueError("StemParams: widths other than 3 -> 64 are not supported (the ResNet stem's only)")
        if not is_plain_conv(conv, 7, 2, 3, 1):
            raise ValueError("StemParams: expected Conv2d(3, 64, 7, 2, 3, bias=False)")
        return cls(*fold_batchnorm(conv, bn))

    @classmethod
    def from_network(cls, net):
        """From a network with the reference's ``resnet18_8s.{conv1,bn1,relu,maxpool}`` (its ``Resnet18_8s``) or the ``stem`` (a
        ``Sequential`` of conv, bn, act) and ``pool`` of the stand-in of tools/e2e_amd.py."""
        parts = NetworkParts(net, "StemParams")
        conv, bn, act = parts.stem_triple
        return cls.from_modules(conv, bn, act=act, pool=parts.pool)


def fused_stem(image, params, *, out=None, out_dtype=None, pool=True):
    """The stem for a batch, on the current stream, without synchronising: one launch, no workspace.  Returns ``(x2s, pooled)``.

    :param image:     [b,3,h,w] float32 / float16 / bfloat16 CUDA tensor, any strides (channels-last is one)
    :param params:    ``StemParams``
    :param out:       None or the tensors to write into and return: ``(x2s, pooled)``, contiguous ``[b,64,Ho,Wo]`` and ``[b,64,Hp,Wp]``
                      of one type; with ``pool=False`` ``x2s`` alone, or ``(x2s, None)``
    :param out_dtype: the type of new outputs: float32 / float16 / bfloat16; default ``image``'s
    :param pool:      False: only ``x2s`` is written (the same bits) and ``pooled`` is None
    """
    if not isinstance(params, StemParams):
        raise RuntimeError("params must be a StemParams")
    check_input("image", image, STEM_CIN)
    dev = image.device
    b, _, h, w = (int(v) for v in image.shape)
    if b < 1 or h < 1 or w < 1:
        raise RuntimeError("image must not be empty")
    ho, wo, hp, wp = out_sizes(h, w)
    shapes = ((b, STEM_COUT, ho, wo), (b, STEM_COUT, hp, wp))
    x2s = pooled = None
    if out is not None:
        x2s, pooled = (out, None) if isinstance(out, torch.Tensor) else tuple(out) if len(out) == 2 else (None, None)
        if x2s is None or (pooled is not None) != bool(pool):
            raise RuntimeError("out must be (x2s, pooled) with the pool and x2s or (x2s, None) without it")
    x2s = new_or_checked_out(x2s, out_dtype, image.dtype, shapes[0], dev, "out: x2s")
    pooled = new_or_checked_out(pooled, x2s.dtype, None, shapes[1], dev, "out: pooled") if pool else None
    w32, bias = params.on(dev)
    lib = load_stem_library()
    with torch.cuda.device(dev):
        _check(lib.pvnet_stem_forward(_ptr(image), TYPE_CODES[image.dtype], _strides(image, 4), _ptr(w32), _ptr(bias), b, h, w,
                                      _ptr(x2s), _ptr(pooled) if pool else None, TYPE_CODES[x2s.dtype], _stream(dev)), "pvnet_stem_forward")
    return x2s, pooled


__getattr__ = presets_in_net(__name__, "FusedStemNet")   # the network class: pvnet_amd/net.py, which imports this module
