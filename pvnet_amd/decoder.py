"""The decoder stages on the device, one launch each (include/pvnet_decoder.h, libpvnet_decoder.so): bilinear 2x upsample of the previous
stage, concatenation with the trunk's skip features, 3 x 3 convolution with the eval() BatchNorm folded in and LeakyReLU(0.1) --
``up8sto4s`` + ``cat`` + ``conv4s`` and ``up4sto2s`` + ``cat`` + ``conv2s`` of the reference's ``Resnet18_8s.forward``
(lib/networks/model_repository.py:29-50, 67-73).  Inference only: no autograd, ``eval()`` BatchNorm; training keeps the PyTorch stages.

    params = StageParams.from_network(net, "conv2s")     # folds the BatchNorm in float64 and packs the weights, once
    fm = fused_stage(lo, skip, params)                   # [b,co,h,w]; lo [b,cl,h/2,w/2] the previous stage, skip [b,64,h,w]
    seg_pred, ver_pred = FusedDecoderNet(net)(image)     # pvnet_amd/net.py: FusedNet with these stages and the tail fused

There is one tier: operands rounded to bfloat16, float32 accumulation on the matrix pipe.  PyTorch is plumbing only.  There is NO CPU
fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import torch

from ._abi import DECODER_F_PACKED, DECODER_SHAPES, DECODER_SKIP, _check, load_decoder_library
from ._marshal import ptr as _ptr, stream as _stream, strides as _strides
from ._net import (SLOPE, TYPE_CODES, Params, check_conv_bn, check_input, conv_bn_act, fold_batchnorm, is_leaky, is_plain_conv,
                   new_or_checked_out, pack_weights, presets_in_net)

STAGES = ("conv4s", "conv2s")   # the reference's attribute names, in the order the network runs them
# the stages FusedDecoderNet fuses unless told otherwise: those that tools/decoder_probe.py measured faster than the eager stage by more
# than the spread of the eager stage's rounds (profiles/decoder_probe.txt); the other kernel stays reachable by naming its stage
DEFAULT_STAGES = ("conv4s", "conv2s")


class StageParams(Params):
    """A stage's weights as the library takes them: ``w [co,cl+64,3,3]`` and ``bias [co]`` (the 3 x 3 convolution with the BatchNorm
    folded in), float32 and contiguous, and ``packed``, the same weights rounded to bfloat16 in the kernel's fragment order.  (cl, co)
    is (64, 32) -- conv2s -- or (128, 64) -- conv4s.  ``on(device)`` gives (and keeps) their copies on a device."""

    DEVICE = ("w", "bias", "packed")

    def __init__(self, w, bias):
        w, bias = self.float32(w, bias)
        shape = (int(w.shape[1]) - DECODER_SKIP, DECODER_SKIP, int(w.shape[0])) if w.dim() == 4 else None
        if shape not in DECODER_SHAPES or tuple(w.shape[2:]) != (3, 3) or tuple(bias.shape) != (shape[2],):
            raise ValueError(f"StageParams: w must be [32,128,3,3] or [64,192,3,3] and bias [co] (got {tuple(w.shape)}, {tuple(bias.shape)}): "
                             "widths other than conv2s' and conv4s' of the ResNet-18 network are not supported")
        self.w, self.bias = w, bias
        self.cl, self.cs, self.co = shape
        self.packed = pack_weights(w)

    @classmethod
    def from_modules(cls, conv3x3, bn, act=None):
        """Folds the ``eval()`` BatchNorm into the convolution in float64, with ``_net.fold_batchnorm``: ``s = gamma /
        sqrt(var + eps)``, ``w = W * s``, ``bias = beta - mean * s``, each rounded once to float32.  Refuses what the fused stage does
        not compute: a BatchNorm in training mode or without running statistics, a LeakyReLU slope other than 0.1 (``act``, where
        given), a convolution with a bias, strides, dilations, groups, widths other than the two supported."""
        check_conv_bn("StageParams", conv3x3, bn)
        if act is not None and not is_leaky(act):
            raise ValueError(f"StageParams: the activation must be LeakyReLU({SLOPE}) (got {act})")
        if (conv3x3.in_channels - DECODER_SKIP, DECODER_SKIP, conv3x3.out_channels) not in DECODER_SHAPES:
            raise ValueError("StageParams: widths other than 128 -> 32 and 192 -> 64 are not supported (the ResNet-18 network's shapes only)")
        if not is_plain_conv(conv3x3, 3, 1, 1, 1):
            raise ValueError("StageParams: expected Conv2d(cin, cout, 3, 1, 1)")
        return cls(*fold_batchnorm(conv3x3, bn))

    @classmethod
    def from_network(cls, net, stage):
        """From a network with the reference's ``conv2s`` / ``conv4s``, each a ``Sequential`` of conv, bn, act: its ``Resnet18_8s`` or
        the stand-in of tools/e2e_amd.py."""
        if stage not in STAGES:
            raise ValueError(f'StageParams: the stage must be one of {STAGES} (got {stage!r})')
        conv, bn, act = conv_bn_act(net, stage, "StageParams")
        return cls.from_modules(conv, bn, act=act)


def fused_stage(lo, skip, params, *, out=None, out_dtype=None, packed=True):
    """A decoder stage for a batch, on the current stream, without synchronising: one launch, no workspace.

    :param lo:        [b,cl,hin,win] float32 / float16 / bfloat16 CUDA tensor, any strides: the previous stage's output
    :param skip:      [b,64,2 hin,2 win] of the same three types (its own), any strides, on the same device: the trunk's features
    :param params:    ``StageParams``; its widths select conv2s' or conv4s' kernel
    :param out:       None or the tensor to write into and return: contiguous ``[b,co,h,w]``
    :param out_dtype: the type of a new ``out``: float32 / float16 / bfloat16; default ``lo``'s
    :param packed:    hand the kernel the packed bfloat16 weights (the hot path); False: the float32 weights, which it gathers and
                      rounds itself -- the same values, so the same result bit for bit, several times slower
    """
    if not isinstance(params, StageParams):
        raise RuntimeError("params must be a StageParams")
    check_input("lo", lo, params.cl)
    check_input("skip", skip, params.cs)
    dev = lo.device
    b, _, hin, win = (int(v) for v in lo.shape)
    h, w = 2 * hin, 2 * win
    if skip.device != dev or tuple(skip.shape) != (b, params.cs, h, w):
        raise RuntimeError(f"skip must be [b,64,2 hin,2 win] = {(b, params.cs, h, w)} on {dev} (got {tuple(skip.shape)} on {skip.device})")
    if b < 1 or hin < 1 or win < 1:
        raise RuntimeError("lo must not be empty")
    shape = (b, params.co, h, w)
    out = new_or_checked_out(out, out_dtype, lo.dtype, shape, dev)
    w32, bias, wpk = params.on(dev)
    lib = load_decoder_library()
    with torch.cuda.device(dev):
        _check(lib.pvnet_decoder_stage(
            _ptr(lo), TYPE_CODES[lo.dtype], _strides(lo, 4), _ptr(skip), TYPE_CODES[skip.dtype], _strides(skip, 4),
            _ptr(wpk if packed else w32), _ptr(bias), b, hin, win, h, w, params.cl, params.cs, params.co,
            DECODER_F_PACKED if packed else 0, _ptr(out), TYPE_CODES[out.dtype], _stream(dev)), "pvnet_decoder_stage")
    return out


__getattr__ = presets_in_net(__name__, "FusedDecoderNet")   # the network class: pvnet_amd/net.py, which imports this module
