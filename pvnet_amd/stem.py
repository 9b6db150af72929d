"""The network's stem on the device in one launch (include/pvnet_stem.h, libpvnet_stem.so): 7 x 7 stride-2 convolution with the eval()
BatchNorm folded in, ReLU, and the 3 x 3 stride-2 max-pool behind it -- ``conv1`` + ``bn1`` + ``relu`` + ``maxpool`` of the reference's
``ResNet.forward`` (lib/networks/resnet.py:138-142, 200-204).  Inference only: no autograd, ``eval()`` BatchNorm; training keeps the
PyTorch stem.

    params = StemParams.from_network(net)                # folds the BatchNorm in float64, once
    x2s, pooled = fused_stem(image, params)              # [b,64,Ho,Wo] (the decoder's skip input) and [b,64,Hp,Wp] (what layer1 takes)
    seg_pred, ver_pred = FusedStemNet(net)(image)        # fused stem, the residual layers and conv8s under PyTorch, fused stages and tail

There is one tier: operands rounded to bfloat16, float32 accumulation on the matrix pipe.  PyTorch is plumbing only.  There is NO CPU
fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import torch
from torch import nn

from ._abi import STEM_CIN, STEM_COUT, STEM_T_BF16, STEM_T_F16, STEM_T_F32, _check, load_stem_library
from ._marshal import ptr as _ptr, stream as _stream, strides as _strides
from .decoder import DEFAULT_STAGES, FusedDecoderNet

_TYPE_CODES = {torch.float32: STEM_T_F32, torch.float16: STEM_T_F16, torch.bfloat16: STEM_T_BF16}
# whether FusedStemNet fuses the stem unless told otherwise: tools/stem_probe.py measured fused_stem faster than the eager stem and pool
# by more than the spread of the eager rounds (profiles/stem_probe.txt) -- the rule decoder.DEFAULT_STAGES was set by
DEFAULT_STEM = True


def out_sizes(h, w):
    """(Ho, Wo, Hp, Wp) of an h x w image: the header's integer divisions"""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return ho, wo, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1


class StemParams:
    """The stem's weights as the library takes them: ``w [64,3,7,7]`` and ``bias [64]`` (the 7 x 7 convolution with the BatchNorm folded
    in), float32 and contiguous.  ``on(device)`` gives (and keeps) their copies on a device."""

    def __init__(self, w, bias):
        w, bias = (torch.as_tensor(t).detach().to(torch.float32).contiguous() for t in (w, bias))
        if tuple(w.shape) != (STEM_COUT, STEM_CIN, 7, 7) or tuple(bias.shape) != (STEM_COUT,):
            raise ValueError(f"StemParams: w must be [64,3,7,7] and bias [64] (got {tuple(w.shape)}, {tuple(bias.shape)}): "
                             "widths other than the ResNet stem's are not supported")
        self.w, self.bias = w, bias
        self._on = {}

    def on(self, device):
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = tuple(t.to(device) for t in (self.w, self.bias))
        return self._on[device]

    @classmethod
    def from_modules(cls, conv, bn, act=None, pool=None):
        """Folds the ``eval()`` BatchNorm into the convolution in float64, exactly as ``StageParams.from_modules`` does: ``s = gamma /
        sqrt(var + eps)``, ``w = W * s``, ``bias = beta - mean * s``, each rounded once to float32.  Refuses what the fused stem does not
        compute: a BatchNorm in training mode or without running statistics, a convolution that is not ``Conv2d(3, 64, 7, 2, 3,
        bias=False)``, an activation (``act``, where given) that is not ``ReLU``, a pool (where given) that is not ``MaxPool2d(3, 2, 1)``
        with dilation 1 and ``ceil_mode=False``."""
        if not (isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d)):
            raise ValueError("StemParams: expected Conv2d, BatchNorm2d")
        if bn.training or bn.running_mean is None or bn.running_var is None:
            raise ValueError("StemParams: the BatchNorm must be in eval() mode with running statistics (inference only)")
        if act is not None and not isinstance(act, nn.ReLU):
            raise ValueError(f"StemParams: the activation must be ReLU (got {act})")
        if pool is not None:
            def pair(v):
                return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
            if not isinstance(pool, nn.MaxPool2d) or (pair(pool.kernel_size), pair(pool.stride), pair(pool.padding), pair(pool.dilation),
                                                      bool(pool.ceil_mode)) != ((3, 3), (2, 2), (1, 1), (1, 1), False):
                raise ValueError(f"StemParams: the pool must be MaxPool2d(3, 2, 1) with dilation 1 and ceil_mode=False (got {pool})")
        if conv.bias is not None:
            raise ValueError("StemParams: the reference's 7 x 7 convolution has no bias")
        if (conv.in_channels, conv.out_channels, bn.num_features) != (STEM_CIN, STEM_COUT, STEM_COUT):
            raise ValueError("StemParams: widths other than 3 -> 64 are not supported (the ResNet stem's only)")
        plain = (tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation), conv.groups, conv.padding_mode)
        if plain != ((7, 7), (2, 2), (3, 3), (1, 1), 1, "zeros"):
            raise ValueError("StemParams: expected Conv2d(3, 64, 7, 2, 3, bias=False)")
        with torch.no_grad():
            var, mean = bn.running_var.double(), bn.running_mean.double()
            gamma = bn.weight.double() if bn.weight is not None else torch.ones_like(var)
            beta = bn.bias.double() if bn.bias is not None else torch.zeros_like(var)
            s = gamma / torch.sqrt(var + bn.eps)
            return cls((conv.weight.double() * s[:, None, None, None]).float().cpu(), (beta - mean * s).float().cpu())

    @classmethod
    def from_network(cls, net):
        """From a network with the reference's ``resnet18_8s.{conv1,bn1,relu,maxpool}`` (its ``Resnet18_8s``) or the ``stem`` (a
        ``Sequential`` of conv, bn, act) and ``pool`` of the stand-in of tools/e2e_amd.py."""
        trunk = getattr(net, "resnet18_8s", None)
        if trunk is not None and all(hasattr(trunk, n) for n in ("conv1", "bn1", "relu", "maxpool")):
            return cls.from_modules(trunk.conv1, trunk.bn1, act=trunk.relu, pool=trunk.maxpool)
        seq = getattr(net, "stem", None)
        if isinstance(seq, nn.Sequential) and len(seq) == 3 and hasattr(net, "pool"):
            return cls.from_modules(seq[0], seq[1], act=seq[2], pool=net.pool)
        raise ValueError("StemParams: neither the reference's `resnet18_8s.conv1, bn1, relu, maxpool` nor the stand-in's `stem` "
                         "Sequential of conv, bn, act with `pool`")


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
    if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dim() == 4 and image.dtype in _TYPE_CODES):
        raise RuntimeError("image must be a 4-D float32, float16 or bfloat16 CUDA tensor")
    if image.shape[1] != STEM_CIN:
        raise RuntimeError(f"image must have {STEM_CIN} channels (got {image.shape[1]})")
    dev = image.device
    b, _, h, w = (int(v) for v in image.shape)
    if b < 1 or h < 1 or w < 1:
        raise RuntimeError("image must not be empty")
    ho, wo, hp, wp = out_sizes(h, w)
    shapes = ((b, STEM_COUT, ho, wo), (b, STEM_COUT, hp, wp))
    if out is None:
        dtype = out_dtype if out_dtype is not None else image.dtype
        if dtype not in _TYPE_CODES:
            raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
        x2s = torch.empty(shapes[0], dtype=dtype, device=dev)
        pooled = torch.empty(shapes[1], dtype=dtype, device=dev) if pool else None
    else:
        x2s, pooled = (out, None) if isinstance(out, torch.Tensor) else tuple(out) if len(out) == 2 else (None, None)
        if (pooled is not None) != bool(pool):
            raise RuntimeError("out must be (x2s, pooled) with the pool and x2s or (x2s, None) without it")
        want = out_dtype if out_dtype is not None else x2s.dtype if isinstance(x2s, torch.Tensor) else None
        for name, t, shape in (("x2s", x2s, shapes[0]), ("pooled", pooled, shapes[1]))[:2 if pool else 1]:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == want and t.dtype in _TYPE_CODES and
                    tuple(t.shape) == shape and t.is_contiguous()):
                raise RuntimeError(f"out: {name} must be a contiguous {want} CUDA tensor of shape {shape} on {dev}")
    w32, bias = params.on(dev)
    lib = load_stem_library()
    with torch.cuda.device(dev):
        _check(lib.pvnet_stem_forward(_ptr(image), _TYPE_CODES[image.dtype], _strides(image, 4), _ptr(w32), _ptr(bias), b, h, w,
                                      _ptr(x2s), _ptr(pooled) if pool else None, _TYPE_CODES[x2s.dtype], _stream(dev)), "pvnet_stem_forward")
    return x2s, pooled


class FusedStemNet(FusedDecoderNet):
    """``FusedDecoderNet`` with the trunk run piecewise: ``fused_stem``, then the wrapped network's own ``layer1 .. layer4`` and ``fc``
    (the stand-in's ``l1 .. l4``, ``fc``) and ``conv8s`` under PyTorch, then the fused stages and the fused tail.  Returns the reference's
    ``(seg_pred, ver_pred)``, as views of one tensor.

    ``stem=False`` runs the wrapped stem modules: the network is then ``FusedDecoderNet``'s, bit for bit.  ``precision`` is
    ``FusedDecoderNet``'s: ``None`` follows autocast -- the stem is fused where autocast is enabled for the image's device with float16 or
    bfloat16, and x2s and the pooled tensor then have that type, as the eager stem's have; with float32 features the stem runs the
    wrapped modules, because the library has one tier --, ``"bf16"`` forces the fused stem (with the image's type out, outside autocast),
    ``"f32"`` the modules."""

    def __init__(self, net, stem=DEFAULT_STEM, stages=DEFAULT_STAGES, precision=None):
        super().__init__(net, stages=stages, precision=precision)
        self.stem = bool(stem)
        self.stem_params = StemParams.from_network(net) if self.stem else None
        trunk = getattr(net, "resnet18_8s", None)
        if trunk is not None:    # the reference's spelling: its forward, piecewise, is the fully convolutional one only
            if not (getattr(trunk, "fully_conv", False) and getattr(trunk, "remove_avg_pool_layer", False)):
                raise ValueError("FusedStemNet: the reference's trunk must be built with fully_conv=True, remove_avg_pool_layer=True")
            self._stem_modules = lambda x: trunk.relu(trunk.bn1(trunk.conv1(x)))
            self._pool, self._layers, self._fc = trunk.maxpool, (trunk.layer1, trunk.layer2, trunk.layer3, trunk.layer4), trunk.fc
        else:                    # the stand-in's (FusedDecoderNet has refused anything else)
            self._stem_modules, self._pool, self._layers, self._fc = net.stem, net.pool, (net.l1, net.l2, net.l3, net.l4), net.fc
        self._trunk = self._trunk_piecewise

    def _stem_dtype(self, x):
        """the type the fused stem writes, or None where the wrapped modules run"""
        if not self.stem or self.precision == "f32":
            return None
        if x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") in (torch.float16, torch.bfloat16):
            return torch.get_autocast_dtype("cuda")
        if self.precision == "bf16":
            return x.dtype
        return x.dtype if x.dtype in (torch.float16, torch.bfloat16) else None   # float32 features: the one tier does not serve them

    def _trunk_piecewise(self, x):
        dtype = self._stem_dtype(x)
        if dtype is None:
            x2s = self._stem_modules(x)
            p = self._pool(x2s)
        else:
            x2s, p = fused_stem(x, self.stem_params, out_dtype=dtype)
        x4s = self._layers[0](p)
        x8s = self._layers[1](x4s)
        xfc = self._fc(self._layers[3](self._layers[2](x8s)))
        return self.net.conv8s(torch.cat([xfc, x8s], 1)), x4s, x2s
