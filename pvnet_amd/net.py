"""The fused network for inference: a ``Resnet18_8s`` (the reference's, or the stand-in of tools/e2e_amd.py) with each of its pieces run
through its fused launch or through the wrapped network's own modules -- ``Resnet18_8s.forward`` (lib/networks/model_repository.py:60-78)
and the ``ResNet.forward`` behind it (lib/networks/resnet.py:200-220), written once.

    seg_pred, ver_pred = FusedNet(net)(image)            # the pieces the probes measured faster are fused, the others run their modules
    FusedNet(net, stem=True, layers=LAYERS, stages=STAGES)   # every piece fused

``FusedNet`` is the name to construct.  ``FusedTailNet``, ``FusedDecoderNet``, ``FusedStemNet`` and ``FusedTrunkNet`` are its presets, one
per library in the order the libraries arrived: each fixes the pieces its signature does not offer to "not fused" and holds no forward
code.  The trunk always runs piece by piece, so the reference's must be the fully convolutional one; piece by piece it is the
reference's own forward, bit for bit.  PyTorch is plumbing only.  There is NO CPU fallback for a fused piece.
"""
from __future__ import annotations

import torch
from torch import nn

from ._net import NetworkParts, conv_bn_act
from .decoder import DEFAULT_STAGES, STAGES, StageParams, fused_stage
from .stem import DEFAULT_STEM, StemParams, fused_stem
from .tail import TailParams, fused_tail
from .trunk import DEFAULT_LAYERS, LAYERS, ConvParams, FusedBasicBlock, fused_conv3x3


def bf16_tier_serves(precision, t):
    """whether the bfloat16 tier -- the only one the stem's, the trunk's and the decoder's library have -- serves tensor ``t``: forced
    by ``"bf16"``, barred by ``"f32"``, and with None the tensor's own type decides (float16 / bfloat16, as under ``torch.autocast``)"""
    return precision == "bf16" or (precision is None and t.dtype != torch.float32)


def _drawn_from(what, names, allowed):
    names = tuple(names)
    if not set(names) <= set(allowed) or len(set(names)) != len(names):
        raise ValueError(f"{what} must be drawn from {allowed} (got {names})")
    return names


class FusedNet(nn.Module):
    """The wrapped network with ``fused_stem`` where ``stem`` is true, the pieces of the trunk named in ``layers`` (drawn from
    ``trunk.LAYERS``) through ``fused_conv3x3`` -- ``layer1 .. layer4`` as ``FusedBasicBlock``s, ``fc`` as one launch, ``conv8s`` as one
    launch that reads ``xfc`` and ``x8s`` as its two inputs, so its ``torch.cat`` is not made --, the stages named in ``stages`` (drawn
    from ``decoder.STAGES``) through ``fused_stage``, and always ``fused_tail``.  A piece not named runs the wrapped network's own
    modules.  Returns the reference's ``(seg_pred, ver_pred)``, as views of one tensor of the features' type.

    ``precision=None`` follows autocast: a named piece is fused where what it is handed is float16 or bfloat16, as under
    ``torch.autocast`` (the stem: where autocast is enabled for the image's device with one of the two, or the image has such a type);
    float32 runs the wrapped modules, because those libraries have one tier, and the tail's ``"f32"`` tier.  ``"bf16"`` forces the
    fused pieces and the bfloat16 tail (with the image's type out, outside autocast), ``"f32"`` the modules and the float32 tail."""

    def __init__(self, net, stem=DEFAULT_STEM, layers=DEFAULT_LAYERS, stages=DEFAULT_STAGES, precision=None):
        super().__init__()
        who = type(self).__name__
        if precision not in (None, "bf16", "f32"):
            raise ValueError('precision must be None, "bf16" or "f32"')
        self.stages, self.layers = _drawn_from("stages", stages, STAGES), _drawn_from("layers", layers, LAYERS)
        self.net = net
        self.precision = precision
        self.stem = bool(stem)
        self.seg_dim = int(net.seg_dim)
        self.tail_params = TailParams.from_network(net)
        self.stage_params = {s: StageParams.from_network(net, s) for s in self.stages}
        self.parts = NetworkParts(net, who)
        self.parts.require_fully_conv(who)
        self.stem_params = StemParams.from_network(net) if self.stem else None
        self.blocks = nn.ModuleDict({name: nn.ModuleList(FusedBasicBlock(blk) for blk in seq)
                                     for name, seq in zip(LAYERS[:4], self.parts.layers) if name in self.layers})
        self.fc_params, self.conv8s_params = (ConvParams.from_modules(*conv_bn_act(self.parts, name, who)) if name in self.layers
                                              else None for name in ("fc", "conv8s"))

    def _stem_dtype(self, x):
        """the type the fused stem writes, or None where the wrapped modules run"""
        if not self.stem or self.precision == "f32":
            return None
        if x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") in (torch.float16, torch.bfloat16):
            return torch.get_autocast_dtype("cuda")
        if self.precision == "bf16":
            return x.dtype
        return x.dtype if x.dtype in (torch.float16, torch.bfloat16) else None   # float32 features: the one tier does not serve them

    def _stem(self, x):
        """(x2s, the pooled tensor): fused, or by the wrapped modules"""
        dtype = self._stem_dtype(x)
        return self.parts.eager_stem(x) if dtype is None else fused_stem(x, self.stem_params, out_dtype=dtype)

    def _layer(self, k, x, fuse):
        name = LAYERS[k]
        if not (fuse and name in self.layers):
            return self.parts.layers[k](x)
        for blk in self.blocks[name]:
            x = blk(x)
        return x

    def _trunk(self, x):
        """(conv8s' output, x4s, x2s): what the decoder stages take"""
        x2s, p = self._stem(x)
        fuse = bf16_tier_serves(self.precision, p)
        x4s = self._layer(0, p, fuse)
        x8s = self._layer(1, x4s, fuse)
        x32s = self._layer(3, self._layer(2, x8s, fuse), fuse)
        xfc = fused_conv3x3(x32s, self.fc_params) if fuse and "fc" in self.layers else self.parts.fc(x32s)
        if fuse and "conv8s" in self.layers:
            return fused_conv3x3(xfc, self.conv8s_params, src2=x8s), x4s, x2s
        return self.parts.eager_conv8s(xfc, x8s), x4s, x2s

    def _features(self, x):
        """the output of ``conv2s``"""
        fm, x4s, x2s = self._trunk(x)
        fuse = bf16_tier_serves(self.precision, fm)
        for k, (stage, skip) in enumerate(zip(STAGES, (x4s, x2s))):
            if fuse and stage in self.stages:
                fm = fused_stage(fm, skip, self.stage_params[stage])
            else:
                fm = self.parts.eager_stage(k, fm, skip)
        return fm

    @torch.no_grad()
    def forward(self, x):
        if self.net.training:
            raise RuntimeError(f"{type(self).__name__} is inference only: call eval() on the wrapped network")
        fm = self._features(x)
        y = fused_tail(fm, x, self.tail_params, precision="bf16" if bf16_tier_serves(self.precision, fm) else "f32")
        return y[:, :self.seg_dim], y[:, self.seg_dim:]


class FusedTailNet(FusedNet):
    """``FusedNet`` with only the tail fused (pvnet_amd/tail.py)"""

    def __init__(self, net, precision=None):
        FusedNet.__init__(self, net, stem=False, layers=(), stages=(), precision=precision)

    params = property(lambda self: self.tail_params)


class FusedDecoderNet(FusedNet):
    """``FusedNet`` with the stages named and the tail fused (pvnet_amd/decoder.py); ``stages=()`` is ``FusedTailNet``, bit for bit"""

    def __init__(self, net, stages=DEFAULT_STAGES, precision=None):
        FusedNet.__init__(self, net, stem=False, layers=(), stages=stages, precision=precision)


class FusedStemNet(FusedDecoderNet):
    """``FusedDecoderNet`` with the stem fused as well (pvnet_amd/stem.py); ``stem=False`` is ``FusedDecoderNet``, bit for bit"""

    def __init__(self, net, stem=DEFAULT_STEM, stages=DEFAULT_STAGES, precision=None):
        FusedNet.__init__(self, net, stem=stem, layers=(), stages=stages, precision=precision)


class FusedTrunkNet(FusedStemNet):
    """``FusedNet`` under its first name, with ``layers`` in front (pvnet_amd/trunk.py); ``layers=()`` is ``FusedStemNet``, bit for bit"""

    def __init__(self, net, layers=DEFAULT_LAYERS, stem=DEFAULT_STEM, stages=DEFAULT_STAGES, precision=None):
        FusedNet.__init__(self, net, stem=stem, layers=layers, stages=stages, precision=precision)
