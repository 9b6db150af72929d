"""The decoder stages on the device, one launch each (include/pvnet_decoder.h, libpvnet_decoder.so): bilinear 2x upsample of the previous
stage, concatenation with the trunk's skip features, 3 x 3 convolution with the eval() BatchNorm folded in and LeakyReLU(0.1) --
``up8sto4s`` + ``cat`` + ``conv4s`` and ``up4sto2s`` + ``cat`` + ``conv2s`` of the reference's ``Resnet18_8s.forward``
(lib/networks/model_repository.py:29-50, 67-73).  Inference only: no autograd, ``eval()`` BatchNorm; training keeps the PyTorch stages.

    params = StageParams.from_network(net, "conv2s")     # folds the BatchNorm in float64 and packs the weights, once
    fm = fused_stage(lo, skip, params)                   # [b,co,h,w]; lo [b,cl,h/2,w/2] the previous stage, skip [b,64,h,w]
    seg_pred, ver_pred = FusedDecoderNet(net)(image)     # trunk and conv8s under PyTorch, the fused stages, then the fused tail

There is one tier: operands rounded to bfloat16, float32 accumulation on the matrix pipe.  PyTorch is plumbing only.  There is NO CPU
fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import torch
from torch import nn

from ._abi import DECODER_F_PACKED, DECODER_SHAPES, DECODER_SKIP, DECODER_T_BF16, DECODER_T_F16, DECODER_T_F32, _check, load_decoder_library
from ._marshal import ptr as _ptr, stream as _stream, strides as _strides
from .tail import SLOPE, TailParams, fused_tail

_TYPE_CODES = {torch.float32: DECODER_T_F32, torch.float16: DECODER_T_F16, torch.bfloat16: DECODER_T_BF16}
STAGES = ("conv4s", "conv2s")   # the reference's attribute names, in the order the network runs them
# the stages FusedDecoderNet fuses unless told otherwise: those that tools/decoder_probe.py measured faster than the eager stage by more
# than the spread of the eager stage's rounds (profiles/decoder_probe.txt); the other kernel stays reachable by naming its stage
DEFAULT_STAGES = ("conv4s", "conv2s")


def pack_weights(w):
    """``w [co,cin,3,3]`` float32 -> the bfloat16 image PVNET_DECODER_F_PACKED takes, ``[cin/32, 9, 2, co/32, 64, 8]``: element
    (chunk, tap, half, m, lane, j) is ``bf16(w[32 m + (lane & 31)][32 chunk + 16 half + 8 (lane >> 5) + j][tap / 3][tap % 3])``, the
    rounding torch's round-to-nearest-even"""
    co, cin = int(w.shape[0]), int(w.shape[1])
    v = w.to(torch.bfloat16).reshape(co // 32, 32, cin // 32, 2, 2, 8, 9)   # m, r, chunk, half, hh, j, tap
    return v.permute(2, 6, 3, 0, 4, 1, 5).contiguous().reshape(cin // 32, 9, 2, co // 32, 64, 8)


class StageParams:
    """A stage's weights as the library takes them: ``w [co,cl+64,3,3]`` and ``bias [co]`` (the 3 x 3 convolution with the BatchNorm
    folded in), float32 and contiguous, and ``packed``, the same weights rounded to bfloat16 in the kernel's fragment order.  (cl, co)
    is (64, 32) -- conv2s -- or (128, 64) -- conv4s.  ``on(device)`` gives (and keeps) their copies on a device."""

    def __init__(self, w, bias):
        w, bias = (torch.as_tensor(t).detach().to(torch.float32).contiguous() for t in (w, bias))
        shape = (int(w.shape[1]) - DECODER_SKIP, DECODER_SKIP, int(w.shape[0])) if w.dim() == 4 else None
        if shape not in DECODER_SHAPES or tuple(w.shape[2:]) != (3, 3) or tuple(bias.shape) != (shape[2],):
            raise ValueError(f"StageParams: w must be [32,128,3,3] or [64,192,3,3] and bias [co] (got {tuple(w.shape)}, {tuple(bias.shape)}): "
                             "widths other than conv2s' and conv4s' of the ResNet-18 network are not supported")
        self.w, self.bias = w, bias
        self.cl, self.cs, self.co = shape
        self.packed = pack_weights(w)
        self._on = {}

    def on(self, device):
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = tuple(t.to(device) for t in (self.w, self.bias, self.packed))
        return self._on[device]

    @classmethod
    def from_modules(cls, conv3x3, bn, act=None):
        """Folds the ``eval()`` BatchNorm into the convolution in float64, exactly as ``TailParams.from_modules`` does: ``s = gamma /
        sqrt(var + eps)``, ``w = W * s``, ``bias = beta - mean * s``, each rounded once to float32.  Refuses what the fused stage does
        not compute: a BatchNorm in training mode or without running statistics, a LeakyReLU slope other than 0.1 (``act``, where
        given), a convolution with a bias, strides, dilations, groups, widths other than the two supported."""
        if not (isinstance(conv3x3, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d)):
            raise ValueError("StageParams: expected Conv2d, BatchNorm2d")
        if bn.training or bn.running_mean is None or bn.running_var is None:
            raise ValueError("StageParams: the BatchNorm must be in eval() mode with running statistics (inference only)")
        if act is not None and not (isinstance(act, nn.LeakyReLU) and float(act.negative_slope) == SLOPE):
            raise ValueError(f"StageParams: the activation must be LeakyReLU({SLOPE}) (got {act})")
        if conv3x3.bias is not None:
            raise ValueError("StageParams: the reference's 3 x 3 convolution has no bias")
        if (conv3x3.in_channels - DECODER_SKIP, DECODER_SKIP, conv3x3.out_channels) not in DECODER_SHAPES or bn.num_features != conv3x3.out_channels:
            raise ValueError("StageParams: widths other than 128 -> 32 and 192 -> 64 are not supported (the ResNet-18 network's shapes only)")
        plain = (tuple(conv3x3.kernel_size), tuple(conv3x3.stride), tuple(conv3x3.padding), tuple(conv3x3.dilation), conv3x3.groups,
                 conv3x3.padding_mode)
        if plain != ((3, 3), (1, 1), (1, 1), (1, 1), 1, "zeros"):
            raise ValueError("StageParams: expected Conv2d(cin, cout, 3, 1, 1)")
        with torch.no_grad():
            var, mean = bn.running_var.double(), bn.running_mean.double()
            gamma = bn.weight.double() if bn.weight is not None else torch.ones_like(var)
            beta = bn.bias.double() if bn.bias is not None else torch.zeros_like(var)
            s = gamma / torch.sqrt(var + bn.eps)
            return cls((conv3x3.weight.double() * s[:, None, None, None]).float().cpu(), (beta - mean * s).float().cpu())

    @classmethod
    def from_network(cls, net, stage):
        """From a network with the reference's ``conv2s`` / ``conv4s``, each a ``Sequential`` of conv, bn, act: its ``Resnet18_8s`` or
        the stand-in of tools/e2e_amd.py."""
        if stage not in STAGES:
            raise ValueError(f'StageParams: the stage must be one of {STAGES} (got {stage!r})')
        seq = getattr(net, stage, None)
        if not isinstance(seq, nn.Sequential) or len(seq) != 3:
            raise ValueError(f"StageParams: the network has no `{stage}` Sequential of conv, bn, act")
        return cls.from_modules(seq[0], seq[1], act=seq[2])


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
    for name, t, ch in (("lo", lo, params.cl), ("skip", skip, params.cs)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.dtype in _TYPE_CODES):
            raise RuntimeError(f"{name} must be a 4-D float32, float16 or bfloat16 CUDA tensor")
        if t.shape[1] != ch:
            raise RuntimeError(f"{name} must have {ch} channels for these parameters (got {t.shape[1]})")
    dev = lo.device
    b, _, hin, win = (int(v) for v in lo.shape)
    h, w = 2 * hin, 2 * win
    if skip.device != dev or tuple(skip.shape) != (b, params.cs, h, w):
        raise RuntimeError(f"skip must be [b,64,2 hin,2 win] = {(b, params.cs, h, w)} on {dev} (got {tuple(skip.shape)} on {skip.device})")
    if b < 1 or hin < 1 or win < 1:
        raise RuntimeError("lo must not be empty")
    shape = (b, params.co, h, w)
    if out is None:
        dtype = out_dtype if out_dtype is not None else lo.dtype
        if dtype not in _TYPE_CODES:
            raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
        out = torch.empty(shape, dtype=dtype, device=dev)
    else:
        want = out_dtype if out_dtype is not None else out.dtype if isinstance(out, torch.Tensor) else None
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == want and out.dtype in _TYPE_CODES and
                tuple(out.shape) == shape and out.is_contiguous()):
            raise RuntimeError(f"out must be a contiguous {want} CUDA tensor of shape {shape} on {dev}")
    w32, bias, wpk = params.on(dev)
    lib = load_decoder_library()
    with torch.cuda.device(dev):
        _check(lib.pvnet_decoder_stage(
            _ptr(lo), _TYPE_CODES[lo.dtype], _strides(lo, 4), _ptr(skip), _TYPE_CODES[skip.dtype], _strides(skip, 4),
            _ptr(wpk if packed else w32), _ptr(bias), b, hin, win, h, w, params.cl, params.cs, params.co,
            DECODER_F_PACKED if packed else 0, _ptr(out), _TYPE_CODES[out.dtype], _stream(dev)), "pvnet_decoder_stage")
    return out


class FusedDecoderNet(nn.Module):
    """A ``Resnet18_8s`` (the reference's, or the stand-in of tools/e2e_amd.py) for inference with the fused decoder: the wrapped
    network's own trunk and ``conv8s`` run under PyTorch, the stages named in ``stages`` through ``fused_stage`` (a stage not named runs
    its own modules), then ``fused_tail``.  Returns the reference's ``(seg_pred, ver_pred)``, as views of one tensor.

    ``precision=None`` follows autocast: with float16 / bfloat16 features (as under ``torch.autocast``) the named stages and the
    bfloat16 tail run; with float32 features the stages run the wrapped modules -- the library has no float32 tier -- and the tail
    ``"f32"``, as ``FusedTailNet`` does.  ``"bf16"`` forces the fused stages and the bfloat16 tail, ``"f32"`` the modules and the float32
    tail.  The output has the features' type."""

    def __init__(self, net, stages=DEFAULT_STAGES, precision=None):
        super().__init__()
        if precision not in (None, "bf16", "f32"):
            raise ValueError('precision must be None, "bf16" or "f32"')
        stages = tuple(stages)
        if not set(stages) <= set(STAGES) or len(set(stages)) != len(stages):
            raise ValueError(f"stages must be drawn from {STAGES} (got {stages})")
        self.net = net
        self.precision = precision
        self.stages = stages
        self.seg_dim = int(net.seg_dim)
        self.tail_params = TailParams.from_network(net)
        self.stage_params = {s: StageParams.from_network(net, s) for s in stages}
        if hasattr(net, "resnet18_8s"):      # the reference's spelling
            self._trunk, self._ups = self._trunk_reference, (net.up8sto4s, net.up4sto2s)
        elif hasattr(net, "stem"):           # the stand-in's
            self._trunk, self._ups = self._trunk_standin, (net.up, net.up)
        else:
            raise ValueError("FusedDecoderNet: neither the reference's `resnet18_8s` nor the stand-in's `stem`")

    def _trunk_reference(self, x):
        n = self.net
        x2s, x4s, x8s, _, _, xfc = n.resnet18_8s(x)
        return n.conv8s(torch.cat([xfc, x8s], 1)), x4s, x2s

    def _trunk_standin(self, x):
        n = self.net
        x2s = n.stem(x)
        x4s = n.l1(n.pool(x2s))
        x8s = n.l2(x4s)
        xfc = n.fc(n.l4(n.l3(x8s)))
        return n.conv8s(torch.cat([xfc, x8s], 1)), x4s, x2s

    def _features(self, x):
        """the output of ``conv2s`` and whether a fused stage may run on what the trunk handed over"""
        fm, x4s, x2s = self._trunk(x)
        fuse = self.precision == "bf16" or (self.precision is None and fm.dtype != torch.float32)
        for stage, up, skip in zip(STAGES, self._ups, (x4s, x2s)):
            if fuse and stage in self.stages:
                fm = fused_stage(fm, skip, self.stage_params[stage])
            else:
                fm = getattr(self.net, stage)(torch.cat([up(fm), skip], 1))
        return fm

    @torch.no_grad()
    def forward(self, x):
        if self.net.training:
            raise RuntimeError("FusedDecoderNet is inference only: call eval() on the wrapped network")
        fm = self._features(x)
        precision = self.precision or ("f32" if fm.dtype == torch.float32 else "bf16")
        y = fused_tail(fm, x, self.tail_params, precision=precision)
        return y[:, :self.seg_dim], y[:, self.seg_dim:]
