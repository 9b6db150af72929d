"""The network's tail on the device in one launch (include/pvnet_tail.h, libpvnet_tail.so): bilinear 2x upsample of the last decoder
stage, concatenation with the image, 3 x 3 convolution with the eval() BatchNorm folded in, LeakyReLU(0.1) and the 1 x 1 convolution
to the seg / vertex channels -- ``up2storaw`` + ``cat`` + ``convraw`` of the reference's ``Resnet18_8s.forward``
(lib/networks/model_repository.py:51-58, 74-78).  Inference only: no autograd, ``eval()`` BatchNorm; training keeps the PyTorch tail.

    params = TailParams.from_network(net)              # folds the BatchNorm in float64, once
    out = fused_tail(fm, image, params)                # [b,cout,h,w]; fm [b,32,h/2,w/2] is the output of conv2s, image [b,3,h,w]
    seg_pred, ver_pred = FusedTailNet(net)(image)      # the wrapped network's trunk under PyTorch, then the fused tail

``seg_pred`` / ``ver_pred`` are views of one tensor; ``voting.EvalWrapper`` / ``PoseEvalWrapper`` and the ``_from_logits`` entries take
them as they are.  PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise
``RuntimeError``.
"""
from __future__ import annotations

import torch
from torch import nn

from ._abi import TAIL_BF16, TAIL_F32, TAIL_F_RAW, TAIL_MAX_COUT, TAIL_T_BF16, TAIL_T_F16, TAIL_T_F32, TAIL_WIDTH, _check, load_tail_library
from ._marshal import ptr as _ptr, stream as _stream, strides as _strides

_TYPE_CODES = {torch.float32: TAIL_T_F32, torch.float16: TAIL_T_F16, torch.bfloat16: TAIL_T_BF16}
_PRECISIONS = {"bf16": TAIL_BF16, "f32": TAIL_F32}
SLOPE = 0.1   # the LeakyReLU of the reference's decoder stages


class TailParams:
    """The tail's weights as the library takes them, float32 and contiguous: ``w1 [32,35,3,3]`` and ``b1 [32]`` (the 3 x 3 convolution
    with the BatchNorm folded in), ``w2 [cout,32]`` and ``b2 [cout]`` (the 1 x 1 convolution).  ``on(device)`` gives (and keeps) their
    copies on a device."""

    def __init__(self, w1, b1, w2, b2):
        w1, b1, w2, b2 = (torch.as_tensor(t).detach().to(torch.float32).contiguous() for t in (w1, b1, w2, b2))
        cout = int(w2.shape[0]) if w2.dim() == 2 else -1
        if tuple(w1.shape) != (TAIL_WIDTH, TAIL_WIDTH + 3, 3, 3) or tuple(b1.shape) != (TAIL_WIDTH,):
            raise ValueError(f"TailParams: w1 must be [32,35,3,3] and b1 [32] (got {tuple(w1.shape)}, {tuple(b1.shape)}): the ResNet-18 widths only")
        if not 1 <= cout <= TAIL_MAX_COUT or tuple(w2.shape) != (cout, TAIL_WIDTH) or tuple(b2.shape) != (cout,):
            raise ValueError(f"TailParams: w2 must be [cout,32] and b2 [cout] with 1 <= cout <= 32 (got {tuple(w2.shape)}, {tuple(b2.shape)})")
        self.w1, self.b1, self.w2, self.b2 = w1, b1, w2, b2
        self.cout = cout
        self._on = {}

    def on(self, device):
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = tuple(t.to(device) for t in (self.w1, self.b1, self.w2, self.b2))
        return self._on[device]

    @classmethod
    def from_modules(cls, conv3x3, bn, conv1x1, act=None):
        """Folds the ``eval()`` BatchNorm into the 3 x 3 convolution in float64: ``s = gamma / sqrt(var + eps)``, ``w1 = W * s``,
        ``b1 = beta - mean * s``, each rounded once to float32.  Refuses what the fused tail does not compute: a BatchNorm in training
        mode or without running statistics, a LeakyReLU slope other than 0.1 (``act``, where given), a 3 x 3 convolution with a bias or
        a 1 x 1 convolution without one, widths other than 32, strides, dilations, groups."""
        if not (isinstance(conv3x3, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d) and isinstance(conv1x1, nn.Conv2d)):
            raise ValueError("TailParams: expected Conv2d, BatchNorm2d, Conv2d")
        if bn.training or bn.running_mean is None or bn.running_var is None:
            raise ValueError("TailParams: the BatchNorm must be in eval() mode with running statistics (inference only)")
        if act is not None and not (isinstance(act, nn.LeakyReLU) and float(act.negative_slope) == SLOPE):
            raise ValueError(f"TailParams: the activation must be LeakyReLU({SLOPE}) (got {act})")
        if conv3x3.bias is not None or conv1x1.bias is None:
            raise ValueError("TailParams: the reference's 3 x 3 convolution has no bias and its 1 x 1 convolution has one")
        if (conv3x3.in_channels, conv3x3.out_channels, conv1x1.in_channels, bn.num_features) != (TAIL_WIDTH + 3, TAIL_WIDTH, TAIL_WIDTH, TAIL_WIDTH):
            raise ValueError("TailParams: widths other than 35 -> 32 -> cout are not supported (the ResNet-18 network's shapes only)")
        if not 1 <= conv1x1.out_channels <= TAIL_MAX_COUT:
            raise ValueError("TailParams: 1 <= cout <= 32")
        plain3 = (tuple(conv3x3.kernel_size), tuple(conv3x3.stride), tuple(conv3x3.padding), tuple(conv3x3.dilation), conv3x3.groups,
                  conv3x3.padding_mode)
        plain1 = (tuple(conv1x1.kernel_size), tuple(conv1x1.stride), tuple(conv1x1.padding), tuple(conv1x1.dilation), conv1x1.groups)
        if plain3 != ((3, 3), (1, 1), (1, 1), (1, 1), 1, "zeros") or plain1 != ((1, 1), (1, 1), (0, 0), (1, 1), 1):
            raise ValueError("TailParams: expected Conv2d(35, 32, 3, 1, 1) and Conv2d(32, cout, 1, 1)")
        with torch.no_grad():
            var, mean = bn.running_var.double(), bn.running_mean.double()
            gamma = bn.weight.double() if bn.weight is not None else torch.ones_like(var)
            beta = bn.bias.double() if bn.bias is not None else torch.zeros_like(var)
            s = gamma / torch.sqrt(var + bn.eps)
            w1 = conv3x3.weight.double() * s[:, None, None, None]
            b1 = beta - mean * s
            return cls(w1.float().cpu(), b1.float().cpu(), conv1x1.weight.detach().reshape(conv1x1.out_channels, TAIL_WIDTH).float().cpu(),
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
    for name, t, ch in (("fm", fm, TAIL_WIDTH), ("image", image, 3)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.dtype in _TYPE_CODES):
            raise RuntimeError(f"{name} must be a 4-D float32, float16 or bfloat16 CUDA tensor")
        if t.shape[1] != ch:
            raise RuntimeError(f"{name} must have {ch} channels (got {t.shape[1]}): the ResNet-18 network's shapes only")
    dev = fm.device
    b, _, hin, win = (int(v) for v in fm.shape)
    h, w = 2 * hin, 2 * win
    if image.device != dev or tuple(image.shape) != (b, 3, h, w):
        raise RuntimeError(f"image must be [b,3,2 hin,2 win] = {(b, 3, h, w)} on {dev} (got {tuple(image.shape)} on {image.device})")
    if b < 1 or hin < 1 or win < 1:
        raise RuntimeError("fm must not be empty")
    shape = (b, TAIL_WIDTH if raw else params.cout, h, w)
    if out is None:
        dtype = torch.float32 if raw else (out_dtype if out_dtype is not None else fm.dtype)
        if dtype not in _TYPE_CODES:
            raise RuntimeError("out_dtype must be float32, float16 or bfloat16")
        out = torch.empty(shape, dtype=dtype, device=dev)
    else:
        want = torch.float32 if raw else (out_dtype if out_dtype is not None else out.dtype if isinstance(out, torch.Tensor) else None)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == want and out.dtype in _TYPE_CODES and
                tuple(out.shape) == shape and out.is_contiguous()):
            raise RuntimeError(f"out must be a contiguous {want} CUDA tensor of shape {shape} on {dev}")
    w1, b1, w2, b2 = params.on(dev)
    lib = load_tail_library()
    with torch.cuda.device(dev):
        _check(lib.pvnet_tail_forward(
            _ptr(fm), _TYPE_CODES[fm.dtype], _strides(fm, 4), _ptr(image), _TYPE_CODES[image.dtype], _strides(image, 4),
            _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), b, hin, win, h, w, TAIL_WIDTH, TAIL_WIDTH, params.cout, _PRECISIONS[precision],
            TAIL_F_RAW if raw else 0, _ptr(out), _TYPE_CODES[out.dtype], _stream(dev)), "pvnet_tail_forward")
    return out


class FusedTailNet(nn.Module):
    """A ``Resnet18_8s`` (the reference's, or the stand-in of tools/e2e_amd.py) for inference with the fused tail: the wrapped network's
    own trunk and decoder modules run under PyTorch up to ``conv2s``, then ``fused_tail``.  Returns the reference's ``(seg_pred,
    ver_pred)``, as views of one tensor.

    ``precision=None`` follows autocast: the tail runs ``"bf16"`` when the trunk hands it float16 / bfloat16 features (as under
    ``torch.autocast``) and ``"f32"`` for float32 features; ``"bf16"`` / ``"f32"`` fix it.  The output has the features' type."""

    def __init__(self, net, precision=None):
        super().__init__()
        if precision is not None and precision not in _PRECISIONS:
            raise ValueError('precision must be None, "bf16" or "f32"')
        self.net = net
        self.precision = precision
        self.seg_dim = int(net.seg_dim)
        self.params = TailParams.from_network(net)
        if hasattr(net, "resnet18_8s"):      # the reference's spelling
            self._features = self._features_reference
        elif hasattr(net, "stem"):           # the stand-in's
            self._features = self._features_standin
        else:
            raise ValueError("FusedTailNet: neither the reference's `resnet18_8s` nor the stand-in's `stem`")

    def _features_reference(self, x):
        n = self.net
        x2s, x4s, x8s, _, _, xfc = n.resnet18_8s(x)
        fm = n.up8sto4s(n.conv8s(torch.cat([xfc, x8s], 1)))
        fm = n.up4sto2s(n.conv4s(torch.cat([fm, x4s], 1)))
        return n.conv2s(torch.cat([fm, x2s], 1))

    def _features_standin(self, x):
        n = self.net
        x2s = n.stem(x)
        x4s = n.l1(n.pool(x2s))
        x8s = n.l2(x4s)
        xfc = n.fc(n.l4(n.l3(x8s)))
        fm = n.up(n.conv8s(torch.cat([xfc, x8s], 1)))
        fm = n.up(n.conv4s(torch.cat([fm, x4s], 1)))
        return n.conv2s(torch.cat([fm, x2s], 1))

    @torch.no_grad()
    def forward(self, x):
        if self.net.training:
            raise RuntimeError("FusedTailNet is inference only: call eval() on the wrapped network")
        fm = self._features(x)
        precision = self.precision or ("f32" if fm.dtype == torch.float32 else "bf16")
        y = fused_tail(fm, x, self.params, precision=precision)
        return y[:, :self.seg_dim], y[:, self.seg_dim:]
