"""The inputs of a training step on the device: geometric augmentation of a batch from the decoded uint8 sample.

The reference augments on the host, per sample (``LineModDatasetRealAug.augmentation``, lib/datasets/linemod_dataset.py:254-290, and
lib/datasets/augmentation.py), then ``ToTensor`` + ``Normalize``, and ships a float32 image and an int64 mask.  With the targets made
from the key-points (``validation.HeadLoss.from_keypoints``) a sample's supervision is a mask and ``hcoords [vn,3]``, so the same
augmentation is one fused warp of a uint8 image and a mask plus a few affine updates of 3 vn numbers:

* ``AugmentConfig``   -- the reference's configuration keys that are implemented, with its defaults;
* ``draw_uniforms``   -- the randomness, an input: one row of twelve U[0,1) numbers per sample;
* ``augment_batch``   -- ``(rgb, mask, hcoords) -> (image, mask, hcoords', status)`` (``pvnet_augment``, pvnet_amd/csrc/augment.hip,
  libpvnet_augment.so; C ABI and THE DEFINITION: include/pvnet_augment.h; a numpy restatement: tests/augment_restatement.py);
* ``normalize_batch`` -- the identity plan, the reference's ``test_img_transforms`` for a validation batch.

PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import torch

from ._abi import (AUGMENT_F_CROP, AUGMENT_F_FLIP, AUGMENT_F_MASK, AUGMENT_F_ROTATION, AUGMENT_F_USE_MASK_OUT, AUGMENT_OUT_BF16,
                   AUGMENT_OUT_F16, AUGMENT_OUT_F32, AUGMENT_S_DEGENERATE, AUGMENT_S_EMPTIED, AUGMENT_S_NO_FOREGROUND,  # noqa: F401
                   AUGMENT_S_RANGE, AUGMENT_UNIFORMS, MASK_I32, MASK_I64, MASK_U8, AugmentConfigStruct, _check, load_augment_library)
from ._marshal import nbytes as _nbytes, ptr as _ptr, stream as _stream, strides as _strides, workspace as _workspace

N_UNIFORMS = 12   # u0 .. u11 of include/pvnet_augment.h
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # the reference's Normalize (linemod_dataset.py:188-189)
_OUT_CODES = {torch.float32: AUGMENT_OUT_F32, torch.bfloat16: AUGMENT_OUT_BF16, torch.float16: AUGMENT_OUT_F16}
_MASK_CODES = {torch.uint8: MASK_U8, torch.int32: MASK_I32, torch.int64: MASK_I64}
_MASK_OUT_CODES = {torch.uint8: MASK_U8, torch.int64: MASK_I64}


@dataclasses.dataclass
class AugmentConfig:
    """The keys of the reference's ``default_linemod_cfg.json`` that are implemented, with its default values
    (tests/golden/default_linemod_cfg.json holds a copy).  ``use_old`` (crop_resize_instance_v1), ``blur`` and ``jitter`` are not
    implemented: asking for them raises ``NotImplementedError``."""
    mask: bool = True
    min_mask: float = 0.1
    max_mask: float = 0.4
    rotation: bool = True
    rot_ang_min: float = -30
    rot_ang_max: float = 30
    crop: bool = True
    overlap_ratio: float = 0.5
    resize_hmin: float = 20
    resize_hmax: float = 130
    resize_wmin: float = 20
    resize_wmax: float = 130
    flip: bool = True
    use_mask_out: bool = False
    use_old: bool = False
    blur: bool = False
    jitter: bool = False

    def __post_init__(self):
        for name in ("use_old", "blur", "jitter"):
            if getattr(self, name):
                raise NotImplementedError(f"AugmentConfig: {name}=True is not implemented on the device")

    @classmethod
    def from_reference(cls, cfg: dict, **overrides):
        """from a dict with the reference's keys (its JSON); keys this class does not know are ignored, ``overrides`` win"""
        names = {f.name for f in dataclasses.fields(cls)}
        return cls(**{**{k: v for k, v in cfg.items() if k in names}, **overrides})

    @classmethod
    def identity(cls):
        """every step off: ``augment_batch`` then normalises only"""
        return cls(mask=False, rotation=False, crop=False, flip=False, use_mask_out=False)

    def flags(self) -> int:
        return (AUGMENT_F_MASK if self.mask else 0) | (AUGMENT_F_ROTATION if self.rotation else 0) | (AUGMENT_F_CROP if self.crop else 0) | \
            (AUGMENT_F_FLIP if self.flip else 0) | (AUGMENT_F_USE_MASK_OUT if self.use_mask_out else 0)

    def struct(self) -> AugmentConfigStruct:
        s = AugmentConfigStruct()
        s.flags, s.reserved = self.flags(), 0
        for name in ("min_mask", "max_mask", "overlap_ratio", "resize_hmin", "resize_hmax", "resize_wmin", "resize_wmax"):
            setattr(s, name, float(getattr(self, name)))
        s.mean[:], s.std[:] = MEAN, STD
        return s


def draw_uniforms(b, generator=None):
    """``[b,12]`` float64 on the host: one row of independent U[0,1) numbers per sample (u0 .. u11 of include/pvnet_augment.h)"""
    return torch.rand((int(b), N_UNIFORMS), dtype=torch.float64, generator=generator)


def pack_uniforms(uniforms, cfg, device):
    """``uniforms [b,12]`` (host) -> ``[b,14]`` float64 on ``device``: the row, then cos and sin of the rotation angle
    ``(rot_ang_min + (rot_ang_max - rot_ang_min) u5) pi / 180``, computed here on the host with ``math.cos`` / ``math.sin``.
    ``augment_batch`` does this itself for a host tensor; do it beforehand where the call is captured in a graph."""
    if not (isinstance(uniforms, torch.Tensor) and not uniforms.is_cuda and uniforms.dtype == torch.float64 and uniforms.dim() == 2
            and uniforms.shape[1] == N_UNIFORMS):
        raise RuntimeError(f"uniforms must be a host float64 tensor [b,{N_UNIFORMS}]")
    if not bool(((uniforms >= 0) & (uniforms < 1)).all()):
        raise RuntimeError("uniforms must lie in [0, 1)")
    lo, hi = float(cfg.rot_ang_min), float(cfg.rot_ang_max)
    rows = []
    for row in uniforms.tolist():
        ang = (lo + (hi - lo) * row[5]) * math.pi / 180.0
        rows.append(row + [math.cos(ang), math.sin(ang)])
    return torch.tensor(rows, dtype=torch.float64).reshape(-1, AUGMENT_UNIFORMS).to(device)


def _check_rgb(rgb):
    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda):
        raise RuntimeError("rgb must be a CUDA tensor (there is no CPU fallback)")
    if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.stride(3) != 1:
        raise RuntimeError(f"rgb must be uint8 [b,h,w,3] with the channel stride 1, got {rgb.dtype} {tuple(rgb.shape)}")
    return rgb.device, tuple(int(x) for x in rgb.shape[:3])


def _prepare_augment(rgb, mask, hcoords, height, width, cfg, uniforms, out_dtype, mask_dtype, out):
    """the argument checks, the packed uniforms and the four outputs of ``augment_batch`` (shared with ``color.augment_jitter_batch``)
    -> ``dev, (b, h, w), vn, hcoords (contiguous), packed uniforms, (image, mask, hcoords', status)``"""
    dev, (b, h, w) = _check_rgb(rgb)
    height, width = int(height), int(width)
    if not isinstance(cfg, AugmentConfig):
        raise RuntimeError("cfg must be an AugmentConfig")
    for name, t in (("mask", mask), ("hcoords", hcoords)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev):
            raise RuntimeError(f"{name} must be a CUDA tensor on {dev} (there is no CPU fallback)")
    if tuple(mask.shape) != (b, h, w) or mask.dtype not in _MASK_CODES:
        raise RuntimeError(f"mask must be uint8, int32 or int64 [b,h,w]={(b, h, w)}, got {mask.dtype} {tuple(mask.shape)}")
    if hcoords.dtype != torch.float64 or hcoords.dim() != 3 or hcoords.shape[0] != b or hcoords.shape[2] != 3 or hcoords.shape[1] == 0:
        raise RuntimeError(f"hcoords must be float64 [b,vn,3] with b={b}, got {hcoords.dtype} {tuple(hcoords.shape)}")
    if out_dtype not in _OUT_CODES or mask_dtype not in _MASK_OUT_CODES:
        raise RuntimeError("out_dtype must be float32, bfloat16 or float16 and mask_dtype uint8 or int64")
    if not cfg.crop and (height, width) != (h, w):
        raise RuntimeError("without cfg.crop the output size must be the source's")
    vn = int(hcoords.shape[1])
    hc = hcoords.contiguous()
    if isinstance(uniforms, torch.Tensor) and uniforms.is_cuda:
        if not (uniforms.device == dev and uniforms.dtype == torch.float64 and tuple(uniforms.shape) == (b, AUGMENT_UNIFORMS) and
                uniforms.is_contiguous()):
            raise RuntimeError(f"device uniforms must be a contiguous float64 tensor [b,{AUGMENT_UNIFORMS}] (pack_uniforms)")
        packed = uniforms
    else:
        packed = pack_uniforms(uniforms, cfg, dev)
        if packed.shape[0] != b:
            raise RuntimeError(f"uniforms must have b={b} rows")
    shapes = ((torch.Size((b, 3, height, width)), out_dtype), (torch.Size((b, height, width)), mask_dtype),
              (torch.Size((b, vn, 3)), torch.float64), (torch.Size((b,)), torch.int32))
    if out is None:
        out = tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in shapes)
    else:
        out = tuple(out)
        if len(out) != 4:
            raise RuntimeError("out must be (image, mask, hcoords, status)")
        for k, (t, (s, dt)) in enumerate(zip(out, shapes)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dt and t.shape == s and t.is_contiguous()):
                raise RuntimeError(f"out[{k}] must be a contiguous {dt} CUDA tensor of shape {tuple(s)} on {dev}")
    return dev, (b, h, w), vn, hc, packed, out


def augment_workspace_bytes(b):
    """the workspace ``augment_batch`` needs for b images (bytes)"""
    return int(load_augment_library().pvnet_augment_workspace_bytes(int(b)))


def augment_batch(rgb, mask, hcoords, height, width, cfg, uniforms, seed, out_dtype=torch.float32, mask_dtype=torch.uint8, out=None,
                  workspace=None):
    """The reference's ``augmentation`` + ``ToTensor`` + ``Normalize`` for a batch, on the current stream, without synchronising.

    :param rgb:      [b,h,w,3] uint8 CUDA tensor, any strides with the channel stride 1
    :param mask:     [b,h,w] uint8 / int32 / int64, any strides
    :param hcoords:  [b,vn,3] float64
    :param cfg:      ``AugmentConfig``
    :param uniforms: ``draw_uniforms(b)`` (host, [b,12]) or ``pack_uniforms(...)`` of it (device, [b,14])
    :param seed:     of the masked-out rectangle's fill
    :param out:      None or ``(image, mask, hcoords', status)`` to write into (contiguous, of the shapes and types below)
    :param workspace: None, or a uint8 CUDA tensor of at least ``augment_workspace_bytes(b)`` bytes
    :return: ``image [b,3,height,width]`` of ``out_dtype`` (float32 / bfloat16 / float16), normalised; ``mask [b,height,width]`` of
             ``mask_dtype`` (uint8 / int64); ``hcoords' [b,vn,3]`` float64, what ``HeadLoss.from_keypoints`` takes; ``status [b]``
             int32 (``AUGMENT_S_*``)
    """
    height, width = int(height), int(width)
    dev, (b, h, w), vn, hc, packed, (image, mask_o, hc_o, status) = _prepare_augment(rgb, mask, hcoords, height, width, cfg, uniforms,
                                                                                   out_dtype, mask_dtype, out)
    lib = load_augment_library()
    workspace = _workspace(workspace, lib.pvnet_augment_workspace_bytes(b), dev, least=8)
    struct = cfg.struct()
    with torch.cuda.device(dev):
        _check(lib.pvnet_augment(
            _ptr(rgb), _strides(rgb, (0, 1, 2)), _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)), _ptr(hc), _ptr(packed),
            b, h, w, vn, height, width, C.byref(struct), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(image), _OUT_CODES[out_dtype],
            _ptr(mask_o), _MASK_OUT_CODES[mask_dtype], _ptr(hc_o), _ptr(status), _ptr(workspace), _nbytes(workspace), _stream(dev)),
            "pvnet_augment")
    return image, mask_o, hc_o, status


def normalize_batch(rgb, out_dtype=torch.float32, out=None):
    """The identity plan, the reference's ``test_img_transforms`` for a batch: ``rgb [b,h,w,3]`` uint8 ->
    ``[b,3,h,w]`` of ``out_dtype``, ``((float)rgb / 255 - mean) / std`` in float32, rounded once.  One launch on the current stream."""
    dev, (b, h, w) = _check_rgb(rgb)
    if out_dtype not in _OUT_CODES:
        raise RuntimeError("out_dtype must be float32, bfloat16 or float16")
    if out is None:
        out = torch.empty((b, 3, h, w), dtype=out_dtype, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == out_dtype and
              tuple(out.shape) == (b, 3, h, w) and out.is_contiguous()):
        raise RuntimeError(f"out must be a contiguous {out_dtype} CUDA tensor of shape {(b, 3, h, w)} on {dev}")
    struct = AugmentConfig.identity().struct()
    with torch.cuda.device(dev):
        _check(load_augment_library().pvnet_normalize(
            _ptr(rgb), _strides(rgb, (0, 1, 2)), b, h, w, C.byref(struct), _ptr(out), _OUT_CODES[out_dtype], _stream(dev)),
            "pvnet_normalize")
    return out
