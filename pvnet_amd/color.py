"""The colour jitter of a training batch on the device, alone or fused behind the geometric augmentation.

Every training sample of the reference passes through ``transforms.ColorJitter(brightness, contrast, saturation, hue)``
(lib/datasets/linemod_dataset.py:185-190, applied at :233-234) between its geometric augmentation and ``ToTensor`` + ``Normalize``:

* ``ColorJitterConfig``     -- the reference's ``brightness``, ``contrast``, ``saturation`` and ``hue``, with its defaults;
* ``draw_jitter_uniforms``  -- the randomness, an input: one row of five U[0,1) numbers per sample;
* ``jitter_batch``          -- ``rgb [b,h,w,3] uint8 -> image [b,3,h,w]``, jittered and normalised (``pvnet_color_jitter``);
* ``augment_jitter_batch``  -- ``augment.augment_batch`` with the jitter between its warp and its normalisation
  (``pvnet_augment_jitter``; the plan and the warp are the code ``augment_batch`` runs);
* ``training_configs_from_reference`` -- the reference's JSON as it stands -> ``(AugmentConfig, ColorJitterConfig or None)``.

pvnet_amd/csrc/color_jitter.hip, libpvnet_color.so; C ABI and THE DEFINITION: include/pvnet_color.h (this project's own text of
torchvision 0.2.1's and Pillow's arithmetic, held to Pillow byte for byte: tests/pillow_jitter_oracle.py, tests/golden/color_pillow.npz); a
numpy restatement: tests/color_restatement.py.

``blur`` needs no kernel: the reference calls ``blur_image(rgb, k)`` at linemod_dataset.py:232 and discards what it returns
(augmentation.py:204-205 returns a new array), so ``blur: true`` changes no pixel, and ``training_configs_from_reference`` accepts it.

PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import torch

from ._abi import COLOR_UNIFORMS, ColorConfigStruct, _check, load_color_library
from ._marshal import nbytes as _nbytes, ptr as _ptr, stream as _stream, strides as _strides, workspace as _workspace
from .augment import _MASK_CODES, _MASK_OUT_CODES, _OUT_CODES, MEAN, STD, AugmentConfig, _check_rgb, _prepare_augment


@dataclasses.dataclass
class ColorJitterConfig:
    """The reference's ``brightness``, ``contrast``, ``saturation`` and ``hue`` (the arguments of its ``ColorJitter``), with the values of its
    ``default_linemod_cfg.json`` (tests/golden/default_linemod_cfg.json holds a copy).  A range of 0 leaves its step out."""
    brightness: float = 0.1
    contrast: float = 0.1
    saturation: float = 0.1
    hue: float = 0.1

    def __post_init__(self):
        for name in ("brightness", "contrast", "saturation"):
            if not 0 <= float(getattr(self, name)) <= 1e6:
                raise ValueError(f"ColorJitterConfig: {name} must lie in [0, 1e6]")
        if not 0 <= float(self.hue) <= 0.5:
            raise ValueError("ColorJitterConfig: hue must lie in [0, 0.5]")

    @classmethod
    def from_reference(cls, cfg: dict, **overrides):
        """from a dict with the reference's keys (its JSON); keys this class does not know are ignored, ``overrides`` win"""
        names = {f.name for f in dataclasses.fields(cls)}
        return cls(**{**{k: v for k, v in cfg.items() if k in names}, **overrides})

    def struct(self) -> ColorConfigStruct:
        s = ColorConfigStruct()
        s.brightness, s.contrast, s.saturation, s.hue = (float(getattr(self, n)) for n in ("brightness", "contrast", "saturation", "hue"))
        s.mean[:], s.std[:] = MEAN, STD
        return s


def training_configs_from_reference(cfg: dict, **overrides):
    """The reference's training configuration as it stands (its ``default_linemod_cfg.json``) -> ``(AugmentConfig, ColorJitterConfig)``;
    the second is None for ``jitter: false``.  ``blur`` is accepted as the no-op it is in the reference (see the module's text);
    ``use_old: true`` still raises ``NotImplementedError``.  ``overrides`` are ``AugmentConfig``'s."""
    jitter = ColorJitterConfig.from_reference(cfg) if cfg.get("jitter", False) else None
    return AugmentConfig.from_reference(cfg, **{"blur": False, "jitter": False, **overrides}), jitter


def draw_jitter_uniforms(b, generator=None):
    """``[b,5]`` float64 on the host: one row of independent U[0,1) numbers per sample (u0 .. u4 of include/pvnet_color.h)"""
    return torch.rand((int(b), COLOR_UNIFORMS), dtype=torch.float64, generator=generator)


def _device_jitter_uniforms(uniforms, b, dev):
    if not (isinstance(uniforms, torch.Tensor) and uniforms.dtype == torch.float64 and tuple(uniforms.shape) == (b, COLOR_UNIFORMS)):
        raise RuntimeError(f"jitter uniforms must be a float64 tensor [b,{COLOR_UNIFORMS}] with b={b}")
    if uniforms.is_cuda:
        if uniforms.device != dev or not uniforms.is_contiguous():
            raise RuntimeError(f"device jitter uniforms must be contiguous and on {dev}")
        return uniforms
    if not bool(((uniforms >= 0) & (uniforms < 1)).all()):
        raise RuntimeError("jitter uniforms must lie in [0, 1)")
    return uniforms.contiguous().to(dev)


def color_workspace_bytes(b, height=0, width=0):
    """the workspace ``augment_jitter_batch`` needs for b images of height x width output pixels; with the sizes 0, ``jitter_batch``'s"""
    return int(load_color_library().pvnet_color_workspace_bytes(int(b), int(height), int(width)))


def jitter_batch(rgb, cfg, uniforms, out_dtype=torch.float32, mask=None, maskmul=None, out=None, workspace=None):
    """The reference's ``ColorJitter`` + ``ToTensor`` + ``Normalize`` for a batch, on the current stream, without synchronising.

    :param rgb:      [b,h,w,3] uint8 CUDA tensor, any strides with the channel stride 1
    :param cfg:      ``ColorJitterConfig``
    :param uniforms: ``draw_jitter_uniforms(b)`` (host) or the same on the device, [b,5] float64
    :param mask:     None, or [b,h,w] uint8 / int32 / int64, any strides; with it
    :param maskmul:  [b] int32 (host or device): the images whose normalised value is multiplied by ``(float)mask`` (``use_mask_out``)
    :param out:      None or the image to write into (contiguous [b,3,h,w] of ``out_dtype``)
    :param workspace: None, or a uint8 CUDA tensor of at least ``color_workspace_bytes(b)`` bytes
    :return: ``image [b,3,h,w]`` of ``out_dtype`` (float32 / bfloat16 / float16)
    """
    dev, (b, h, w) = _check_rgb(rgb)
    if not isinstance(cfg, ColorJitterConfig):
        raise RuntimeError("cfg must be a ColorJitterConfig")
    if out_dtype not in _OUT_CODES:
        raise RuntimeError("out_dtype must be float32, bfloat16 or float16")
    if (mask is None) != (maskmul is None):
        raise RuntimeError("mask and maskmul go together")
    mask_ptr, mask_code, mask_strides, mul_ptr = None, 0, None, None
    if mask is not None:
        if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.device == dev and tuple(mask.shape) == (b, h, w) and
                mask.dtype in _MASK_CODES):
            raise RuntimeError(f"mask must be a uint8, int32 or int64 CUDA tensor [b,h,w]={(b, h, w)} on {dev}")
        maskmul = torch.as_tensor(maskmul)
        if tuple(maskmul.shape) != (b,) or maskmul.is_floating_point():
            raise RuntimeError(f"maskmul must be [b]={b} integers")
        maskmul = maskmul.to(device=dev, dtype=torch.int32).contiguous()
        mask_ptr, mask_code, mask_strides, mul_ptr = _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)), _ptr(maskmul)
    packed = _device_jitter_uniforms(uniforms, b, dev)
    if out is None:
        out = torch.empty((b, 3, h, w), dtype=out_dtype, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == out_dtype and
              tuple(out.shape) == (b, 3, h, w) and out.is_contiguous()):
        raise RuntimeError(f"out must be a contiguous {out_dtype} CUDA tensor of shape {(b, 3, h, w)} on {dev}")
    lib = load_color_library()
    workspace = _workspace(workspace, lib.pvnet_color_workspace_bytes(b, 0, 0), dev, least=16)
    struct = cfg.struct()
    with torch.cuda.device(dev):
        _check(lib.pvnet_color_jitter(
            _ptr(rgb), _strides(rgb, (0, 1, 2)), _ptr(packed), b, h, w, C.byref(struct), mask_ptr, mask_code, mask_strides, mul_ptr,
            _ptr(out), _OUT_CODES[out_dtype], _ptr(workspace), _nbytes(workspace), _stream(dev)), "pvnet_color_jitter")
    return out


def augment_jitter_batch(rgb, mask, hcoords, height, width, cfg, jitter_cfg, uniforms, jitter_uniforms, seed, out_dtype=torch.float32,
                         mask_dtype=torch.uint8, out=None, workspace=None):
    """``augment.augment_batch`` with the colour jitter between its warp and its normalisation: the reference's ``augmentation`` +
    ``ColorJitter`` + ``ToTensor`` + ``Normalize`` for a batch, on the current stream, without synchronising.  The arguments and the
    four results are ``augment_batch``'s, and ``mask``, ``hcoords'`` and ``status`` equal its own; added:

    :param jitter_cfg:      ``ColorJitterConfig``
    :param jitter_uniforms: ``draw_jitter_uniforms(b)`` (host) or the same on the device, [b,5] float64
    :param workspace: None, or a uint8 CUDA tensor of at least ``color_workspace_bytes(b, height, width)`` bytes, 16-byte aligned
    """
    height, width = int(height), int(width)
    if not isinstance(jitter_cfg, ColorJitterConfig):
        raise RuntimeError("jitter_cfg must be a ColorJitterConfig")
    dev, (b, h, w), vn, hc, packed, (image, mask_o, hc_o, status) = _prepare_augment(rgb, mask, hcoords, height, width, cfg, uniforms,
                                                                                   out_dtype, mask_dtype, out)
    jpacked = _device_jitter_uniforms(jitter_uniforms, b, dev)
    lib = load_color_library()
    workspace = _workspace(workspace, lib.pvnet_color_workspace_bytes(b, height, width), dev, least=16)
    struct, jstruct = cfg.struct(), jitter_cfg.struct()
    with torch.cuda.device(dev):
        _check(lib.pvnet_augment_jitter(
            _ptr(rgb), _strides(rgb, (0, 1, 2)), _ptr(mask), _MASK_CODES[mask.dtype], _strides(mask, (0, 1, 2)), _ptr(hc), _ptr(packed),
            b, h, w, vn, height, width, C.byref(struct), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(jstruct), _ptr(jpacked),
            _ptr(image), _OUT_CODES[out_dtype], _ptr(mask_o), _MASK_OUT_CODES[mask_dtype], _ptr(hc_o), _ptr(status),
            _ptr(workspace), _nbytes(workspace), _stream(dev)), "pvnet_augment_jitter")
    return image, mask_o, hc_o, status
