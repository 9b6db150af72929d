"""Textured images of posed meshes on the device: ``shade.render_color`` for meshes that may carry a texture image and per-vertex UV
coordinates, the step from a pose to a training image for a scanned or YCB-style model.

The reference's OpenGL renderer has that branch (lib/utils/opengl_render_backend.py:68-69, 95-96: ``u_use_texture``; 316-323, 344-352: the
flipped texture and ``model['texture_uv']``; lib/utils/render_utils.py:424-427, 471-473: ``texture_u`` / ``texture_v`` of the PLY file).
Here:

* ``TexturedMeshes``        -- ``shade.ColorMeshes`` whose meshes may also carry ``uv [P,2]`` and a texture ``uint8 [th,tw,3 or 4]``;
* ``render_textured``       -- ``shade.render_color``'s front end with a ``filter``: a covered pixel of a textured mesh takes its colour
                               from the texture (nearest or bilinear, clamp to edge, perspective-correct), any other pixel is
                               ``render_color``'s; textured and untextured meshes may share an image;
* ``texture_workspace_bytes``;
* ``read_textured_ply``     -- ``shade.read_ply`` plus the per-vertex ``uv``.

pvnet_amd/csrc/texture.hip, libpvnet_texture.so; C ABI and THE DEFINITION: include/pvnet_texture.h; a numpy restatement:
tests/texture_restatement.py.  The texel value is this project's own definition: no pixel of the reference's renderer could be recorded.

Everything is enqueued on the current stream without synchronising; with caller-owned outputs and ``workspace`` a call is capturable
in a graph.  PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _mesh
from ._abi import TEXTURE_BILINEAR, TEXTURE_MAX_INSTANCES, TEXTURE_MAX_SIDE, TEXTURE_NEAREST
from ._marshal import ptr as _ptr
from .shade import SHADING, ColorMeshes, parse_ply   # noqa: F401 (SHADING: this module's name for it too)

FILTER = {"nearest": TEXTURE_NEAREST, "bilinear": TEXTURE_BILINEAR}


def pack_texels(texture):
    """uint8 [th,tw,3] or [th,tw,4] (alpha is dropped) -> uint32 [th,tw]: R | G << 8 | B << 16, rows as given (the top row first)"""
    t = np.asarray(texture)
    if t.dtype != np.uint8 or t.ndim != 3 or t.shape[2] not in (3, 4) or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("a texture must be uint8 [th,tw,3] or [th,tw,4] with th, tw >= 1")
    t = t.astype(np.uint32)
    return np.ascontiguousarray(t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16))


class TexturedMeshes(ColorMeshes):
    """A table of meshes ``[(vertices [P_i,3], faces [T_i,3], colors [P_i,3] uint8 or None, normals [P_i,3] or None, uv [P_i,2] or None,
    texture uint8 [th,tw,3 or 4] or None)]``.  Vertices, faces, colours and normals are ``ColorMeshes``'.  A mesh with a texture needs
    ``uv`` (float32 as the library reads it; finite or not: THE DEFINITION clamps, NaN becomes 0) and may go without colours, which are
    then zeros, as in the reference (opengl_render_backend.py:321); a mesh without a texture needs colours, and its ``uv``, if any,
    is kept but never read.  The texels are packed to one uint32 each and uploaded once per device."""

    def __init__(self, meshes):
        meshes = [tuple(m) for m in meshes]
        if any(len(m) != 6 for m in meshes):
            raise ValueError("TexturedMeshes takes (vertices, faces, colors or None, normals or None, uv or None, texture or None) per mesh")
        plain, uvs, texels, toff, th, tw = [], [], [], [0], [], []
        for k, (v, f, c, n, uv, tex) in enumerate(meshes):
            P = int(np.asarray(v).shape[0]) if np.asarray(v).ndim == 2 else 0
            if tex is None:
                if c is None:
                    raise ValueError(f"mesh {k}: a mesh without a texture needs colors")
                packed = np.zeros((0, 0), np.uint32)
            else:
                if uv is None:
                    raise ValueError(f"mesh {k}: a mesh with a texture needs uv [{P},2]")
                try:
                    packed = pack_texels(tex)
                except ValueError as e:
                    raise ValueError(f"mesh {k}: {e}") from None
                if max(packed.shape) > TEXTURE_MAX_SIDE:
                    raise ValueError(f"mesh {k}: a texture has at most {TEXTURE_MAX_SIDE} texels along a side")
                if c is None:
                    c = np.zeros((P, 3), np.uint8)
            if uv is None:
                uv = np.zeros((P, 2), np.float32)
            else:
                uv = np.asarray(uv)
                if uv.shape != (P, 2) or not (np.issubdtype(uv.dtype, np.floating) or np.issubdtype(uv.dtype, np.integer)):
                    raise ValueError(f"mesh {k}: uv must be numbers [{P},2]")
            plain.append((v, f, c, n))
            with np.errstate(over="ignore"):
                uvs.append(uv.astype(np.float32))
            texels.append(packed.reshape(-1))
            th.append(packed.shape[0])
            tw.append(packed.shape[1])
            toff.append(toff[-1] + packed.size)
        if toff[-1] >= 1 << 31:
            raise ValueError("the textures of one table must hold fewer than 2^31 texels")
        super().__init__(plain)
        self.uv = np.ascontiguousarray(np.concatenate(uvs, 0))
        self.texels = np.ascontiguousarray(np.concatenate(texels))
        self.tex_offset, self.tex_h, self.tex_w = np.asarray(toff, np.int64), np.asarray(th, np.int32), np.asarray(tw, np.int32)
        self._c_toff = (C.c_int64 * len(toff))(*toff)
        self._c_th = (C.c_int32 * len(th))(*th)
        self._c_tw = (C.c_int32 * len(tw))(*tw)
        self._texture_device = {}

    def mesh(self, k):
        """(vertices, faces, colors, normals, uv, texture uint8 [th,tw,3] or None) of mesh k, as the table holds them"""
        v0, v1 = self.vertex_offset[k], self.vertex_offset[k + 1]
        tex = None
        if self.tex_h[k]:
            words = self.texels[self.tex_offset[k]:self.tex_offset[k + 1]].reshape(self.tex_h[k], self.tex_w[k])
            tex = np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255], -1).astype(np.uint8)
        return super().mesh(k) + (self.uv[v0:v1], tex)

    def textures_on(self, dev):
        """(uv, texels) on ``dev``, uploaded on first use; the texels as int32 words (torch has no uint32 arithmetic to offer, and
        needs none: the library reads the bits)"""
        dev = torch.device(dev)
        if dev not in self._texture_device:
            words = self.texels.view(np.int32) if self.texels.size else np.zeros(1, np.int32)   # (an address even for no texel)
            self._texture_device[dev] = (torch.from_numpy(self.uv).to(dev), torch.from_numpy(words).to(dev))
        return self._texture_device[dev]


def texture_workspace_bytes(q, b, h, w, meshes=None):
    """bytes of workspace for q instances composed into b images of h x w pixels: ``shade.shade_workspace_bytes``'s"""
    return _mesh.workspace_bytes("texture", q, b, h, w, meshes)


def render_textured(meshes, mesh_ids, labels, poses, K, h, w, ambient=0.5, shading="flat", filter="nearest", background=None,  # noqa: A002
                    far=math.inf, out_rgb=None, out_depth=None, out_labels=None, workspace=None, return_visible=False,
                    return_status=False, max_instances=TEXTURE_MAX_INSTANCES):
    """m instances per image, textured or vertex-coloured, shaded and composed through a z-buffer over a background.

    :param meshes:   ``TexturedMeshes``
    :param filter:   "nearest" (what the reference is believed to get from its OpenGL binding's default) or "bilinear"; both clamp to
                     the edge, there are no mip levels
    :param workspace: None or a uint8 CUDA tensor of ``texture_workspace_bytes(b * m, b, h, w, meshes)`` bytes, 16-byte aligned
    Every other parameter, and the return value, as ``shade.render_color``:
    ``(rgb [b,h,w,3] uint8, depth [b,h,w] float32, labels [b,h,w] uint8[, visible [b,m] int32][, status [b,m] int32])``.
    """
    def extra(dev):
        uv, texels = meshes.textures_on(dev)
        return _ptr(uv), _ptr(texels), meshes._c_toff, meshes._c_th, meshes._c_tw, FILTER[filter]

    return _mesh.render_shaded(_TEXTURE, meshes, mesh_ids, labels, poses, K, h, w, ambient=ambient, shading=shading, background=background,
                               far=far, out_rgb=out_rgb, out_depth=out_depth, out_labels=out_labels, workspace=workspace,
                               return_visible=return_visible, return_status=return_status, max_instances=max_instances,
                               choice=("filter", filter, FILTER), extra=extra)


_TEXTURE = _mesh.Front("texture", TexturedMeshes, TEXTURE_MAX_INSTANCES, "pvnet_render_textured")

_UV_SPELLINGS = (("texture_u", "texture_v"), ("u", "v"), ("s", "t"))


def read_textured_ply(path):
    """``shade.read_ply``'s result plus ``"uv": [P,2] float32 or None``: the per-vertex texture coordinates, read from the vertex
    properties ``texture_u texture_v`` (what the reference's ``OpenGLRenderer.load_ply`` reads) or, failing those, ``u v`` or ``s t``.
    The texture image itself is a file of its own; load it with any image reader and hand it to ``TexturedMeshes`` as it was loaded.
    OBJ files, and PLY files whose faces carry per-corner ``texcoord`` lists or ``vt`` indices, are out of scope: one vertex, one uv."""
    out, cols = parse_ply(path)
    out["uv"] = None
    for names in _UV_SPELLINGS:
        uv = cols(names, np.float32)
        if uv is not None:
            out["uv"] = uv
            break
    return out
