"""Colour images of posed meshes on the device: a shaded vertex-colour renderer over a background, the step from a pose to a training
image.

The reference trains on rendered and fused images it makes offline with an OpenGL / Blender renderer
(lib/utils/opengl_render_backend.py:19-102, 203-264, 306-399): vertex colours, one light at the camera, an ambient weight, flat or Phong
shading.  Here:

* ``ColorMeshes``           -- ``render.DeviceMeshes`` with vertex colours and normals (given, or computed on the host);
* ``render_color``          -- m instances per image -> ``rgb [b,h,w,3]`` uint8 over a background colour or image, with the depth,
                               occlusion-correct labels, visible counts and status of ``depth.render_depth`` from the same call; ``rgb``
                               and the labels are what ``augment.augment_batch`` takes;
* ``shade_workspace_bytes``;
* ``read_ply``              -- a small reader of ASCII and binary_little_endian PLY files (vertex positions, optional normals and
                               colours, triangular faces): what ``LineModModelDB.get_ply_mesh`` reads with the ``plyfile`` package.

pvnet_amd/csrc/shade.hip, libpvnet_shade.so; C ABI and THE DEFINITION: include/pvnet_shade.h; a numpy restatement:
tests/shade_restatement.py.  Textured meshes: pvnet_amd/texture.py, a library of its own.  Poses are float64 ``[b,m,3,4]`` (``pnp_batch_device``'s output is read in place).

Everything is enqueued on the current stream without synchronising; with caller-owned outputs and ``workspace`` a call is capturable
in a graph.  PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _mesh
from ._abi import (SHADE_FLAT, SHADE_MAX_FACES, SHADE_MAX_INSTANCES, SHADE_NONE, SHADE_PHONG, SHADE_S_BADFACE,  # noqa: F401
                   SHADE_S_BEHIND, SHADE_S_NONFINITE)
from ._mesh import SHADING   # noqa: F401 (this module's name for it)
from .render import DeviceMeshes


def vertex_normals(vertices, faces):
    """per vertex the normalised weighted sum of the normals of the faces that name it, every face weighted by its area over the squared
    lengths of its two edges at that vertex (N. Max, "Weights for computing vertex normals from facet normals", 1999): exact for the
    vertices of a mesh inscribed in a sphere, which the plain area-weighted sum misses by up to 0.020 on ``icosphere(2)``.  (0, 0, 0)
    where that sum vanishes; a face with an edge of no length adds nothing."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = np.zeros_like(v)
    for k in range(3):
        apex = f[:, k]
        e1, e2 = v[f[:, (k + 1) % 3]] - v[apex], v[f[:, (k + 2) % 3]] - v[apex]
        den = (e1 * e1).sum(1) * (e2 * e2).sum(1)
        c = np.cross(e1, e2)   # its length is twice the face's area
        np.add.at(n, apex, np.where(den[:, None] > 0, c / np.where(den > 0, den, 1.0)[:, None], 0.0))
    length = np.sqrt((n * n).sum(1))
    return np.where(length[:, None] > 0, n / np.where(length > 0, length, 1.0)[:, None], 0.0)


class ColorMeshes(DeviceMeshes):
    """A table of coloured meshes ``[(vertices [P_i,3], faces [T_i,3], colors [P_i,3] uint8[, normals [P_i,3]])]``.  Vertices and
    faces are validated as ``DeviceMeshes`` validates them; colours must be uint8 (or integers in 0 .. 255); normals are taken as
    given (finite, any length) or, when absent or None, computed here (``vertex_normals``: sphere-exact weights).  Uploaded once per device."""

    def __init__(self, meshes):
        meshes = [tuple(m) for m in meshes]
        if any(len(m) not in (3, 4) for m in meshes):
            raise ValueError("ColorMeshes takes (vertices, faces, colors) or (vertices, faces, colors, normals) per mesh")
        super().__init__([(m[0], m[1]) for m in meshes])
        cs, ns = [], []
        for k, m in enumerate(meshes):
            P = int(self.vertex_offset[k + 1] - self.vertex_offset[k])
            c = np.asarray(m[2])
            if c.shape != (P, 3) or not (c.dtype == np.uint8 or np.issubdtype(c.dtype, np.integer)):
                raise ValueError(f"mesh {k}: colors must be uint8 [{P},3]")
            if c.size and (int(c.min()) < 0 or int(c.max()) > 255):
                raise ValueError(f"mesh {k}: colors must lie in 0 .. 255")
            if self.face_count(k) > SHADE_MAX_FACES:
                raise ValueError(f"mesh {k}: at most {SHADE_MAX_FACES} faces")
            if len(m) == 4 and m[3] is not None:
                n = np.asarray(m[3], np.float64)
                if n.shape != (P, 3) or not np.isfinite(n).all():
                    raise ValueError(f"mesh {k}: normals must be finite [{P},3]")
            else:
                n = vertex_normals(m[0], m[1])
            cs.append(c.astype(np.uint8))
            ns.append(n)
        self.colors = np.ascontiguousarray(np.concatenate(cs, 0))
        self.normals = np.ascontiguousarray(np.concatenate(ns, 0))
        self._shade_device = {}

    def mesh(self, k):
        """(vertices, faces, colors, normals) of mesh k, as the table holds them"""
        v0, v1, f0, f1 = self.vertex_offset[k], self.vertex_offset[k + 1], self.face_offset[k], self.face_offset[k + 1]
        return self.vertices[v0:v1], self.faces[f0:f1], self.colors[v0:v1], self.normals[v0:v1]

    def shading_on(self, dev):
        """(colors, normals) on ``dev``, uploaded on first use"""
        dev = torch.device(dev)
        if dev not in self._shade_device:
            self._shade_device[dev] = (torch.from_numpy(self.colors).to(dev), torch.from_numpy(self.normals).to(dev))
        return self._shade_device[dev]


def shade_workspace_bytes(q, b, h, w, meshes=None):
    """bytes of workspace for q instances composed into b images of h x w pixels"""
    return _mesh.workspace_bytes("shade", q, b, h, w, meshes)


def render_color(meshes, mesh_ids, labels, poses, K, h, w, ambient=0.5, shading="flat", background=None, far=math.inf, out_rgb=None,
                 out_depth=None, out_labels=None, workspace=None, return_visible=False, return_status=False,
                 max_instances=SHADE_MAX_INSTANCES):
    """m instances per image, shaded and composed through a z-buffer over a background.

    :param meshes:   ``ColorMeshes``
    :param mesh_ids: [m] mesh per instance;  :param labels: [m] label per instance, 1 .. 255
    :param poses:    [b,m,3,4] float64 CUDA tensor
    :param K:        [3,3] shared or [b,m,3,3], float64 (CUDA tensor, or numpy: uploaded here)
    :param ambient:  the ambient weight, finite and >= 0 (the reference's ``ambient_weight``, 0.5 there)
    :param shading:  "flat" (the face normal), "phong" (the interpolated vertex normals) or "none" (the interpolated colour alone)
    :param background: None (black), a colour triple in 0 .. 255, or a contiguous uint8 CUDA tensor [b,h,w,3]
    :param far:      float32 > 0: only depths below it are kept, as in ``depth.render_depth``
    :param out_rgb, out_depth, out_labels: None or contiguous CUDA tensors [b,h,w,3] uint8 / [b,h,w] float32 / [b,h,w] uint8;
                     every element is overwritten
    :param workspace: None or a uint8 CUDA tensor of ``shade_workspace_bytes(b * m, b, h, w, meshes)`` bytes, 16-byte aligned
    :param max_instances: instances per library call, at most ``SHADE_MAX_INSTANCES``: a larger batch is split between images
    :return: ``(rgb [b,h,w,3] uint8, depth [b,h,w] float32, labels [b,h,w] uint8[, visible [b,m] int32][, status [b,m] int32])``;
             depth, labels, visible and status are ``depth.render_depth``'s
    """
    return _mesh.render_shaded(_SHADE, meshes, mesh_ids, labels, poses, K, h, w, ambient=ambient, shading=shading, background=background,
                               far=far, out_rgb=out_rgb, out_depth=out_depth, out_labels=out_labels, workspace=workspace,
                               return_visible=return_visible, return_status=return_status, max_instances=max_instances)


_SHADE = _mesh.Front("shade", ColorMeshes, SHADE_MAX_INSTANCES, "pvnet_render_color")


# ---- PLY -------------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """An ASCII or binary_little_endian PLY file -> ``{"vertices": [P,3] float64, "faces": [T,3] int32, "normals": [P,3] float64 or
    None, "colors": [P,3] uint8 or None}``.  Reads the vertex properties ``x y z``, ``nx ny nz`` and ``red green blue`` (others are
    skipped) and the face element's list property (``vertex_indices`` / ``vertex_index``), whose lists must all have three entries."""
    return parse_ply(path)[0]


def parse_ply(path):
    """(what ``read_ply`` returns, ``cols``: (property names, dtype) -> those vertex properties as columns, or None when one is missing):
    the parser behind ``read_ply`` and ``texture.read_textured_ply``"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.find(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok or tok[0] in ("ply", "comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property" and elements:
            if tok[1] == "list":
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: format {fmt!r} is not read (ascii and binary_little_endian are)")
    tables = {}
    words = data[body:].split() if fmt == "ascii" else None
    pos = 0 if fmt == "ascii" else body
    for name, count, props in elements:
        lists = [p for p in props if p[2] is not None]
        if lists and (len(props) != 1 or name != "face"):
            raise ValueError(f"{path}: element {name!r}: a list property is read only as the face element's single property")
        if lists:
            _, ctype, itype = props[0]
            if fmt == "ascii":
                raw = np.asarray(words[pos:pos + 4 * count], np.float64).reshape(count, 4) if count else np.zeros((0, 4))
                if len(raw) != count or (count and (raw[:, 0] != 3).any()):
                    raise ValueError(f"{path}: every face must have three vertices")
                pos += 4 * count
                tables[name] = raw[:, 1:].astype(np.int32)
            else:
                rec = np.dtype([("n", "<" + ctype), ("v", "<" + itype, (3,))])
                raw = np.frombuffer(data, rec, count, pos)
                if count and (raw["n"] != 3).any():
                    raise ValueError(f"{path}: every face must have three vertices")
                pos += rec.itemsize * count
                tables[name] = raw["v"].astype(np.int32)
        elif fmt == "ascii":
            raw = np.asarray(words[pos:pos + len(props) * count], np.float64).reshape(count, len(props))
            pos += len(props) * count
            tables[name] = {p[0]: raw[:, k] for k, p in enumerate(props)}
        else:
            rec = np.dtype([(p[0], "<" + p[1]) for p in props])
            raw = np.frombuffer(data, rec, count, pos)
            pos += rec.itemsize * count
            tables[name] = {p[0]: raw[p[0]] for p in props}
    vert = tables.get("vertex")
    if not isinstance(vert, dict) or not all(k in vert for k in "xyz"):
        raise ValueError(f"{path}: no vertex element with x, y, z")

    def cols(names, dtype):
        return np.ascontiguousarray(np.stack([vert[k] for k in names], 1).astype(dtype)) if all(k in vert for k in names) else None

    faces = tables.get("face")
    return {"vertices": cols("xyz", np.float64), "faces": faces if faces is not None else np.zeros((0, 3), np.int32),
            "normals": cols(("nx", "ny", "nz"), np.float64), "colors": cols(("red", "green", "blue"), np.uint8)}, cols
