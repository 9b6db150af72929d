"""Depth images, occlusion-correct label images and visible pixel counts of posed meshes on the device: a z-buffered mesh renderer.

The reference makes Occlusion LINEMOD's label images from depth (``OcclusionLineModDB.get_mask_of_all_objects``,
lib/utils/data_utils.py:788-826): per pixel the label of the object with the smallest depth, the depth map starting at 10, the earlier
object winning a tie.  ``render.render_labels`` composes in painter's order instead, which no order makes equal to that for instances that
interpenetrate or wrap around each other.  Here:

* ``render_depth``          -- m instances per image -> depth ``[b,h,w]`` float32 and labels ``[b,h,w]`` uint8, optionally the pixels
                               each instance wins (its visible area: the occlusion ratio's numerator) and its status bits;
* ``render_visible_labels`` -- the labels only: the occlusion-correct counterpart of ``render.render_labels``;
* ``render_mesh_depth``     -- the reference's call form (lib/utils/extend_utils/extend_utils.py:196-213, which has no native body
                               there): numpy in, numpy float32 ``[h,w]`` out;
* ``depth_workspace_bytes``.

pvnet_amd/csrc/depth.hip, libpvnet_depth.so; C ABI and THE DEFINITION: include/pvnet_depth.h; a numpy restatement:
tests/depth_restatement.py.  The mesh table is ``render.DeviceMeshes``; poses are float64 ``[b,m,3,4]`` (``pnp_batch_device``'s output
is read in place).

Everything is enqueued on the current stream without synchronising; with caller-owned outputs and ``workspace`` a call is capturable
in a graph.  PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from ._abi import (DEPTH_MAX_INSTANCES, DEPTH_S_BADFACE, DEPTH_S_BEHIND, DEPTH_S_NONFINITE, _check,  # noqa: F401
                   load_depth_library)
from ._marshal import nbytes as _nbytes, ptr as _ptr, stream as _stream, workspace as _workspace
from .render import DeviceMeshes, _camera, _poses


def depth_workspace_bytes(q, b, h, w, meshes=None):
    """bytes of workspace for q instances composed into b images of h x w pixels"""
    P, T = (meshes.total_vertices, meshes.total_faces) if meshes is not None else (0, 0)
    n = int(load_depth_library().pvnet_depth_workspace_bytes(int(q), P, T, int(b), int(h), int(w)))
    if n == 0:
        raise RuntimeError(f"depth_workspace_bytes: arguments out of range (q={q}, b={b}, h={h}, w={w}; h, w >= 2)")
    return n


def _out(out, shape, dtype, dev, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == dtype and
            tuple(out.shape) == tuple(shape) and out.is_contiguous()):
        raise RuntimeError(f"{what} must be a contiguous {dtype} CUDA tensor of shape {tuple(shape)} on {dev}")
    return out


def _image_stretches(b, m, limit):
    """(first image, end) of every stretch of whole images with at most ``limit`` instances, m per image: one library call each
    (``shade.render_color`` splits the same way)"""
    images = max(1, limit // m) if m else max(b, 1)
    return [(i0, min(b, i0 + images)) for i0 in range(0, b, images)]


def _render(meshes, mesh_ids, labels, poses, K, h, w, far, depth, label, visible, status, workspace):
    """one pvnet_render_depth call per stretch of whole images with at most DEPTH_MAX_INSTANCES instances; ``poses`` [b,m,3,4]"""
    lib = load_depth_library()
    dev = poses.device
    b, m = int(poses.shape[0]), int(poses.shape[1])
    Kd, per = _camera(K, dev, (b, m))
    vertices, faces, _ = meshes.on(dev)
    flat = poses.view(-1, 3, 4)
    with torch.cuda.device(dev):
        for i0, i1 in _image_stretches(b, m, DEPTH_MAX_INSTANCES):
            nb, n = i1 - i0, (i1 - i0) * m
            s = i0 * m
            ws = _workspace(workspace, depth_workspace_bytes(n, nb, h, w, meshes), dev, align=16, sized=True)
            arr = lambda vals: (C.c_int32 * max(n, 1))(*vals)   # noqa: E731
            _check(lib.pvnet_render_depth(
                _ptr(vertices), _ptr(faces), meshes._c_voff, meshes._c_foff, meshes.count, meshes.total_vertices, meshes.total_faces, n,
                arr(mesh_ids * nb), _ptr(flat[s:]) if n else None, _ptr(Kd[s:] if per else Kd), 1 if per else 0,
                arr([i for i in range(nb) for _ in range(m)]), arr(labels * nb), nb, h, w, far,
                _ptr(depth[i0:]) if depth is not None else None, _ptr(label[i0:]) if label is not None else None,
                _ptr(visible[s:]) if visible is not None and n else None, _ptr(status[s:]) if status is not None and n else None,
                _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_render_depth")


def _checked(meshes, mesh_ids, labels, poses, h, w, far, limit=DEPTH_MAX_INSTANCES):
    if not isinstance(meshes, DeviceMeshes):
        raise RuntimeError("meshes must be a DeviceMeshes")
    dev = poses.device if isinstance(poses, torch.Tensor) else None
    poses = _poses(poses, dev, 4)
    m, h, w, far = int(poses.shape[1]), int(h), int(w), float(far)
    mesh_ids, labels = [int(x) for x in mesh_ids], [int(x) for x in labels]
    if len(mesh_ids) != m or len(labels) != m or any(not 0 <= x < meshes.count for x in mesh_ids):
        raise RuntimeError(f"mesh_ids and labels must have m={m} entries, mesh ids in 0 .. {meshes.count - 1}")
    if any(not 1 <= x <= 255 for x in labels):
        raise RuntimeError("labels must lie in 1 .. 255")
    if h < 2 or w < 2:
        raise RuntimeError("h and w must be at least 2")
    if m > limit:
        raise RuntimeError(f"at most {limit} instances per image")
    if math.isnan(far) or not float(np.float32(far)) > 0:
        raise RuntimeError("far must be a positive float32 (not NaN)")
    return mesh_ids, labels, poses, h, w, far


def render_depth(meshes, mesh_ids, labels, poses, K, h, w, far=math.inf, out_depth=None, out_labels=None, workspace=None,
                 return_visible=False, return_status=False):
    """m instances per image through a z-buffer: a pixel takes the smallest depth below ``far`` over all triangles of all instances of
    its image, and the label of the instance that gave it; at equal float32 depth the instance earlier in the list wins.

    :param meshes:   ``render.DeviceMeshes``
    :param mesh_ids: [m] mesh per instance;  :param labels: [m] label per instance, 1 .. 255
    :param poses:    [b,m,3,4] float64 CUDA tensor
    :param K:        [3,3] shared or [b,m,3,3], float64 (CUDA tensor, or numpy: uploaded here)
    :param far:      float32 > 0: only depths below it are kept (10 reproduces the reference's ``get_mask_of_all_objects``)
    :param out_depth, out_labels: None or contiguous CUDA tensors [b,h,w], float32 / uint8; every element is overwritten
    :param workspace: None or a uint8 CUDA tensor of ``depth_workspace_bytes(b * m, b, h, w, meshes)`` bytes, 16-byte aligned
    :return: ``(depth [b,h,w] float32, labels [b,h,w] uint8[, visible [b,m] int32][, status [b,m] int32])``: depth 0 and label 0 where
             nothing is kept; ``visible`` the pixels each instance wins; ``status`` its ``DEPTH_S_*`` bits
    """
    mesh_ids, labels, poses, h, w, far = _checked(meshes, mesh_ids, labels, poses, h, w, far)
    dev, b, m = poses.device, int(poses.shape[0]), int(poses.shape[1])
    depth = _out(out_depth, (b, h, w), torch.float32, dev, "out_depth")
    label = _out(out_labels, (b, h, w), torch.uint8, dev, "out_labels")
    visible = torch.empty(b * m, dtype=torch.int32, device=dev) if return_visible else None
    status = torch.empty(b * m, dtype=torch.int32, device=dev) if return_status else None
    if b:
        _render(meshes, mesh_ids, labels, poses, K, h, w, far, depth, label, visible, status, workspace)
    res = (depth, label)
    if return_visible:
        res += (visible.view(b, m),)
    if return_status:
        res += (status.view(b, m),)
    return res


def render_visible_labels(meshes, mesh_ids, labels, poses, K, h, w, far=math.inf, out=None, workspace=None, return_visible=False,
                          return_status=False):
    """The labels of ``render_depth`` alone (no depth image is written): the occlusion-correct counterpart of ``render.render_labels``.

    :return: ``labels [b,h,w]`` uint8; with ``return_visible`` / ``return_status`` a tuple with ``[b,m]`` int32 of each behind it"""
    mesh_ids, labels, poses, h, w, far = _checked(meshes, mesh_ids, labels, poses, h, w, far)
    dev, b, m = poses.device, int(poses.shape[0]), int(poses.shape[1])
    label = _out(out, (b, h, w), torch.uint8, dev, "out")
    visible = torch.empty(b * m, dtype=torch.int32, device=dev) if return_visible else None
    status = torch.empty(b * m, dtype=torch.int32, device=dev) if return_status else None
    if b:
        _render(meshes, mesh_ids, labels, poses, K, h, w, far, None, label, visible, status, workspace)
    if not (return_visible or return_status):
        return label
    return (label,) + ((visible.view(b, m),) if return_visible else ()) + ((status.view(b, m),) if return_status else ())


def render_mesh_depth(RT, K, vert, face, h, w):
    """The reference's call form (lib/utils/extend_utils/extend_utils.py:196-213): numpy pose ``[3,4]``, ``K [3,3]``, vertices ``[P,3]``
    and faces ``[T,3]`` in, numpy float32 ``[h,w]`` out (0 where the mesh does not cover), computed on the current device.  The
    reference's ``init`` flag belongs to its OpenGL context and is not taken."""
    RT, K = np.asarray(RT, np.float64), np.asarray(K, np.float64)
    assert RT.shape == (3, 4) and K.shape == (3, 3)
    table = DeviceMeshes([(vert, face)])
    poses = torch.from_numpy(np.ascontiguousarray(RT)).to("cuda").view(1, 1, 3, 4)
    mesh_ids, labels, poses, h, w, far = _checked(table, [0], [1], poses, h, w, math.inf)
    depth = torch.empty((1, h, w), dtype=torch.float32, device=poses.device)
    _render(table, mesh_ids, labels, poses, K, h, w, far, depth, None, None, None, None)   # the depth image alone
    return depth[0].cpu().numpy()
