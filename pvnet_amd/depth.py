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

import math

import numpy as np
import torch

from . import _mesh
from ._abi import DEPTH_MAX_INSTANCES, DEPTH_S_BADFACE, DEPTH_S_BEHIND, DEPTH_S_NONFINITE  # noqa: F401
from .render import DeviceMeshes

_DEPTH = _mesh.Front("depth", DeviceMeshes, DEPTH_MAX_INSTANCES, "pvnet_render_depth")


def depth_workspace_bytes(q, b, h, w, meshes=None):
    """bytes of workspace for q instances composed into b images of h x w pixels"""
    return _mesh.workspace_bytes("depth", q, b, h, w, meshes)


def _render(meshes, mesh_ids, labels, poses, K, h, w, far, out_depth, out_labels, workspace, return_visible, return_status):
    """the checks and the calls of every function here; ``out_depth`` / ``out_labels``: ``(the caller's or None, its name)``, or None
    for an image that is not written"""
    mesh_ids, labels, poses, h, w, far = _mesh.check_scene(DeviceMeshes, meshes, mesh_ids, labels, poses, h, w, far, DEPTH_MAX_INSTANCES)
    shape, dev = (int(poses.shape[0]), h, w), poses.device
    depth = _mesh.check_out(out_depth[0], shape, torch.float32, dev, out_depth[1]) if out_depth else None
    label = _mesh.check_out(out_labels[0], shape, torch.uint8, dev, out_labels[1]) if out_labels else None
    return _mesh.compose(_DEPTH, meshes, mesh_ids, labels, poses, K, h, w, far, DEPTH_MAX_INSTANCES,
                         lambda i0: (_mesh.at(depth, i0), _mesh.at(label, i0)), tuple(t for t in (depth, label) if t is not None),
                         return_visible, return_status, workspace)


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
    return _render(meshes, mesh_ids, labels, poses, K, h, w, far, (out_depth, "out_depth"), (out_labels, "out_labels"), workspace,
                   return_visible, return_status)


def render_visible_labels(meshes, mesh_ids, labels, poses, K, h, w, far=math.inf, out=None, workspace=None, return_visible=False,
                          return_status=False):
    """The labels of ``render_depth`` alone (no depth image is written): the occlusion-correct counterpart of ``render.render_labels``.

    :return: ``labels [b,h,w]`` uint8; with ``return_visible`` / ``return_status`` a tuple with ``[b,m]`` int32 of each behind it"""
    res = _render(meshes, mesh_ids, labels, poses, K, h, w, far, None, (out, "out"), workspace, return_visible, return_status)
    return res if return_visible or return_status else res[0]


def render_mesh_depth(RT, K, vert, face, h, w):
    """The reference's call form (lib/utils/extend_utils/extend_utils.py:196-213): numpy pose ``[3,4]``, ``K [3,3]``, vertices ``[P,3]``
    and faces ``[T,3]`` in, numpy float32 ``[h,w]`` out (0 where the mesh does not cover), computed on the current device.  The
    reference's ``init`` flag belongs to its OpenGL context and is not taken."""
    RT, K = np.asarray(RT, np.float64), np.asarray(K, np.float64)
    assert RT.shape == (3, 4) and K.shape == (3, 3)
    table = DeviceMeshes([(vert, face)])
    poses = torch.from_numpy(np.ascontiguousarray(RT)).to("cuda").view(1, 1, 3, 4)
    depth, = _render(table, [0], [1], poses, K, h, w, math.inf, (None, "out_depth"), None, None, False, False)   # the depth image alone
    return depth[0].cpu().numpy()
