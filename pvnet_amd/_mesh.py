"""What the front ends of the four mesh renderers share (render.py, depth.py, shade.py, texture.py): the float64 upload, the checks of
meshes, poses, camera, outputs and the instance list, the split of a batch into library calls, the workspace formula, the head of
arguments every ``pvnet_render*`` entry point opens with, the one loop the three z-buffer renderers call their library through, and the
body of the two that colour.  Private: the public names stay in the four modules."""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np
import torch

from ._abi import SHADE_FLAT, SHADE_NONE, SHADE_PHONG, _check, _load_side
from ._marshal import nbytes, ptr, stream, workspace as checked_workspace

SHADING = {"none": SHADE_NONE, "flat": SHADE_FLAT, "phong": SHADE_PHONG}   # (_abi: the texture library's codes are the same)

# what tells the z-buffer renderers apart: the library (a row of _abi.SIDE_LIBRARIES), the table it takes, its limit, its entry point
Front = collections.namedtuple("Front", "side kind limit entry")


def device_f64(x, dev, what):
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float64:
            raise RuntimeError(f"{what} must be float64")
        return x.to(dev).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64))).to(dev)


def check_meshes(meshes, kind):
    if not isinstance(meshes, kind):
        raise RuntimeError(f"meshes must be a {kind.__name__}")


def check_poses(poses, dims):
    if not (isinstance(poses, torch.Tensor) and poses.is_cuda):
        raise RuntimeError("poses must be a CUDA tensor (there is no CPU fallback)")
    if poses.dtype != torch.float64 or poses.dim() != dims or tuple(poses.shape[-2:]) != (3, 4):
        raise RuntimeError(f"poses must be float64 [{'b,m' if dims == 4 else 'n'},3,4], got {poses.dtype} {tuple(poses.shape)}")
    return poses.contiguous()


def check_camera(K, dev, lead):
    """-> (K on the device, per instance?) for K [3,3] or [*lead,3,3]"""
    K = device_f64(K, dev, "K")
    if tuple(K.shape) == (3, 3):
        return K, False
    if tuple(K.shape) == tuple(lead) + (3, 3):
        return K.reshape(-1, 3, 3), True
    raise RuntimeError(f"K must be [3,3] or {tuple(lead) + (3, 3)}, got {tuple(K.shape)}")


def check_out(out, shape, dtype, dev, what, spelled=None):
    """a new tensor, or the caller's ``what`` where it is one of that shape and dtype (``spelled`` in the refusal, where not as torch
    spells it) on that device"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == dtype and
            tuple(out.shape) == tuple(shape) and out.is_contiguous()):
        raise RuntimeError(f"{what} must be a contiguous {spelled or dtype} CUDA tensor of shape {tuple(shape)} on {dev}")
    return out


def check_instances(meshes, mesh_ids, labels, m, h, w, limit):
    """the instance list of a composed image -> (mesh_ids, labels) as lists of int"""
    mesh_ids, labels = [int(x) for x in mesh_ids], [int(x) for x in labels]
    if len(mesh_ids) != m or len(labels) != m or any(not 0 <= x < meshes.count for x in mesh_ids):
        raise RuntimeError(f"mesh_ids and labels must have m={m} entries, mesh ids in 0 .. {meshes.count - 1}")
    if any(not 1 <= x <= 255 for x in labels):
        raise RuntimeError("labels must lie in 1 .. 255")
    if h < 2 or w < 2:
        raise RuntimeError("h and w must be at least 2")
    if m > limit:
        raise RuntimeError(f"at most {limit} instances per image")
    return mesh_ids, labels


def check_scene(kind, meshes, mesh_ids, labels, poses, h, w, far, limit):
    """what every z-buffer call checks first -> (mesh_ids, labels, poses, h, w, far)"""
    check_meshes(meshes, kind)
    poses = check_poses(poses, 4)
    h, w, far = int(h), int(w), float(far)
    mesh_ids, labels = check_instances(meshes, mesh_ids, labels, int(poses.shape[1]), h, w, limit)
    if math.isnan(far) or not float(np.float32(far)) > 0:
        raise RuntimeError("far must be a positive float32 (not NaN)")
    return mesh_ids, labels, poses, h, w, far


def image_stretches(b, m, limit):
    """(first image, end) of every stretch of whole images with at most ``limit`` instances, m per image: one library call each"""
    images = max(1, limit // m) if m else max(b, 1)
    return [(i0, min(b, i0 + images)) for i0 in range(0, b, images)]


def workspace_bytes(side, q, b, h, w, meshes=None, told=None):
    """bytes of workspace library ``side`` wants for q instances composed into b images of h x w pixels"""
    P, T = (meshes.total_vertices, meshes.total_faces) if meshes is not None else (0, 0)
    n = int(getattr(_load_side(side), f"pvnet_{side}_workspace_bytes")(int(q), P, T, int(b), int(h), int(w)))
    if n == 0:
        told = told or f"q={q}, b={b}, h={h}, w={w}"
        raise RuntimeError(f"{side}_workspace_bytes: arguments out of range ({told}; h, w >= 2)")
    return n


def at(t, i):
    """the address of ``t[i]``; None stays None"""
    return None if t is None else ptr(t[i:])


def argument_head(meshes, dev, mesh_ids, poses, K, per, image_ids, labels, *sizes):
    """The arguments every ``pvnet_render*`` entry point opens with: the mesh table, n, the mesh ids, ``poses`` and ``K`` (each from the
    call's first instance on), the per-instance flag, the image ids (from the call's first image) and the labels -- fourteen, behind
    which pvnet_render has its own; the z-buffer entry points go on with ``sizes``: b, h, w, far -- eighteen."""
    n = len(mesh_ids)
    arr = lambda vals: (C.c_int32 * max(n, 1))(*vals)   # noqa: E731
    return meshes.table_arguments(dev) + (n, arr(mesh_ids), ptr(poses) if n else None, ptr(K), 1 if per else 0, arr(image_ids),
                                          arr(labels)) + sizes


def stretch_heads(meshes, mesh_ids, labels, poses, K, per, h, w, far, limit):
    """per stretch of ``image_stretches``: (its first image, its first instance, its images, ``argument_head`` through ``far``);
    ``poses`` [b,m,3,4], ``K`` and ``per`` as ``check_camera`` gives them"""
    m, flat = int(poses.shape[1]), poses.view(-1, 3, 4)
    for i0, i1 in image_stretches(int(poses.shape[0]), m, limit):
        nb, s = i1 - i0, i0 * m
        yield i0, s, nb, argument_head(meshes, poses.device, mesh_ids * nb, flat[s:], K[s:] if per else K, per,
                                       [i for i in range(nb) for _ in range(m)], labels * nb, nb, h, w, far)


def compose(front, meshes, mesh_ids, labels, poses, K, h, w, far, limit, own, images, return_visible, return_status, workspace):
    """One call of ``front``'s entry point per stretch of whole images with at most ``limit`` instances (none for no image): the head,
    ``own(first image)`` -- the call's arguments between ``far`` and ``visible_out``, its outputs last --, the counts, the workspace,
    the stream.  -> ``images`` followed by ``visible`` and ``status`` [b,m] int32, each where asked for."""
    dev, b, m = poses.device, int(poses.shape[0]), int(poses.shape[1])
    visible, status = (torch.empty(b * m, dtype=torch.int32, device=dev) if asked else None for asked in (return_visible, return_status))
    if b:
        entry = getattr(_load_side(front.side), front.entry)
        Kd, per = check_camera(K, dev, (b, m))
        with torch.cuda.device(dev):
            for i0, s, nb, head in stretch_heads(meshes, mesh_ids, labels, poses, Kd, per, h, w, far, limit):
                ws = checked_workspace(workspace, workspace_bytes(front.side, nb * m, nb, h, w, meshes), dev, align=16, sized=True)
                _check(entry(*head, *own(i0), at(visible, s) if m else None, at(status, s) if m else None, ptr(ws), nbytes(ws),
                             stream(dev)), front.entry)
    return images + tuple(t.view(b, m) for t in (visible, status) if t is not None)


def render_shaded(front, meshes, mesh_ids, labels, poses, K, h, w, *, ambient, shading, background, far, out_rgb, out_depth, out_labels,
                  workspace, return_visible, return_status, max_instances, choice=None, extra=None):
    """The body of ``shade.render_color`` and of ``texture.render_textured``.  ``choice``: ``(name, value, allowed)`` of one more argument
    that must be a key of ``allowed``, checked after ``shading``; ``extra(dev)``: the arguments the library takes between the normals
    and the shading, as a tuple."""
    check_meshes(meshes, front.kind)
    max_instances = int(max_instances)
    if not 1 <= max_instances <= front.limit:
        raise RuntimeError(f"max_instances must lie in 1 .. {front.limit}")
    mesh_ids, labels, poses, h, w, far = check_scene(front.kind, meshes, mesh_ids, labels, poses, h, w, far, max_instances)
    if shading not in SHADING:
        raise RuntimeError(f"shading must be one of {sorted(SHADING)}")
    if choice is not None and choice[1] not in choice[2]:
        raise RuntimeError(f"{choice[0]} must be one of {sorted(choice[2])}")
    ambient = float(ambient)
    if not (math.isfinite(ambient) and ambient >= 0):
        raise RuntimeError("ambient must be finite and >= 0")
    dev, b = poses.device, int(poses.shape[0])
    bg_image, bg_color = None, (0, 0, 0)
    if isinstance(background, torch.Tensor):
        bg_image = check_out(background, (b, h, w, 3), torch.uint8, dev, "background")
    elif background is not None:
        bg_color = tuple(int(x) for x in background)
        if len(bg_color) != 3 or any(not 0 <= x <= 255 for x in bg_color):
            raise RuntimeError("background must be a colour triple in 0 .. 255 or a uint8 CUDA tensor [b,h,w,3]")
    rgb = check_out(out_rgb, (b, h, w, 3), torch.uint8, dev, "out_rgb")
    depth = check_out(out_depth, (b, h, w), torch.float32, dev, "out_depth")
    label = check_out(out_labels, (b, h, w), torch.uint8, dev, "out_labels")
    c_bg = (C.c_uint8 * 3)(*bg_color)
    # (a table goes to the device on first use; the order is kept as it was measured -- the textures, K and the geometry in
    # ``compose``, the colours -- see profiles/mesh_front_probe.txt)
    between = extra(dev) if b and extra is not None else ()

    def own(i0):
        colors, normals = meshes.shading_on(dev)
        return (ptr(colors), ptr(normals) if shading == "phong" else None) + between + (
            SHADING[shading], ambient, c_bg, at(bg_image, i0), at(rgb, i0), at(depth, i0), at(label, i0))

    return compose(front, meshes, mesh_ids, labels, poses, K, h, w, far, max_instances, own, (rgb, depth, label), return_visible,
                   return_status, workspace)
