"""Silhouettes and label images of posed meshes on the device: the way back from a pose to pixels.

The reference's helper library has ``mesh_binary_rasterization`` (lib/utils/extend_utils/src/mesh_rasterization.cpp:43-71, called
through extend_utils.py:7-20): the triangle-coverage mask of a projected mesh.  Here:

* ``DeviceMeshes``              -- a table of meshes, validated on the host, uploaded once per device;
* ``project_triangles``         -- stage P: pose and K -> the float32 triangles the reference's caller hands to its rasteriser;
* ``rasterize_triangles``       -- stage R: ``[n,tn,3,2]`` float32 triangles -> ``[n,h,w]`` uint8 masks, bit for bit the reference's;
* ``render_masks``              -- P + R: one instance per image, ``poses [n,3,4]`` float64 (``pnp_batch_device``'s output in place);
* ``render_labels``             -- P + R + C: several instances per image composed in painter's order into one label image;
* ``mesh_binary_rasterization`` -- the reference's Python-level call form, numpy in and out;
* ``raster_workspace_bytes``, and ``icosphere`` / ``box_mesh`` / ``l_prism_mesh``: small synthetic meshes for tests and probes.

pvnet_amd/csrc/raster.hip, libpvnet_raster.so; C ABI and THE DEFINITION (with its deviations where the reference's C is undefined):
include/pvnet_raster.h; a numpy restatement: tests/raster_restatement.py.  The masks are uint8, as ``ransac_voting_layer_v3`` / ``_v2``,
``vertex_targets_device``, ``HeadLoss.from_keypoints`` and ``augment_batch`` take them.

Everything is enqueued on the current stream without synchronising; with caller-owned ``out`` and ``workspace`` a call is capturable
in a graph.  PyTorch is plumbing only.  There is NO CPU fallback: without the library, or with CPU tensors, these raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _mesh
from ._abi import (RASTER_MAX_IMAGES, RASTER_MAX_INSTANCES, RASTER_MAX_MESHES, RASTER_S_BADFACE, RASTER_S_BEHIND,  # noqa: F401
                   RASTER_S_NONFINITE, _check, load_raster_library)
from ._marshal import nbytes as _nbytes, ptr as _ptr, stream as _stream, workspace as _workspace


# ---- small synthetic meshes (numpy; vertices float64 [P,3], faces int32 [T,3]) -------------------------------------------------------
def icosphere(subdivisions=0, radius=1.0):
    """the unit icosahedron, every triangle split in four ``subdivisions`` times, vertices pushed to the sphere: 20 * 4**s faces"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(int(subdivisions)):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float64) * float(radius), np.asarray(f, np.int32)


def box_mesh(sx=1.0, sy=1.0, sz=1.0):
    """an axis-aligned box centred at the origin with the given side lengths: 8 vertices, 12 faces"""
    v = np.array([(x, y, z) for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float64) * (sx, sy, sz)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v, np.asarray(f, np.int32)


def l_prism_mesh(size=1.0, depth=0.5):
    """a non-convex prism: an L-shaped hexagon extruded along z, centred on its bounding box: 12 vertices, 20 faces"""
    poly = np.array([(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)], np.float64) / 2.0 - 0.5
    v = np.array([(x, y, z) for z in (-0.5, 0.5) for x, y in poly], np.float64) * (size, size, depth)
    fan = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]
    f = [(a, c, b) for a, b, c in fan] + [(a + 6, b + 6, c + 6) for a, b, c in fan]
    for i in range(6):
        j = (i + 1) % 6
        f += [(i, j, j + 6), (i, j + 6, i + 6)]
    return v, np.asarray(f, np.int32)


# ---- the mesh table -------------------------------------------------------------------------------------------------------------------
class DeviceMeshes:
    """A table of meshes ``[(vertices [P_i,3], faces [T_i,3])]``: face indices are validated here, on the host (a face that names a
    vertex outside its mesh raises ``ValueError``); the concatenated table is uploaded once per device, on first use there."""

    def __init__(self, meshes):
        meshes = list(meshes)
        if not 1 <= len(meshes) <= RASTER_MAX_MESHES:
            raise ValueError(f"DeviceMeshes takes 1 .. {RASTER_MAX_MESHES} meshes")
        vs, fs, voff, foff, cent = [], [], [0], [0], []
        for k, (v, f) in enumerate(meshes):
            v = np.ascontiguousarray(np.asarray(v, np.float64))
            f = np.asarray(f)
            if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
                raise ValueError(f"mesh {k}: vertices must be [P,3] with P >= 1")
            if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
                raise ValueError(f"mesh {k}: faces must be integers [T,3]")
            if f.size and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
                raise ValueError(f"mesh {k}: a face names a vertex outside 0 .. {v.shape[0] - 1}")
            vs.append(v)
            fs.append(np.ascontiguousarray(f.astype(np.int32)))
            voff.append(voff[-1] + v.shape[0])
            foff.append(foff[-1] + f.shape[0])
            cent.append(v.mean(0))
        self.count = len(meshes)
        self.vertices = np.concatenate(vs, 0)
        self.faces = np.concatenate(fs, 0).reshape(-1, 3)
        self.vertex_offset, self.face_offset = np.asarray(voff, np.int32), np.asarray(foff, np.int32)
        self.centroids = np.stack(cent, 0)   # what render_labels(order=None) sorts by
        self._c_voff = (C.c_int32 * len(voff))(*voff)
        self._c_foff = (C.c_int32 * len(foff))(*foff)
        self._device = {}

    @property
    def total_vertices(self):
        return int(self.vertex_offset[-1])

    @property
    def total_faces(self):
        return int(self.face_offset[-1])

    def face_count(self, mesh_id):
        return int(self.face_offset[mesh_id + 1] - self.face_offset[mesh_id])

    def table_arguments(self, dev):
        """the seven arguments every ``pvnet_render*`` entry point opens with: vertices, faces, the two offset arrays, M, P, T"""
        vertices, faces, _ = self.on(dev)
        return _ptr(vertices), _ptr(faces), self._c_voff, self._c_foff, self.count, self.total_vertices, self.total_faces

    def on(self, dev):
        """(vertices, faces, centroids) on ``dev``, uploaded on first use"""
        dev = torch.device(dev)
        if dev not in self._device:
            self._device[dev] = (torch.from_numpy(self.vertices).to(dev), torch.from_numpy(self.faces).to(dev),
                                 torch.from_numpy(self.centroids).to(dev))
        return self._device[dev]


def raster_workspace_bytes(q, h, w, meshes=None, b=None):
    """bytes of workspace for q instances of h x w pixels (``rasterize_triangles``: q = n images)"""
    return _mesh.workspace_bytes("raster", q, q if b is None else b, h, w, meshes, told=f"q={q}, h={h}, w={w}")


def _out(out, shape, dev):
    return _mesh.check_out(out, shape, torch.uint8, dev, "out", spelled="uint8")


def rasterize_triangles(triangles_2d, h, w, out=None, workspace=None, return_status=False):
    """Stage R: ``[n,tn,3,2]`` (or ``[tn,3,2]``) float32 CUDA triangles -> ``[n,h,w]`` (or ``[h,w]``) uint8, 0 or 1: the reference's
    mesh_binary_rasterization per image.  ``return_status``: also ``[n]`` int32 (``RASTER_S_NONFINITE`` where a triangle was skipped)."""
    if not (isinstance(triangles_2d, torch.Tensor) and triangles_2d.is_cuda):
        raise RuntimeError("triangles_2d must be a CUDA tensor (there is no CPU fallback)")
    single = triangles_2d.dim() == 3
    tri = triangles_2d[None] if single else triangles_2d
    if tri.dtype != torch.float32 or tri.dim() != 4 or tuple(tri.shape[2:]) != (3, 2):
        raise RuntimeError(f"triangles_2d must be float32 [n,tn,3,2] or [tn,3,2], got {triangles_2d.dtype} {tuple(triangles_2d.shape)}")
    h, w = int(h), int(w)
    if h < 2 or w < 2:
        raise RuntimeError("h and w must be at least 2")
    tri = tri.contiguous()
    dev, n, tn = tri.device, int(tri.shape[0]), int(tri.shape[1])
    if out is not None and single:
        out = out[None] if out.dim() == 2 else out
    out = _out(out, (n, h, w), dev)
    status = torch.empty(n, dtype=torch.int32, device=dev) if return_status else None
    lib = load_raster_library()
    with torch.cuda.device(dev):
        for i0 in range(0, n, RASTER_MAX_IMAGES):
            k = min(RASTER_MAX_IMAGES, n - i0)
            ws = _workspace(workspace, raster_workspace_bytes(k, h, w), dev, align=16, sized=True)
            _check(lib.pvnet_raster_triangles(_ptr(tri[i0:]), k, tn, h, w, _ptr(out[i0:]), _ptr(status[i0:]) if return_status else None,
                                              _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_raster_triangles")
    res = out[0] if single else out
    return (res, status) if return_status else res


def mesh_binary_rasterization(triangles_2d, h, w):
    """The reference's call form (lib/utils/extend_utils/extend_utils.py:7-20): numpy ``[tn,3,2]`` in, numpy uint8 ``[h,w]`` out,
    computed on the current device."""
    triangles_2d = np.asarray(triangles_2d)
    assert triangles_2d.ndim == 3 and triangles_2d.shape[1] == 3 and triangles_2d.shape[2] == 2
    tri = torch.from_numpy(np.ascontiguousarray(triangles_2d, np.float32)).to("cuda")
    return rasterize_triangles(tri, h, w).cpu().numpy()


def _render(meshes, dev, mesh_ids, image_ids, labels, poses, K, k_per_instance, order, b, h, w, out, tri_out, status, workspace):
    """one pvnet_render call per stretch of at most RASTER_MAX_INSTANCES instances, cut at image boundaries; ``poses`` [q,3,4]"""
    lib = load_raster_library()
    q = len(mesh_ids)
    cuts, start = [], 0
    while start < q:   # stretches of whole images
        stop = min(q, start + RASTER_MAX_INSTANCES)
        if stop < q:
            while stop > start and image_ids[stop] == image_ids[stop - 1]:
                stop -= 1
            if stop == start:
                raise RuntimeError(f"more than {RASTER_MAX_INSTANCES} instances in one image")
        cuts.append((start, stop))
        start = stop
    if not cuts:
        cuts = [(0, 0)]
    tri0 = 0
    with torch.cuda.device(dev):
        for ci, (s, e) in enumerate(cuts):
            # the images of this stretch: from its first image (or 0) up to the next stretch's first image (or b)
            i0 = 0 if ci == 0 else image_ids[s]
            i1 = b if ci == len(cuts) - 1 else image_ids[e]
            head = _mesh.argument_head(meshes, dev, mesh_ids[s:e], poses[s:], K[s:] if k_per_instance else K, k_per_instance,
                                       [i - i0 for i in image_ids[s:e]], labels[s:e])
            ws = _workspace(workspace, raster_workspace_bytes(e - s, h, w, meshes, i1 - i0) if h >= 2 and w >= 2 else 16, dev, align=16,
                            sized=True)
            _check(lib.pvnet_render(*head, _mesh.at(order, s), i1 - i0, h, w, _mesh.at(out, i0), _mesh.at(tri_out, tri0),
                                    _mesh.at(status, s), _ptr(ws), _nbytes(ws), _stream(dev)), "pvnet_render")
            tri0 += sum(meshes.face_count(m) for m in mesh_ids[s:e])


def project_triangles(meshes, mesh_id, poses, K):
    """Stage P: the float32 triangles of mesh ``mesh_id`` under ``poses [n,3,4]`` (float64 CUDA) -> ``[n,tn,3,2]`` float32."""
    _mesh.check_meshes(meshes, DeviceMeshes)
    mesh_id = int(mesh_id)
    if not 0 <= mesh_id < meshes.count:
        raise RuntimeError(f"mesh_id must lie in 0 .. {meshes.count - 1}")
    poses = _mesh.check_poses(poses, 3)
    dev, n, tn = poses.device, int(poses.shape[0]), meshes.face_count(mesh_id)
    Kd, per = _mesh.check_camera(K, dev, (n,))
    tri = torch.empty((n, tn, 3, 2), dtype=torch.float32, device=dev)
    if n and tn:
        _render(meshes, dev, [mesh_id] * n, list(range(n)), [1] * n, poses, Kd, per, None, n, 2, 2, None, tri.view(-1, 3, 2), None, None)
    return tri


def render_masks(meshes, mesh_id, poses, K, h, w, out=None, workspace=None, return_status=False):
    """P + R, one instance per image: the silhouette of mesh ``mesh_id`` under every pose.

    :param meshes:  ``DeviceMeshes``
    :param mesh_id: which mesh (one for all images), or a sequence of n
    :param poses:   [n,3,4] float64 CUDA tensor (what ``pnp_batch_device`` returns is read in place)
    :param K:       [3,3] shared or [n,3,3], float64 (CUDA tensor, or numpy: uploaded here)
    :param out:     None or a contiguous uint8 CUDA tensor [n,h,w]; every byte is overwritten
    :param workspace: None or a uint8 CUDA tensor of ``raster_workspace_bytes(n, h, w, meshes)`` bytes, 16-byte aligned
    :return: ``masks [n,h,w]`` uint8 (0 / 1); with ``return_status`` also ``[n]`` int32 of ``RASTER_S_*`` bits
    """
    _mesh.check_meshes(meshes, DeviceMeshes)
    poses = _mesh.check_poses(poses, 3)
    dev, n, h, w = poses.device, int(poses.shape[0]), int(h), int(w)
    ids = [int(mesh_id)] * n if np.ndim(mesh_id) == 0 else [int(m) for m in mesh_id]
    if len(ids) != n or any(not 0 <= m < meshes.count for m in ids):
        raise RuntimeError(f"mesh_id: one id, or n={n} ids, in 0 .. {meshes.count - 1}")
    if h < 2 or w < 2:
        raise RuntimeError("h and w must be at least 2")
    Kd, per = _mesh.check_camera(K, dev, (n,))
    out = _out(out, (n, h, w), dev)
    status = torch.empty(n, dtype=torch.int32, device=dev) if return_status else None
    if n:
        _render(meshes, dev, ids, list(range(n)), [1] * n, poses, Kd, per, None, n, h, w, out, None, status, workspace)
    return (out, status) if return_status else out


def render_labels(meshes, mesh_ids, labels, poses, K, h, w, order=None, out=None, workspace=None, return_status=False):
    """P + R + C: m instances per image composed in painter's order -- a pixel takes the label of the LAST painted instance covering it.

    :param mesh_ids: [m] mesh per instance;  :param labels: [m] label per instance, 1 .. 255
    :param poses:    [b,m,3,4] float64 CUDA tensor
    :param K:        [3,3] shared or [b,m,3,3], float64
    :param order:    None: far to near by the camera-space z of each mesh's centroid, decided on the device
                     (``torch.argsort(stable=True)``, no synchronisation); or the instances' indices in the order they are painted,
                     [m] for all images or [b,m] (a sequence, or an integer CUDA tensor)
    :return: ``labels [b,h,w]`` uint8; with ``return_status`` also ``[b,m]`` int32 of ``RASTER_S_*`` bits
    """
    _mesh.check_meshes(meshes, DeviceMeshes)
    poses = _mesh.check_poses(poses, 4)
    dev, b, m, h, w = poses.device, int(poses.shape[0]), int(poses.shape[1]), int(h), int(w)
    mesh_ids, labels = _mesh.check_instances(meshes, mesh_ids, labels, m, h, w, RASTER_MAX_INSTANCES)
    Kd, per = _mesh.check_camera(K, dev, (b, m))
    if order is None:
        cent = meshes.on(dev)[2][torch.as_tensor(mesh_ids, device=dev)] if m else torch.zeros((0, 3), dtype=torch.float64, device=dev)
        z = ((poses[:, :, 2, 0] * cent[:, 0] + poses[:, :, 2, 1] * cent[:, 1]) + poses[:, :, 2, 2] * cent[:, 2]) + poses[:, :, 2, 3]
        seq = torch.argsort(z, dim=1, descending=True, stable=True)
    else:
        seq = order.to(dev) if isinstance(order, torch.Tensor) else torch.as_tensor(np.asarray(order, np.int64)).to(dev)
        if seq.dim() == 1:
            seq = seq[None].expand(b, m)
        if tuple(seq.shape) != (b, m):
            raise RuntimeError(f"order must be [m] or [b,m] = {(b, m)}")
    rank = torch.argsort(seq, dim=1, stable=True).to(torch.int32).contiguous().view(-1)   # the inverse permutation: position of instance i
    out = _out(out, (b, h, w), dev)
    status = torch.empty(b * m, dtype=torch.int32, device=dev) if return_status else None
    if b:
        _render(meshes, dev, mesh_ids * b, [i for i in range(b) for _ in range(m)], labels * b, poses.view(-1, 3, 4), Kd, per, rank, b, h, w,
                out, None, status, workspace)
    return (out, status.view(b, m)) if return_status else out
