"""What the tests of the four mesh renderers share (tests/test_raster_*.py, test_depth_*.py, test_shade_*.py, test_texture_*.py) and
tools/raster_probe.py: poses, the camera, vertex colours, a texture and its uv, the device plumbing, and the list of bad arguments
every ``pvnet_render*`` entry point refuses.  One copy of every helper that was the same function in each file that had it; the makers
under tests/golden/ keep their own copies (the record of how a fixture was made)."""
import ctypes as C

import numpy as np

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3   # PVNET_E_*


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose(axis, angle, t):
    return np.concatenate([rotation(axis, angle), np.asarray(t, np.float64).reshape(3, 1)], 1)


def camera(h, w):   # the camera of tests/golden/make_raster_golden.py
    return np.array([[0.95 * w, 0.0, w / 2.0 + 0.37], [0.0, 0.97 * w, h / 2.0 - 0.21], [0.0, 0.0, 1.0]])


def smooth_colors(vertices, phase=0.0):
    """vertex colours that are a smooth function of the position: 40 .. 215 in every channel"""
    v = np.asarray(vertices, np.float64)
    s = v / np.abs(v).max()
    c = 127.5 + 87.5 * np.stack([np.sin(2.1 * s[:, 0] + 0.3 + phase), np.sin(1.7 * s[:, 1] - 0.8 + phase), np.cos(2.4 * s[:, 2] + 0.5)], 1)
    return np.round(c).astype(np.uint8)


def smooth_texture(n=64):
    y, x = np.mgrid[0:n, 0:n] / float(n)
    c = 127.5 + 43.75 * np.stack([np.sin(2 * np.pi * x + 0.3) + np.sin(2 * np.pi * y - 0.8), np.sin(4 * np.pi * x - 0.8) + np.cos(2 * np.pi * y),
                                  np.cos(2 * np.pi * (x + y) + 0.5) + np.sin(2 * np.pi * y + 1.1)], -1)
    return np.round(c).astype(np.uint8)


def spherical_uv(vertices):
    n = np.asarray(vertices, np.float64)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return np.stack([np.arctan2(n[:, 1], n[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 2], -1, 1)) / np.pi], 1)


# ---- the device tests' plumbing (torch is imported where it is used: the probes and the CPU tests take the rest without it) ----------
def dev():
    import torch
    return torch.device("cuda:0")


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def coop_count(workspace):
    """the triangles of the last call on this workspace that took the cooperative path (PVNET_*_WS_COOP_COUNT_OFFSET = 0)"""
    import torch
    return int(workspace[:4].view(torch.int32).cpu()[0])


# ---- the "pvnet_render list": what every entry point refuses of the arguments all four open with, without a device --------------------
def i32(*v):
    return (C.c_int32 * len(v))(*v)


def refuses_the_pvnet_render_list(call, ws_n, max_meshes, max_instances, max_side, max_images):
    """``call(**changed)``: the entry point on a good argument list -- M=2, P=20, T=32, q=3, b=2, h=20, w=24, never-dereferenced
    pointers, ``nbytes=ws_n`` -- with the named arguments replaced (vertices, faces, voff, foff, M, q, mesh, poses, K, image, label, b,
    h, w, ws, nbytes) -> its code"""
    assert call(h=1) == BADARG and call(w=1) == BADARG
    for name in ("vertices", "faces", "voff", "foff", "mesh", "poses", "K", "image", "label", "ws"):
        assert call(**{name: None}) == BADARG, name
    assert call(image=i32(0, 1, 0)) == BADARG                      # decreasing image_id
    assert call(image=i32(0, 1, 2)) == BADARG and call(image=i32(-1, 0, 1)) == BADARG   # outside 0 .. b-1
    assert call(label=i32(1, 0, 3)) == BADARG and call(label=i32(1, 256, 3)) == BADARG and call(label=i32(-1, 2, 3)) == BADARG
    assert call(mesh=i32(0, 2, 1)) == BADARG and call(mesh=i32(0, -1, 1)) == BADARG     # mesh_id out of range
    assert call(voff=i32(1, 12, 20)) == BADARG and call(voff=i32(0, 12, 19)) == BADARG and call(foff=i32(0, 40, 32)) == BADARG
    assert call(M=0) == BADARG and call(q=-1) == BADARG and call(b=-1) == BADARG
    assert call(ws=C.c_void_p(0x1004)) == BADARG
    assert call(nbytes=ws_n - 1) == WORKSPACE and call(nbytes=0) == WORKSPACE
    assert call(M=max_meshes + 1) == UNSUPPORTED and call(q=max_instances + 1) == UNSUPPORTED
    assert call(w=max_side + 1) == UNSUPPORTED and call(b=max_images + 1) == UNSUPPORTED
    assert call(b=0, q=0) == 0                                      # nothing to do, nothing enqueued
