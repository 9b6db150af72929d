"""GPU tests of the textured renderer (pvnet_amd/texture.py, libpvnet_texture.so) against THE DEFINITION of include/pvnet_texture.h as
tests/texture_restatement.py restates it, against libpvnet_shade.so on untextured meshes and against libpvnet_depth.so on the same
inputs.  Every comparison is ``torch.equal``: the colour bytes, the float32 depth's bits, the labels, the visible counts and the status.

Shapes are the shade device tests': 48 x 64 and 60 x 80 images, once 33 x 47 (the resolve kernel's tail), b <= 3, q <= 6, icosphere(1)
and icosphere(2) with spherical uv for the lane's own walk, a box near the camera for the cooperative path; textures of 1 x 1, 2 x 2,
5 x 3, 8 x 8 and 16 x 16 random bytes and a smooth 64 x 64."""
import ctypes as C

import numpy as np
import pytest
import torch

from pvnet_amd import _abi, depth, render, shade, texture
from tests import test_shade_device as SD   # its fixtures: the crossing bars, backgrounds, the comparison
from tests import texture_restatement as TR
from tests.render_cases import camera, coop_count, cuda, dev, pose, smooth_colors, smooth_texture, spherical_uv

pytestmark = pytest.mark.gpu

SIZES = [(48, 64), (60, 80)]
BG = (12, 200, 77)
FILTERS = ("nearest", "bilinear")


def random_texture(th, tw, seed=0, channels=3):
    return np.random.default_rng(1000 * th + tw + seed).integers(0, 256, (th, tw, channels), dtype=np.uint8)


def box_uv(vertices):
    """a uv per corner of a box from its position: every side shows a different part of the texture, some of it outside 0 .. 1"""
    s = np.asarray(vertices, np.float64) / np.abs(vertices).max(0)   # +-1 per axis
    return np.stack([0.5 + 0.45 * s[:, 0] + 0.1 * s[:, 2], 0.5 + 0.4 * s[:, 1] - 0.15 * s[:, 2]], 1)


def table_of(meshes):
    """(TexturedMeshes, the meshes as the restatement takes them: the table's own colours, normals, float32 uv and texels)"""
    table = texture.TexturedMeshes(meshes)
    return table, [table.mesh(k) for k in range(table.count)]


def crossing_bars():
    """tests/test_shade_device.py's fixture with one bar textured (16 x 16 random bytes), the other vertex-coloured and the sphere
    textured (64 x 64, smooth): textured and untextured instances interpenetrate in one image"""
    _, ids, labels, poses = SD.crossing_bars()
    bar, ball = render.box_mesh(0.25, 0.06, 0.05), render.icosphere(2, 0.04)
    meshes = [(*bar, None, None, box_uv(bar[0]), random_texture(16, 16)), (*bar, smooth_colors(bar[0]), None, None, None),
              (*ball, smooth_colors(ball[0], 1.0), None, spherical_uv(ball[0]), smooth_texture())]
    assert ids == [0, 0, 1]
    return meshes, [0, 1, 2], labels, poses


def restated(meshes, mesh_ids, labels, poses, K, h, w, layers=None, **kw):
    b, m = poses.shape[:2]
    inst = [(mesh_ids[j], poses[i, j], K, i, labels[j]) for i in range(b) for j in range(m)]
    rgb, d, lab, vis, st = TR.render(meshes, inst, b, h, w, layers=layers, **kw)
    return (torch.from_numpy(rgb), torch.from_numpy(d), torch.from_numpy(lab), torch.from_numpy(vis).view(b, m),
            torch.from_numpy(st).view(b, m))


same = SD.same


def full(table, mesh_ids, labels, poses, K, h, w, **kw):
    return texture.render_textured(table, mesh_ids, labels, cuda(poses), K, h, w, return_visible=True, return_status=True, **kw)


# ---- 1. filters and shadings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shading", ["none", "flat", "phong"])
@pytest.mark.parametrize("size", SIZES)
def test_filters_shadings_ambients_and_backgrounds_on_interpenetrating_instances(size, shading):
    h, w = size
    K = camera(h, w)
    meshes, ids, labels, poses = crossing_bars()
    table, rmeshes = table_of(meshes)
    image = SD.background_image(2, h, w)
    layers = {}
    seen = []
    for filt in FILTERS:
        for ambient in (0.0, 0.5):
            got = full(table, ids, labels, poses, K, h, w, shading=shading, ambient=ambient, filter=filt, background=BG)
            same(got, restated(rmeshes, ids, labels, poses, K, h, w, layers, shading=shading, ambient=ambient, filter=filt, background=BG))
            assert set(torch.unique(got[2]).cpu().tolist()) == {0, 1, 2, 3}
            assert (got[0][got[2] == 0].cpu() == torch.tensor(BG, dtype=torch.uint8)).all()
            seen.append(got[0].cpu())
            got = full(table, ids, labels, poses, K, h, w, shading=shading, ambient=ambient, filter=filt, background=cuda(image))
            same(got, restated(rmeshes, ids, labels, poses, K, h, w, layers, shading=shading, ambient=ambient, filter=filt, background=image))
            empty = (got[2] == 0).cpu()
            assert torch.equal(got[0].cpu()[empty], torch.from_numpy(image)[empty])
    assert not torch.equal(seen[1], seen[3])   # the filter is not ignored
    # the defaults: flat, ambient 0.5, nearest, black
    rgb, _, lab = texture.render_textured(table, ids, labels, cuda(poses), K, h, w)
    want = restated(rmeshes, ids, labels, poses, K, h, w, layers)
    assert torch.equal(rgb.cpu(), want[0]) and not rgb[lab == 0].any()


# ---- 2. untextured equals the shade library ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_untextured_meshes_come_out_as_from_the_shade_library(size):
    h, w = size
    K = camera(h, w)
    cmeshes, ids, labels, poses = SD.crossing_bars()
    near = render.box_mesh(0.3, 0.2, 0.2)
    cmeshes = cmeshes + [(*near, smooth_colors(near[0], 2.0))]
    ids, labels = ids + [2], labels + [4]
    poses = np.concatenate([poses, np.stack([pose((2, 1, -1), 0.8, (0.18, 0.02, 0.62)), pose((2, 1, -1), 0.8, (0.18, 0.02, 0.42))])[:, None]], 1)
    ctable = shade.ColorMeshes(cmeshes)
    ttable = texture.TexturedMeshes([(*m, None, None, None) for m in cmeshes])
    image = cuda(SD.background_image(2, h, w))
    ws = torch.empty(texture.texture_workspace_bytes(8, 2, h, w, ttable), dtype=torch.uint8, device=dev())
    ws_c = torch.empty(shade.shade_workspace_bytes(8, 2, h, w, ctable), dtype=torch.uint8, device=dev())
    assert ws.numel() == ws_c.numel()
    for shading in ("none", "flat", "phong"):
        for filt in FILTERS:   # no mesh is textured: the filter changes nothing
            for kw in (dict(ambient=0.5, background=BG), dict(ambient=0.2, background=image, far=0.5)):
                got = full(ttable, ids, labels, poses, K, h, w, shading=shading, filter=filt, workspace=ws, **kw)
                want = shade.render_color(ctable, ids, labels, cuda(poses), K, h, w, shading=shading, return_visible=True, return_status=True,
                                          workspace=ws_c, **kw)
                assert len(got) == len(want) == 5 and all(torch.equal(a, b) for a, b in zip(got, want))
                assert got[2].any() and coop_count(ws) == coop_count(ws_c) > 0


# ---- 3. equals the depth library ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_depth_labels_visible_and_status_are_the_depth_librarys(size):
    h, w = size
    K = camera(h, w)
    meshes, ids, labels, poses = crossing_bars()
    table, _ = table_of(meshes)
    for far in (np.inf, 0.5):
        for filt in FILTERS:
            got = full(table, ids, labels, poses, K, h, w, far=far, filter=filt)
            want = depth.render_depth(table, ids, labels, cuda(poses), K, h, w, far=far, return_visible=True, return_status=True)
            assert all(torch.equal(a, b) for a, b in zip(got[1:], want))
            assert got[2].any() and torch.equal(got[1] != 0, got[2] != 0)


# ---- 4. texel boundaries -----------------------------------------------------------------------------------------------------------------
QUAD_K = np.array([[64.0, 0.0, 31.5], [0.0, 64.0, 23.5], [0.0, 0.0, 1.0]])
QUAD_V = np.array([[-0.25, -0.25, 1.0], [0.25, -0.25, 1.0], [0.25, 0.25, 1.0], [-0.25, 0.25, 1.0]])
QUAD_UV = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0], [0.0, 0.0]])
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


@pytest.mark.parametrize("side", [8, 1, 2])
def test_known_answer_quad_texel_boundaries(side):
    """tests/test_texture_cpu.py's known answer: the screen quad is exactly [15.5, 47.5] x [7.5, 39.5], every texel of an 8 x 8 texture
    a block of 4 x 4 pixels; a 2 x 2 texture over 32 pixels is the strongest bilinear gradient"""
    h, w = 48, 64
    tex = random_texture(side, side, 4)
    table, rmeshes = table_of([(QUAD_V, QUAD_F, None, None, QUAD_UV, tex)])
    p = EYE[None, None]
    for filt in FILTERS:
        for shading in ("none", "flat"):
            got = full(table, [0], [5], p, QUAD_K, h, w, shading=shading, ambient=0.25, filter=filt, background=BG)
            same(got, restated(rmeshes, [0], [5], p, QUAD_K, h, w, shading=shading, ambient=0.25, filter=filt, background=BG))
            assert int(got[3]) == 32 * 32 and int(got[4]) == 0
    rgb = full(table, [0], [5], p, QUAD_K, h, w, shading="none", background=BG)[0].cpu().numpy()
    want = np.empty((h, w, 3), np.uint8)
    want[:] = BG
    want[8:40, 16:48] = np.kron(tex, np.ones((32 // side, 32 // side, 1), np.uint8))
    assert np.array_equal(rgb[0], want)
    soft = full(table, [0], [5], p, QUAD_K, h, w, shading="none", filter="bilinear", background=BG)[0].cpu().numpy()
    assert np.array_equal(soft, rgb) == (side == 1)   # one texel is one colour; otherwise the blend shows


# ---- 5. uv outside the unit square -------------------------------------------------------------------------------------------------------
def test_uv_outside_the_unit_square_nan_and_infinities():
    h, w = 48, 64
    K = camera(h, w)
    v, f = render.icosphere(1, 0.1)
    base = spherical_uv(v)
    stretched = base * 3.0 - 1.0                      # -1 .. 2: most of it clamps to an edge
    exact = np.round(base)                            # exactly 0 and exactly 1
    variants = [stretched, exact]
    for bad in ((np.nan, 0.5), (np.inf, -np.inf), (-np.inf, np.nan), (1e30, -1e30)):
        wild = stretched.copy()
        wild[3] = bad
        variants.append(wild)
    tex = random_texture(5, 3)
    p = pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5))[None, None]
    clean = None
    for uv in variants:
        table, rmeshes = table_of([(v, f, None, None, uv, tex)])
        for filt in FILTERS:
            got = full(table, [0], [1], p, K, h, w, shading="phong", ambient=0.3, filter=filt, background=BG)
            same(got, restated(rmeshes, [0], [1], p, K, h, w, shading="phong", ambient=0.3, filter=filt, background=BG))
            assert int(got[4]) == 0 and int(got[3]) > 300   # uv never touches the status, the coverage or the depth
            clean = got if clean is None else clean
            assert all(torch.equal(a, b) for a, b in zip(got[1:], clean[1:]))


# ---- both paths of the triangle kernel, the tail of the resolve kernel ----------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [(33, 47)])
def test_both_kernel_paths_the_cooperative_counter_and_the_tail(size):
    h, w = size
    K = camera(h, w)
    small, box = render.icosphere(2, 0.1), render.box_mesh(0.3, 0.2, 0.2)
    table, rmeshes = table_of([(*small, None, None, spherical_uv(small[0]), random_texture(2, 2)),
                               (*box, smooth_colors(box[0], 2.0), None, box_uv(box[0]), random_texture(5, 3))])
    ws = torch.empty(texture.texture_workspace_bytes(2, 1, h, w, table), dtype=torch.uint8, device=dev())
    far_ball = pose((1, 2, 3), 0.4, (0.0, 0.0, 0.9))[None, None]             # every face's box is a few pixels
    got = full(table, [0], [1], far_ball, K, h, w, shading="phong", filter="bilinear", workspace=ws)
    same(got, restated(rmeshes, [0], [1], far_ball, K, h, w, shading="phong", filter="bilinear"))
    assert coop_count(ws) == 0 and got[2].any()
    near = np.stack([pose((1, 2, 3), 0.4, (0.0, 0.0, 0.9)), pose((2, 1, -1), 0.8, (0.18, 0.12, 0.42))])[None]   # the box reaches the last rows
    for filt in FILTERS:
        got = full(table, [0, 1], [1, 2], near, K, h, w, shading="flat", ambient=0.2, filter=filt, background=BG, workspace=ws)
        same(got, restated(rmeshes, [0, 1], [1, 2], near, K, h, w, shading="flat", ambient=0.2, filter=filt, background=BG))
        assert coop_count(ws) > 0 and int((got[2] == 2).sum()) > h * w // 10 and got[2][0, -1].any()


# ---- the C ABI itself: colours absent, a dirty workspace, an image without instances ---------------------------------------------------------
def test_raw_call_without_colours_on_a_dirty_workspace_with_an_empty_image():
    h, w = 48, 64
    K = camera(h, w)
    ball, box = render.icosphere(1, 0.1), render.box_mesh(0.15, 0.1, 0.2)
    table, rmeshes = table_of([(*ball, None, None, spherical_uv(ball[0]), random_texture(16, 16, channels=4)),
                               (*box, smooth_colors(box[0]), None, None, None),
                               (*box, None, None, box_uv(box[0]), random_texture(1, 1))])
    poses = np.stack([pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5)), pose((2, 1, -1), 1.2, (0.04, 0.03, 0.6)), pose((3, -1, 2), 2.1, (-0.1, 0.05, 0.55))])
    lib = _abi.load_texture_library()
    vertices, faces, _ = table.on(dev())
    colors, normals = table.shading_on(dev())
    uv, texels = table.textures_on(dev())
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    i32 = lambda vals: (C.c_int32 * len(vals))(*vals)   # noqa: E731
    Kd, pd = cuda(K), cuda(poses)

    def call(mesh_ids, with_colors, fill):
        ws = torch.full((texture.texture_workspace_bytes(3, 3, h, w, table),), fill, dtype=torch.uint8, device=dev())
        rgb = torch.full((3, h, w, 3), 99, dtype=torch.uint8, device=dev())
        d = torch.full((3, h, w), 7.0, dtype=torch.float32, device=dev())
        lab = torch.full((3, h, w), 9, dtype=torch.uint8, device=dev())
        vis = torch.full((3,), -5, dtype=torch.int32, device=dev())
        st = torch.full((3,), -5, dtype=torch.int32, device=dev())
        rc = lib.pvnet_render_textured(ptr(vertices), ptr(faces), table._c_voff, table._c_foff, table.count, table.total_vertices,
                                       table.total_faces, 3, i32(mesh_ids), ptr(pd), ptr(Kd), 0, i32([0, 0, 2]), i32([4, 5, 6]), 3, h, w,
                                       float("inf"), ptr(colors) if with_colors else None, ptr(normals), ptr(uv), ptr(texels), table._c_toff,
                                       table._c_th, table._c_tw, 1, 2, 0.3, (C.c_uint8 * 3)(*BG), None, ptr(rgb), ptr(d), ptr(lab), ptr(vis),
                                       ptr(st), ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, (rgb, d, lab, vis, st)

    def want(mesh_ids):
        inst = [(mesh_ids[0], poses[0], K, 0, 4), (mesh_ids[1], poses[1], K, 0, 5), (mesh_ids[2], poses[2], K, 2, 6)]
        return tuple(torch.from_numpy(x) for x in TR.render(rmeshes, inst, 3, h, w, shading="phong", ambient=0.3, background=BG, filter="bilinear"))

    mixed = want([0, 1, 2])
    for fill in (0xFF, 0x00):   # the workspace may hold anything on entry; every output byte is written
        rc, got = call([0, 1, 2], True, fill)
        assert rc == 0
        same(got, mixed)
        assert (got[0][1].cpu() == torch.tensor(BG, dtype=torch.uint8)).all() and not got[2][1].any()   # the image without instances
    rc, _ = call([0, 1, 2], False, 0)
    assert rc == -1                       # mesh 1 is drawn and has no texture: its colours are needed
    rc, got = call([0, 2, 2], False, 0xFF)
    assert rc == 0                        # every mesh an instance names is textured: no colours are read
    same(got, want([0, 2, 2]))


# ---- reproducible, capturable, split between images ------------------------------------------------------------------------------------------
def test_reproducible_graph_capture_and_a_call_split_between_images():
    h, w = 60, 80
    K = cuda(camera(h, w))
    meshes, ids, labels, base = crossing_bars()
    table, rmeshes = table_of(meshes)
    moved = base.copy()
    moved[1, :, 0, 3] += 0.01
    moved[:, 2, 2, 3] += 0.03
    image = cuda(SD.background_image(2, h, w))
    kw = dict(shading="phong", ambient=0.25, filter="bilinear", background=image)
    a, b = full(table, ids, labels, base, K, h, w, **kw), full(table, ids, labels, base, K, h, w, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    want = restated(rmeshes, ids, labels, base, camera(h, w), h, w, shading="phong", ambient=0.25, filter="bilinear",
                    background=image.cpu().numpy())
    same(a, want)
    for chunk in (3, 5, 6):   # one image per call, then both in one
        same(full(table, ids, labels, base, K, h, w, max_instances=chunk, **kw), want)
    with pytest.raises(RuntimeError):
        full(table, ids, labels, base, K, h, w, max_instances=2, **kw)
    static = cuda(base)
    rgb = torch.full((2, h, w, 3), 99, dtype=torch.uint8, device=dev())
    d = torch.full((2, h, w), 9.0, dtype=torch.float32, device=dev())
    lab = torch.full((2, h, w), 9, dtype=torch.uint8, device=dev())
    ws = torch.empty(texture.texture_workspace_bytes(6, 2, h, w, table), dtype=torch.uint8, device=dev())
    out = dict(out_rgb=rgb, out_depth=d, out_labels=lab, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the table's upload and a first call outside the capture
        texture.render_textured(table, ids, labels, static, K, h, w, **kw, **out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        texture.render_textured(table, ids, labels, static, K, h, w, **kw, **out)
    for p in (moved, base):
        static.copy_(cuda(p))
        rgb.fill_(99)
        d.fill_(9.0)
        lab.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        eager = texture.render_textured(table, ids, labels, cuda(p), K, h, w, **kw)
        assert torch.equal(rgb, eager[0]) and torch.equal(d, eager[1]) and torch.equal(lab, eager[2])
    assert torch.equal(rgb.cpu(), want[0]) and torch.equal(lab.cpu(), want[2])


def test_front_end_rejects_what_it_cannot_render():
    h, w = 48, 64
    K = camera(h, w)
    ball = render.icosphere(1, 0.1)
    table, _ = table_of([(*ball, None, None, spherical_uv(ball[0]), random_texture(2, 2))])
    p = cuda(pose((1, 2, 3), 0.7, (0.0, 0.0, 0.5))[None, None])
    for bad in (dict(filter="trilinear"), dict(filter=1), dict(shading="gouraud"), dict(ambient=-0.1), dict(background=(1, 2)),
                dict(max_instances=0), dict(far=0.0)):
        with pytest.raises(RuntimeError):
            texture.render_textured(table, [0], [1], p, K, h, w, **bad)
    with pytest.raises(RuntimeError):
        texture.render_textured(table, [0], [1], p.cpu(), K, h, w)                                      # a CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        texture.render_textured(shade.ColorMeshes([(*ball, smooth_colors(ball[0]))]), [0], [1], p, K, h, w)   # no texture table
    none = torch.empty((2, 0, 3, 4), dtype=torch.float64, device=dev())
    got = texture.render_textured(table, [], [], none, K, h, w, background=BG, return_visible=True, return_status=True)
    assert (got[0].cpu() == torch.tensor(BG, dtype=torch.uint8)).all() and not got[1].any() and tuple(got[3].shape) == (2, 0)
