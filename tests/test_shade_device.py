"""GPU tests of the shaded vertex-colour renderer (pvnet_amd/shade.py, libpvnet_shade.so) against THE DEFINITION of include/pvnet_shade.h
as tests/shade_restatement.py restates it, and against libpvnet_depth.so on the same inputs.  Every comparison with the restatement is
``torch.equal``: the colour bytes, the float32 depth's bits, the labels, the visible counts and the status.

Shapes: 48 x 64 and 60 x 80 images, b <= 3, q <= 6, icosphere(1) and icosphere(2) for the lane's own walk, a box near the camera for the
cooperative path, the crossing bars of tests/test_depth_device.py; once 33 x 47, a pixel count that is no multiple of 4 (the resolve
kernel's tail)."""
import ctypes as C

import numpy as np
import pytest
import torch

from pvnet_amd import _abi, depth, render, shade
from tests import shade_restatement as SR
from tests.render_cases import camera, coop_count, cuda, dev, pose, smooth_colors

pytestmark = pytest.mark.gpu

SIZES = [(48, 64), (60, 80)]
BG = (12, 200, 77)


def table_of(meshes):
    """(ColorMeshes, the meshes as the restatement takes them: with the table's own colours and normals)"""
    table = shade.ColorMeshes(meshes)
    return table, [table.mesh(k) for k in range(table.count)]


def background_image(b, h, w, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)


def crossing_bars():
    """tests/test_depth_device.py's fixture -- two bars through each other and a sphere in front of one end -- coloured, and a second
    image in which the sphere is moved: [2,3,3,4] poses, meshes, ids, labels"""
    bar, ball = render.box_mesh(0.25, 0.06, 0.05), render.icosphere(2, 0.04)
    meshes = [(*bar, smooth_colors(bar[0])), (*ball, smooth_colors(ball[0], 1.0))]
    first = np.stack([pose((0, 1, 0), 0.5, (-0.02, -0.01, 0.5)), pose((0.1, 1, 0), -0.4, (-0.015, -0.005, 0.505)),
                      pose((1, 1, 0), 0.3, (0.08, 0.0, 0.42))])
    second = first.copy()
    second[2] = pose((1, 0, 1), 1.3, (-0.03, 0.01, 0.44))
    return meshes, [0, 0, 1], [1, 2, 3], np.stack([first, second])


def restated(meshes, mesh_ids, labels, poses, K, h, w, layers=None, **kw):
    """tests/shade_restatement.py for poses [b,m,3,4] -> (rgb, depth, labels, visible [b,m], status [b,m]) as CPU tensors"""
    b, m = poses.shape[:2]
    inst = [(mesh_ids[j], poses[i, j], K, i, labels[j]) for i in range(b) for j in range(m)]
    rgb, d, lab, vis, st = SR.render(meshes, inst, b, h, w, layers=layers, **kw)
    return (torch.from_numpy(rgb), torch.from_numpy(d), torch.from_numpy(lab), torch.from_numpy(vis).view(b, m),
            torch.from_numpy(st).view(b, m))


def same(got, want):
    """(rgb, depth, labels, visible, status) from the device against the restatement: the bytes, the float32 BITS, and everything else"""
    gr, gd, gl, gv, gs = (x.cpu() for x in got)
    wr, wd, wl, wv, ws = want
    assert gr.dtype == torch.uint8 and gd.dtype == torch.float32 and gl.dtype == torch.uint8 and gv.dtype == gs.dtype == torch.int32
    assert torch.equal(gd.view(torch.int32), wd.view(torch.int32))
    assert torch.equal(gl, wl) and torch.equal(gv, wv) and torch.equal(gs, ws)
    assert torch.equal(gr, wr), f"{int((gr != wr).any(-1).sum())} pixels differ"


def full(table, mesh_ids, labels, poses, K, h, w, **kw):
    return shade.render_color(table, mesh_ids, labels, cuda(poses), K, h, w, return_visible=True, return_status=True, **kw)


@pytest.mark.parametrize("shading", ["none", "flat", "phong"])
@pytest.mark.parametrize("size", SIZES)
def test_shading_modes_ambients_and_backgrounds_on_interpenetrating_instances(size, shading):
    h, w = size
    K = camera(h, w)
    meshes, ids, labels, poses = crossing_bars()
    table, rmeshes = table_of(meshes)
    image = background_image(2, h, w)
    layers = {}
    for ambient in (0.0, 0.5, 1.0):
        got = full(table, ids, labels, poses, K, h, w, shading=shading, ambient=ambient, background=BG)
        same(got, restated(rmeshes, ids, labels, poses, K, h, w, layers, shading=shading, ambient=ambient, background=BG))
        assert set(torch.unique(got[2]).cpu().tolist()) == {0, 1, 2, 3}
        assert (got[0][got[2] == 0].cpu() == torch.tensor(BG, dtype=torch.uint8)).all()
        got = full(table, ids, labels, poses, K, h, w, shading=shading, ambient=ambient, background=cuda(image))
        same(got, restated(rmeshes, ids, labels, poses, K, h, w, layers, shading=shading, ambient=ambient, background=image))
        empty = (got[2] == 0).cpu()
        assert torch.equal(got[0].cpu()[empty], torch.from_numpy(image)[empty])
    # the default background is black, the defaults are the reference's: flat, ambient 0.5
    rgb, _, lab = shade.render_color(table, ids, labels, cuda(poses), K, h, w)
    want = restated(rmeshes, ids, labels, poses, K, h, w, layers)
    assert torch.equal(rgb.cpu(), want[0]) and not rgb[lab == 0].any()


@pytest.mark.parametrize("size", SIZES)
def test_depth_labels_visible_and_status_are_the_depth_librarys(size):
    h, w = size
    K = camera(h, w)
    meshes, ids, labels, poses = crossing_bars()
    table, _ = table_of(meshes)
    for far in (np.inf, 0.5):
        got = full(table, ids, labels, poses, K, h, w, far=far)
        want = depth.render_depth(table, ids, labels, cuda(poses), K, h, w, far=far, return_visible=True, return_status=True)
        assert all(torch.equal(a, b) for a, b in zip(got[1:], want))
        assert got[2].any() and torch.equal(got[1] != 0, got[2] != 0)
    # far = 10 cuts a sphere of radius 3 at z = 11: its front is at 8, its rim near 10.6
    ball = render.icosphere(2, 3.0)
    big, rbig = table_of([(*ball, smooth_colors(ball[0]))])
    p = pose((1, 0, 1), 0.3, (0.3, -0.2, 11.0))[None, None]
    whole = full(big, [0], [9], p, K, h, w)
    cut = full(big, [0], [9], p, K, h, w, far=10.0, background=BG)
    want = depth.render_depth(big, [0], [9], cuda(p), K, h, w, far=10.0, return_visible=True, return_status=True)
    assert all(torch.equal(a, b) for a, b in zip(cut[1:], want))
    same(cut, restated(rbig, [0], [9], p, K, h, w, far=10.0, background=BG))
    assert 0 < int(cut[3]) < int(whole[3]) and float(cut[1].max()) < 10.0 < float(whole[1].max())
    dropped = (whole[2] != 0) & (cut[2] == 0)
    assert dropped.any() and (cut[0][dropped].cpu() == torch.tensor(BG, dtype=torch.uint8)).all()
    kept = cut[2] != 0
    assert torch.equal(cut[0][kept], whole[0][kept])   # the colour of a kept pixel does not depend on far


def test_an_exact_tie_of_two_instances_goes_to_the_earlier_one():
    h, w = 48, 64
    K = camera(h, w)
    v, f = render.l_prism_mesh(0.2, 0.08)
    red, blue = np.tile(np.array([[220, 30, 30]], np.uint8), (len(v), 1)), np.tile(np.array([[30, 30, 220]], np.uint8), (len(v), 1))
    table, rmeshes = table_of([(v, f, red), (v, f, blue)])
    p = pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5))
    poses = np.stack([p, p.copy()])[None]
    for ids, first in (([0, 1], (220, 30, 30)), ([1, 0], (30, 30, 220))):
        got = full(table, ids, [3, 7], poses, K, h, w, shading="none", background=BG)
        same(got, restated(rmeshes, ids, [3, 7], poses, K, h, w, shading="none", background=BG))
        covered = got[2] != 0
        assert int(covered.sum()) > 50 and (got[2][covered] == 3).all() and got[3].cpu().tolist() == [[int(covered.sum()), 0]]
        assert (got[0][covered].cpu() == torch.tensor(first, dtype=torch.uint8)).all()
        lit = full(table, ids, [3, 7], poses, K, h, w, shading="flat", ambient=0.3)
        same(lit, restated(rmeshes, ids, [3, 7], poses, K, h, w, shading="flat", ambient=0.3))
        assert (lit[0][covered][:, 1] <= 30).all()    # shaded, but still the first instance's hue
        assert (lit[0][covered][:, 0 if first[0] > 100 else 2] > lit[0][covered][:, 1]).all()


def test_a_duplicated_face_goes_to_the_lower_face_index():
    h, w = 48, 64
    K = camera(h, w)
    v, f = render.icosphere(1, 0.1)
    P = len(v)
    v2 = np.concatenate([v, v])
    colors = np.concatenate([np.tile(np.array([[200, 100, 0]], np.uint8), (P, 1)), np.tile(np.array([[0, 100, 200]], np.uint8), (P, 1))])
    poses = pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5))[None, None]
    for faces, first in ((np.concatenate([f, f + P]), (200, 100, 0)), (np.concatenate([f + P, f]), (0, 100, 200))):
        table, rmeshes = table_of([(v2, faces, colors)])
        got = full(table, [0], [1], poses, K, h, w, shading="none")
        same(got, restated(rmeshes, [0], [1], poses, K, h, w, shading="none"))
        covered = got[2] != 0
        assert int(covered.sum()) > 300 and (got[0][covered].cpu() == torch.tensor(first, dtype=torch.uint8)).all()
        same(full(table, [0], [1], poses, K, h, w, shading="phong", ambient=0.2),
             restated(rmeshes, [0], [1], poses, K, h, w, shading="phong", ambient=0.2))


@pytest.mark.parametrize("size", SIZES)
def test_both_kernel_paths_and_the_cooperative_counter(size):
    h, w = size
    K = camera(h, w)
    small, box = render.icosphere(2, 0.1), render.box_mesh(0.3, 0.2, 0.2)
    table, rmeshes = table_of([(*small, smooth_colors(small[0])), (*box, smooth_colors(box[0], 2.0))])
    ws = torch.empty(shade.shade_workspace_bytes(2, 1, h, w, table), dtype=torch.uint8, device=dev())
    far_ball = pose((1, 2, 3), 0.4, (0.0, 0.0, 0.9))[None, None]             # every face's box is a few pixels
    for shading in ("flat", "phong"):
        got = full(table, [0], [1], far_ball, K, h, w, shading=shading, workspace=ws)
        same(got, restated(rmeshes, [0], [1], far_ball, K, h, w, shading=shading))
        assert coop_count(ws) == 0 and got[2].any()
    near = np.stack([pose((1, 2, 3), 0.4, (0.0, 0.0, 0.9)), pose((2, 1, -1), 0.8, (0.18, 0.02, 0.42))])[None]   # the box fills a third of the frame
    for shading in ("flat", "phong"):
        got = full(table, [0, 1], [1, 2], near, K, h, w, shading=shading, ambient=0.2, background=BG, workspace=ws)
        same(got, restated(rmeshes, [0, 1], [1, 2], near, K, h, w, shading=shading, ambient=0.2, background=BG))
        assert coop_count(ws) > 0 and int((got[2] == 2).sum()) > h * w // 4 and (got[2] == 1).any()


def test_triangles_behind_the_camera_set_the_status_bit_and_draw_nothing():
    h, w = 48, 64
    K = camera(h, w)
    tri = (np.array([[-0.05, -0.05, 0.3], [0.05, -0.05, 0.3], [0.0, 0.05, -0.2]]), np.array([[0, 1, 2]], np.int32))   # one vertex behind
    ball = render.icosphere(2, 0.1)
    table, rmeshes = table_of([(*tri, np.full((3, 3), 255, np.uint8)), (*ball, smooth_colors(ball[0]))])
    eye = pose((0, 0, 1), 0.0, (0, 0, 0))
    got = full(table, [0], [1], eye[None, None], K, h, w, background=BG)
    assert int(got[4]) == SR.S_BEHIND and int(got[3]) == 0 and not got[1].any() and not got[2].any()
    assert (got[0].cpu() == torch.tensor(BG, dtype=torch.uint8)).all()
    same(got, restated(rmeshes, [0], [1], eye[None, None], K, h, w, background=BG))
    # the camera inside the sphere: the triangles wholly in front are drawn, the instance is flagged
    poses = np.stack([eye, pose((1, 0, 1), 1.3, (0.01, 0.02, 0.03))])[None]
    for shading in ("flat", "phong"):
        got = full(table, [0, 1], [1, 2], poses, K, h, w, shading=shading)
        same(got, restated(rmeshes, [0, 1], [1, 2], poses, K, h, w, shading=shading))
        assert (got[4].cpu() & SR.S_BEHIND).all() and (got[2] == 2).any()


def raw_call(table, mesh_ids, image_ids, labels, poses, K, b, h, w, rgb, far=np.inf, shading=1, ambient=0.5, bg=BG, bg_image=None,
             depth_out=None, label_out=None, visible=None, status=None, ws=None):
    """pvnet_render_color itself: an instance list the front end cannot express (an image without instances), outputs at any address"""
    lib = _abi.load_shade_library()
    vertices, faces, _ = table.on(dev())
    colors, normals = table.shading_on(dev())
    q = len(mesh_ids)
    arr = lambda vals: (C.c_int32 * max(q, 1))(*vals)   # noqa: E731
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    if ws is None:
        ws = torch.empty(shade.shade_workspace_bytes(q, b, h, w, table), dtype=torch.uint8, device=dev())
    Kd = cuda(K)
    rc = lib.pvnet_render_color(ptr(vertices), ptr(faces), table._c_voff, table._c_foff, table.count, table.total_vertices,
                                table.total_faces, q, arr(mesh_ids), ptr(poses), ptr(Kd), 0, arr(image_ids), arr(labels), b, h, w, far,
                                ptr(colors), ptr(normals), shading, ambient, (C.c_uint8 * 3)(*bg), ptr(bg_image), ptr(rgb), ptr(depth_out),
                                ptr(label_out), ptr(visible), ptr(status), ptr(ws), ws.numel(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def edge_scene():
    """instances in images 0, 0 and 2 of three, 48 x 64: the restatement with a background colour and with a background image"""
    h, w = 48, 64
    K = camera(h, w)
    shapes = [render.box_mesh(0.15, 0.1, 0.2), render.icosphere(1, 0.1), render.icosphere(2, 0.1)]
    table, rmeshes = table_of([(*m, smooth_colors(m[0], k)) for k, m in enumerate(shapes)])
    poses = np.stack([pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5)), pose((2, 1, -1), 1.2, (0.04, 0.03, 0.6)),
                      pose((3, -1, 2), 2.1, (-0.1, 0.05, 0.55))])
    inst = [(1, poses[0], K, 0, 4), (2, poses[1], K, 0, 5), (0, poses[2], K, 2, 6)]
    image = background_image(3, h, w, 9)
    layers = {}
    plain = tuple(torch.from_numpy(x) for x in SR.render(rmeshes, inst, 3, h, w, shading="phong", ambient=0.3, background=BG, layers=layers))
    over = tuple(torch.from_numpy(x) for x in SR.render(rmeshes, inst, 3, h, w, shading="phong", ambient=0.3, background=image,
                                                       layers=layers))
    return table, poses, K, h, w, image, plain, over


def test_dirty_workspaces_and_an_empty_image_inside_a_batch(edge_scene):
    table, poses, K, h, w, image, plain, over = edge_scene
    args = (table, [1, 2, 0], [0, 0, 2], [4, 5, 6], cuda(poses), K, 3, h, w)
    assert not plain[2][1].any() and plain[2][0].any() and plain[2][2].any()
    results = []
    for fill in (0xFF, 0x00):   # the workspace may hold anything on entry; the outputs are overwritten
        ws = torch.full((shade.shade_workspace_bytes(3, 3, h, w, table),), fill, dtype=torch.uint8, device=dev())
        rgb = torch.full((3, h, w, 3), 99, dtype=torch.uint8, device=dev())
        d = torch.full((3, h, w), 7.0, dtype=torch.float32, device=dev())
        lab = torch.full((3, h, w), 9, dtype=torch.uint8, device=dev())
        vis = torch.full((3,), -5, dtype=torch.int32, device=dev())
        st = torch.full((3,), -5, dtype=torch.int32, device=dev())
        assert raw_call(*args, rgb, shading=2, ambient=0.3, depth_out=d, label_out=lab, visible=vis, status=st, ws=ws) == 0
        same((rgb, d, lab, vis, st), plain)
        results.append(rgb)
    assert torch.equal(results[0], results[1])
    assert (results[0][1].cpu() == torch.tensor(BG, dtype=torch.uint8)).all()   # the empty image is pure background
    # ... and with a background image it is that image; rgb alone is a complete call
    rgb = torch.full((3, h, w, 3), 99, dtype=torch.uint8, device=dev())
    assert raw_call(*args, rgb, shading=2, ambient=0.3, bg_image=cuda(image)) == 0
    assert torch.equal(rgb.cpu(), over[0]) and torch.equal(rgb[1].cpu(), torch.from_numpy(image[1]))
    # each optional output alone beside rgb
    vis = torch.full((3,), -5, dtype=torch.int32, device=dev())
    assert raw_call(*args, rgb, shading=2, ambient=0.3, visible=vis) == 0 and torch.equal(vis.cpu(), plain[3])
    lab = torch.full((3, h, w), 9, dtype=torch.uint8, device=dev())
    assert raw_call(*args, rgb, shading=2, ambient=0.3, label_out=lab) == 0 and torch.equal(lab.cpu(), plain[2])


def test_misaligned_outputs_and_a_pixel_count_that_is_no_multiple_of_four(edge_scene):
    table, poses, K, h, w, image, plain, over = edge_scene
    args = (table, [1, 2, 0], [0, 0, 2], [4, 5, 6], cuda(poses), K, 3, h, w)
    n = 3 * h * w
    # rgb_out and the background image at every byte offset, each also beside an aligned other; depth_out off 16 bytes, the labels off 4
    for off, bg_off in ((1, 3), (2, 2), (3, 1), (0, 1), (1, 0)):
        rgb = torch.full((n * 3 + 8,), 99, dtype=torch.uint8, device=dev())
        bg = torch.zeros((n * 3 + 8,), dtype=torch.uint8, device=dev())
        bg[bg_off:bg_off + n * 3] = cuda(image).view(-1)
        d = torch.full((n + 1,), 7.0, dtype=torch.float32, device=dev())
        lab = torch.full((n + 1,), 9, dtype=torch.uint8, device=dev())
        assert raw_call(*args, rgb[off:], shading=2, ambient=0.3, bg_image=bg[bg_off:], depth_out=d[1:], label_out=lab[1:]) == 0
        assert torch.equal(rgb[off:off + n * 3].view(3, h, w, 3).cpu(), over[0])
        assert (rgb[:off] == 99).all() and (rgb[off + n * 3:] == 99).all() and float(d[0]) == 7.0 and int(lab[0]) == 9
        assert torch.equal(d[1:].view(3, h, w).cpu().view(torch.int32), over[1].view(torch.int32))
        assert torch.equal(lab[1:].view(3, h, w).cpu(), over[2])
    # 33 x 47 = 1551 pixels: the last lane has three
    h2, w2 = 33, 47
    K2 = camera(h2, w2)
    rmeshes = [table.mesh(k) for k in range(3)]
    p = pose((1, 2, 3), 0.7, (0.13, 0.12, 0.5))[None, None]   # reaches the last rows
    for background in (BG, background_image(1, h2, w2, 3)):
        got = full(table, [0], [1], p, K2, h2, w2, shading="flat", background=cuda(background) if isinstance(background, np.ndarray)
                   else background)
        same(got, restated(rmeshes, [0], [1], p, K2, h2, w2, shading="flat", background=background))
        assert got[2][0, -1].any()


def test_no_instances_write_the_background():
    h, w = 60, 80
    K = camera(h, w)
    ball = render.icosphere(1, 0.1)
    table, _ = table_of([(*ball, smooth_colors(ball[0]))])
    none = torch.empty((2, 0, 3, 4), dtype=torch.float64, device=dev())
    rgb = torch.full((2, h, w, 3), 99, dtype=torch.uint8, device=dev())
    d = torch.full((2, h, w), 7.0, dtype=torch.float32, device=dev())
    lab = torch.full((2, h, w), 9, dtype=torch.uint8, device=dev())
    got = shade.render_color(table, [], [], none, K, h, w, background=BG, out_rgb=rgb, out_depth=d, out_labels=lab, return_visible=True,
                             return_status=True)
    assert got[0].data_ptr() == rgb.data_ptr() and (rgb.cpu() == torch.tensor(BG, dtype=torch.uint8)).all() and not d.any() and not lab.any()
    assert tuple(got[3].shape) == (2, 0) and tuple(got[4].shape) == (2, 0)
    image = cuda(background_image(2, h, w))
    assert torch.equal(shade.render_color(table, [], [], none, K, h, w, background=image)[0], image)
    empty = shade.render_color(table, [0], [1], torch.empty((0, 1, 3, 4), dtype=torch.float64, device=dev()), K, h, w)
    assert tuple(empty[0].shape) == (0, h, w, 3) and tuple(empty[1].shape) == (0, h, w)
    p = cuda(pose((1, 2, 3), 0.7, (0.0, 0.0, 0.5))[None, None])
    for bad in (dict(shading="gouraud"), dict(ambient=-0.1), dict(ambient=float("nan")), dict(background=(1, 2)), dict(background=(1, 2, 256)),
                dict(background=image), dict(max_instances=0), dict(far=0.0)):
        with pytest.raises(RuntimeError):
            shade.render_color(table, [0], [1], p, K, h, w, **bad)
    with pytest.raises(RuntimeError):
        shade.render_color(table, [0], [1], p.cpu(), K, h, w)                                # a CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        shade.render_color(render.DeviceMeshes([ball]), [0], [1], p, K, h, w)                # no colours


def test_reproducible_and_graph_capture_and_replay():
    h, w = 60, 80
    K = cuda(camera(h, w))
    meshes, ids, labels, base = crossing_bars()
    table, rmeshes = table_of(meshes)
    all_poses = []
    for k in range(2):
        p = base.copy()
        p[1, :, 0, 3] += 0.01 * (k + 1)
        p[:, 2, 2, 3] += 0.03 * k
        all_poses.append(p)
    image = cuda(background_image(2, h, w))
    kw = dict(shading="phong", ambient=0.25, background=image)
    a = full(table, ids, labels, all_poses[0], K, h, w, **kw)
    b = full(table, ids, labels, all_poses[0], K, h, w, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    static = cuda(all_poses[0])
    rgb = torch.full((2, h, w, 3), 99, dtype=torch.uint8, device=dev())
    d = torch.full((2, h, w), 9.0, dtype=torch.float32, device=dev())
    lab = torch.full((2, h, w), 9, dtype=torch.uint8, device=dev())
    ws = torch.empty(shade.shade_workspace_bytes(6, 2, h, w, table), dtype=torch.uint8, device=dev())
    out = dict(out_rgb=rgb, out_depth=d, out_labels=lab, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the table's upload and a first call outside the capture
        shade.render_color(table, ids, labels, static, K, h, w, **kw, **out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        shade.render_color(table, ids, labels, static, K, h, w, **kw, **out)
    for p in all_poses[1:] + all_poses[:1]:   # replayed twice
        static.copy_(cuda(p))
        rgb.fill_(99)
        d.fill_(9.0)
        lab.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        eager = shade.render_color(table, ids, labels, cuda(p), K, h, w, **kw)
        assert torch.equal(rgb, eager[0]) and torch.equal(d, eager[1]) and torch.equal(lab, eager[2])
    want = restated(rmeshes, ids, labels, all_poses[0], camera(h, w), h, w, shading="phong", ambient=0.25, background=image.cpu().numpy())
    assert torch.equal(rgb.cpu(), want[0]) and torch.equal(lab.cpu(), want[2])


def test_a_call_split_between_images_equals_the_unsplit_restatement():
    h, w = 48, 64
    K = camera(h, w)
    shapes = [render.icosphere(1, 0.08), render.box_mesh(0.15, 0.1, 0.2)]
    table, rmeshes = table_of([(*m, smooth_colors(m[0], k)) for k, m in enumerate(shapes)])
    rng = np.random.default_rng(4)
    poses = np.stack([pose(rng.normal(size=3), rng.uniform(0, 3), (rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(0.4, 0.8)))
                      for _ in range(6)]).reshape(3, 2, 3, 4)
    image = background_image(3, h, w)
    want = restated(rmeshes, [0, 1], [5, 6], poses, K, h, w, shading="flat", ambient=0.4, background=image)
    assert all(want[2][i].any() for i in range(3))
    for chunk in (2, 3, 4, 5, _abi.SHADE_MAX_INSTANCES):   # one image per call (2, 3), two and one (4, 5), all three
        same(full(table, [0, 1], [5, 6], poses, K, h, w, shading="flat", ambient=0.4, background=cuda(image), max_instances=chunk), want)
    with pytest.raises(RuntimeError):   # one image with more instances than a call takes
        full(table, [0, 1], [5, 6], poses, K, h, w, max_instances=1)
    with pytest.raises(RuntimeError):
        full(table, [0, 1], [5, 6], poses, K, h, w, max_instances=_abi.SHADE_MAX_INSTANCES + 1)


def test_hand_over_to_the_augmentation():
    from pvnet_amd import augment as A
    h, w = 60, 80
    K = camera(h, w)
    meshes, ids, labels, poses = crossing_bars()
    table, _ = table_of(meshes)
    image = cuda(background_image(2, h, w))
    rgb, _, lab = shade.render_color(table, ids, labels, cuda(poses), K, h, w, background=image)
    assert rgb.is_contiguous() and tuple(rgb.shape) == (2, h, w, 3) and lab.any()
    hc = torch.ones((2, 4, 3), dtype=torch.float64, device=dev())
    out, mask, _, status = A.augment_batch(rgb, lab, hc, h, w, A.AugmentConfig.identity(), A.draw_uniforms(2, torch.Generator().manual_seed(1)), 0)
    assert status.tolist() == [0, 0]
    visible = depth.render_visible_labels(table, ids, labels, cuda(poses), K, h, w)
    _, want_mask, _, _ = A.augment_batch(rgb, visible, hc, h, w, A.AugmentConfig.identity(),
                                         A.draw_uniforms(2, torch.Generator().manual_seed(1)), 0)
    assert torch.equal(mask, want_mask) and mask.any()
    assert torch.equal(out, A.normalize_batch(rgb))
