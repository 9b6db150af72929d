"""GPU tests of the z-buffered mesh renderer (pvnet_amd/depth.py, libpvnet_depth.so) against THE DEFINITION of include/pvnet_depth.h as
tests/depth_restatement.py restates it, against the silhouettes of libpvnet_raster.so and against what the reference's own
``get_mask_of_all_objects`` recorded (tests/golden/depth.npz).  Every comparison with the restatement is ``torch.equal`` on the float32
bits, the labels, the visible counts and the status.

Shapes are the smallest at which the kernels can go wrong: 48 x 64 and 33 x 47 (a pixel count that is no multiple of 4: the resolve
kernel's tail), boxes of 64 and 65 pixels (the constant between the lane's own walk and the cooperative path), 8 x 8 images for the call
that has to be split, 480 x 640 once for the recorded case."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pvnet_amd import _abi, depth, render, synth
from tests import depth_restatement as DR
from tests import raster_restatement as RS
from tests.render_cases import camera, coop_count, cuda, dev, pose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(48, 64), (33, 47)]
MESHES = [render.box_mesh(0.15, 0.1, 0.2), render.l_prism_mesh(0.2, 0.08), render.icosphere(1, 0.1), render.icosphere(2, 0.1)]


def restated(meshes, mesh_ids, labels, poses, K, h, w, far=np.inf):
    """tests/depth_restatement.py for poses [b,m,3,4] -> (depth, labels, visible [b,m], status [b,m]) as CPU tensors"""
    b, m = poses.shape[:2]
    inst = [(mesh_ids[j], poses[i, j], K, i, labels[j]) for i in range(b) for j in range(m)]
    d, lab, vis, st = DR.render(meshes, inst, b, h, w, far)
    return torch.from_numpy(d), torch.from_numpy(lab), torch.from_numpy(vis).view(b, m), torch.from_numpy(st).view(b, m)


def same(got, want):
    """(depth, labels, visible, status) from the device against the restatement: the float32 BITS, and everything else"""
    gd, gl, gv, gs = (x.cpu() for x in got)
    wd, wl, wv, ws = want
    assert gd.dtype == torch.float32 and gl.dtype == torch.uint8 and gv.dtype == torch.int32 and gs.dtype == torch.int32
    assert torch.equal(gd.view(torch.int32), wd.view(torch.int32))
    assert torch.equal(gl, wl) and torch.equal(gv, wv) and torch.equal(gs, ws)
    assert torch.equal(gd != 0, gl != 0)


def full(table, mesh_ids, labels, poses, K, h, w, **kw):
    return depth.render_depth(table, mesh_ids, labels, cuda(poses), K, h, w, return_visible=True, return_status=True, **kw)


@pytest.mark.parametrize("size", SIZES)
def test_one_instance_per_image(size):
    h, w = size
    K = camera(h, w)
    table = render.DeviceMeshes(MESHES)
    poses = np.stack([pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5)),      # inside the frame
                      pose((3, -1, 2), 2.1, (-0.27, 0.14, 0.5)),     # cut by the border
                      pose((0, 1, 0), 0.3, (1.5, 0.0, 0.5)),         # wholly outside
                      pose((2, 1, -1), 1.2, (0.04, 0.03, 0.8))])[:, None]
    for k in range(len(MESHES)):
        got = full(table, [k], [k + 1], poses, K, h, w)
        same(got, restated(MESHES, [k], [k + 1], poses, K, h, w))
        masks = render.render_masks(table, k, cuda(poses[:, 0]), K, h, w)
        assert torch.equal(got[0] != 0, masks != 0) and torch.equal(got[1], masks * (k + 1))
        assert torch.equal(got[2].view(-1).cpu(), masks.sum((1, 2)).to(torch.int32).cpu()) and not got[3].any()
        assert got[0][0].any() and got[0][1].any() and not got[0][2].any()


def crossing_bars():
    """two bars through each other (one end of each nearer) and a sphere in front of one end: [1,3,3,4] poses, meshes, ids, labels"""
    meshes = [render.box_mesh(0.25, 0.06, 0.05), render.icosphere(2, 0.04)]
    poses = np.stack([pose((0, 1, 0), 0.5, (-0.02, -0.01, 0.5)), pose((0.1, 1, 0), -0.4, (-0.015, -0.005, 0.505)),
                      pose((1, 1, 0), 0.3, (0.08, 0.0, 0.42))])[None]
    return meshes, [0, 0, 1], [1, 2, 3], poses


@pytest.mark.parametrize("size", SIZES)
def test_interpenetrating_instances_differ_from_every_painters_order(size):
    h, w = size
    K = camera(h, w)
    meshes, ids, labels, poses = crossing_bars()
    want = restated(meshes, ids, labels, poses, K, h, w)
    inst = [(ids[j], poses[0, j], K, 0, labels[j]) for j in range(3)]
    centroid, _, _ = RS.render(meshes, inst, 1, h, w, order=RS.centroid_order(meshes, ids, poses[0]))
    assert (centroid[0] != want[1][0].numpy()).sum() >= 1          # on the restatement first
    for order in ([0, 1, 2], [1, 0, 2]):                           # and neither order of the two bars gives it
        painted, _, _ = RS.render(meshes, inst, 1, h, w, order=order)
        assert (painted[0] != want[1][0].numpy()).sum() >= 1
    table = render.DeviceMeshes(meshes)
    got = full(table, ids, labels, poses, K, h, w)
    same(got, want)
    assert set(torch.unique(got[1]).cpu().tolist()) == {0, 1, 2, 3}
    painted = render.render_labels(table, ids, labels, cuda(poses), K, h, w)
    assert np.array_equal(painted.cpu().numpy(), centroid) and int((painted != got[1]).sum()) >= 1
    assert torch.equal(depth.render_visible_labels(table, ids, labels, cuda(poses), K, h, w), got[1])


def test_ties_go_to_the_earlier_instance():
    h, w = 48, 64
    K = camera(h, w)
    table = render.DeviceMeshes(MESHES)
    p = pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5))
    poses = np.stack([p, p.copy()])[None]
    for labels in ([3, 7], [7, 3]):
        got = full(table, [1, 1], labels, poses, K, h, w)
        same(got, restated(MESHES, [1, 1], labels, poses, K, h, w))
        covered = got[1][got[1] != 0]
        assert covered.numel() > 50 and (covered == labels[0]).all()
        assert got[2].cpu().tolist() == [[covered.numel(), 0]]


def test_far_cuts_through_a_sphere():
    h, w = 48, 64
    K = camera(h, w)
    table = render.DeviceMeshes(MESHES)
    poses = pose((1, 0, 1), 0.3, (0.01, 0.0, 0.5))[None, None]
    whole = full(table, [3], [9], poses, K, h, w)
    cut = full(table, [3], [9], poses, K, h, w, far=0.43)          # the sphere's front is at 0.4, its rim at 0.5
    same(cut, restated(MESHES, [3], [9], poses, K, h, w, far=0.43))
    assert 0 < int(cut[2]) < int(whole[2]) and float(cut[0].max()) < 0.43 and float(whole[0].max()) > 0.43
    dropped = (whole[0] != 0) & (cut[0] == 0)
    assert dropped.any() and (whole[0][dropped] >= 0.43).all() and (cut[1][dropped] == 0).all()
    kept = cut[0] != 0
    assert torch.equal(cut[0][kept], whole[0][kept])
    nothing = full(table, [3], [9], poses, K, h, w, far=0.3)
    assert not nothing[0].any() and not nothing[1].any() and int(nothing[2]) == 0
    with pytest.raises(RuntimeError):
        depth.render_depth(table, [3], [9], cuda(poses), K, h, w, far=0.0)
    with pytest.raises(RuntimeError):
        depth.render_depth(table, [3], [9], cuda(poses), K, h, w, far=float("nan"))


def test_the_recorded_reference_composition_at_far_10():
    G = np.load(os.path.join(ROOT, "tests", "golden", "depth.npz"))
    h, w = (int(x) for x in G["size"])
    names = [str(m) for m in G["instance_mesh"]]
    uniq = sorted(set(names))
    meshes = [(G[f"mesh.{m}.vertices"], G[f"mesh.{m}.faces"]) for m in uniq]
    ids, labels = [uniq.index(m) for m in names], [int(x) for x in G["instance_label"]]
    table = render.DeviceMeshes(meshes)
    order = [int(i) for i in G["orders"][0]]
    poses = G["poses"][order][None]
    got = full(table, [ids[i] for i in order], [labels[i] for i in order], poses, G["K"], h, w, far=float(G["far"]))
    assert np.array_equal(got[1][0].cpu().numpy(), G["labels_ref"][0])
    same(got, restated(meshes, [ids[i] for i in order], [labels[i] for i in order], poses, G["K"], h, w, far=float(G["far"])))
    assert float(got[0].max()) < 10.0 and int(got[2][0, order.index(5)]) == 0   # the wall beyond 10 wins nothing
    # the other list order: the tie goes the other way (the labels alone)
    order = [int(i) for i in G["orders"][1]]
    lab = depth.render_visible_labels(table, [ids[i] for i in order], [labels[i] for i in order], cuda(G["poses"][order][None]), G["K"], h, w,
                                      far=float(G["far"]))
    assert np.array_equal(lab[0].cpu().numpy(), G["labels_ref"][1])


def screen_mesh(tri_px, zs, K):
    """a one-face mesh whose vertices project to the given pixel coordinates at the given camera z (identity pose)"""
    v = [((u - K[0, 2]) / K[0, 0] * z, (y - K[1, 2]) / K[1, 1] * z, z) for (u, y), z in zip(tri_px, zs)]
    return np.asarray(v, np.float64), np.array([[0, 1, 2]], np.int32)


def test_both_kernel_paths_in_one_image_and_the_constant_between_them():
    h, w = 48, 64
    K = camera(h, w)
    eye = pose((0, 0, 1), 0.0, (0, 0, 0))
    sphere = render.icosphere(3, 0.1)   # 1 280 small faces
    # one large triangle, tilted: in front of the sphere's left part and behind its right part
    big = screen_mesh([(-20.0, -30.0), (90.0, 20.0), (-20.0, 70.0)], [0.36, 0.62, 0.36], K)
    meshes = [sphere, big]
    table = render.DeviceMeshes(meshes)
    poses = np.stack([pose((1, 2, 3), 0.4, (0.0, 0.0, 0.5)), eye])[None]
    ws = torch.empty(depth.depth_workspace_bytes(2, 1, h, w, table), dtype=torch.uint8, device=dev())
    for ids, labels, p in (([0, 1], [1, 2], poses), ([1, 0], [2, 1], poses[:, ::-1])):
        got = full(table, ids, labels, p, K, h, w, workspace=ws)
        same(got, restated(meshes, ids, labels, p, K, h, w))
        assert coop_count(ws) == 1
        on_sphere = render.render_masks(table, 0, cuda(p[0, ids.index(0)][None]), K, h, w)[0] != 0
        seen = got[1][0][on_sphere]
        assert (seen == 1).sum() > 50 and (seen == 2).sum() > 50   # both reach the same pixels, and each wins some
    # boxes of 64 (8 x 8) and 65 (5 x 13) pixels: the second alone takes the cooperative path
    assert _abi.DEPTH_LANE_PIXELS == 64
    for (bw, bh), coop in (((8, 8), 0), ((5, 13), 1)):
        mesh = screen_mesh([(2.5, 2.5), (2.5 + bw - 2, 2.5), (2.5, 2.5 + bh - 2)], [0.5, 0.6, 0.7], K)
        tri, _ = RS.project_triangles(*mesh, eye, K)
        box = DR.triangle_box(tri[0], h, w)
        assert (box[1] - box[0] + 1, box[3] - box[2] + 1) == (bw, bh)
        t1 = render.DeviceMeshes([mesh])
        ws1 = torch.empty(depth.depth_workspace_bytes(1, 1, h, w, t1), dtype=torch.uint8, device=dev())
        got = full(t1, [0], [5], eye[None, None], K, h, w, workspace=ws1)
        same(got, restated([mesh], [0], [5], eye[None, None], K, h, w))
        assert got[0].any() and coop_count(ws1) == coop, (bw, bh)


def test_behind_the_camera_and_non_finite():
    h, w = 48, 64
    K = camera(h, w)
    meshes = [render.icosphere(2, 0.1), render.box_mesh(0.2, 0.2, 0.6)]
    table = render.DeviceMeshes(meshes)
    poses = np.stack([pose((1, 0, 1), 1.3, (0.01, 0.02, 0.03)),      # the camera inside the sphere
                      pose((1, 0, 0), 0.2, (0.05, 0.02, 0.2))])[None]   # a box from z = -0.1 to 0.5: it straddles the camera plane
    want = restated(meshes, [0, 1], [1, 2], poses, K, h, w)
    got = full(table, [0, 1], [1, 2], poses, K, h, w)
    same(got, want)
    assert (got[3].cpu() & DR.S_BEHIND).all() and got[0].any()       # the triangles wholly in front are drawn
    assert float(got[0][got[0] != 0].min()) > 0
    for k in (0, 1):   # alone: status is per instance
        same(full(table, [k], [k + 1], poses[:, k:k + 1], K, h, w), restated(meshes, [k], [k + 1], poses[:, k:k + 1], K, h, w))
    bad = poses.copy()
    bad[0, 0, 1, 2] = np.nan
    got = full(table, [0, 1], [1, 2], bad, K, h, w)
    same(got, restated(meshes, [0, 1], [1, 2], bad, K, h, w))
    assert int(got[3][0, 0]) & DR.S_NONFINITE and int(got[2][0, 0]) == 0 and not (got[1] == 1).any()
    whole = pose((1, 0, 0), 0.2, (0.0, 0.0, 0.5))[None, None].copy()
    whole[0, 0, 2, 3] = np.nan   # camera z itself is NaN: nothing is drawn, both bits
    got = full(table, [0], [1], whole, K, h, w)
    assert not got[0].any() and not got[1].any() and int(got[3]) == DR.S_NONFINITE | DR.S_BEHIND
    same(got, restated(meshes, [0], [1], whole, K, h, w))


def raw_call(table, mesh_ids, image_ids, labels, poses, K, b, h, w, far=np.inf, depth_out=None, label_out=None, visible=None, status=None,
             ws=None):
    """pvnet_render_depth itself: an instance list the front end cannot express (an image without instances), single outputs"""
    lib = _abi.load_depth_library()
    vertices, faces, _ = table.on(dev())
    q = len(mesh_ids)
    arr = lambda vals: (C.c_int32 * max(q, 1))(*vals)   # noqa: E731
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    if ws is None:
        ws = torch.empty(depth.depth_workspace_bytes(q, b, h, w, table), dtype=torch.uint8, device=dev())
    Kd = cuda(K)
    rc = lib.pvnet_render_depth(ptr(vertices), ptr(faces), table._c_voff, table._c_foff, table.count, table.total_vertices,
                                table.total_faces, q, arr(mesh_ids), ptr(poses), ptr(Kd), 0, arr(image_ids), arr(labels), b, h, w, far,
                                ptr(depth_out), ptr(label_out), ptr(visible), ptr(status), ptr(ws), ws.numel(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("size", SIZES)
def test_workspace_and_batch_edges(size):
    h, w = size
    K = camera(h, w)
    table = render.DeviceMeshes(MESHES)
    poses = np.stack([pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5)), pose((2, 1, -1), 1.2, (0.04, 0.03, 0.6)),
                      pose((3, -1, 2), 2.1, (-0.1, 0.05, 0.55))])
    # an image without instances in the middle of a batch: instances in images 0, 0 and 2 of three
    inst = [(1, poses[0], K, 0, 4), (3, poses[1], K, 0, 5), (0, poses[2], K, 2, 6)]
    wd, wl, wv, wst = (torch.from_numpy(x) for x in DR.render(MESHES, inst, 3, h, w))
    assert not wl[1].any() and wl[0].any() and wl[2].any()
    results = []
    for fill in (0xFF, 0x00):   # the workspace may hold anything on entry; the outputs are overwritten
        ws = torch.full((depth.depth_workspace_bytes(3, 3, h, w, table),), fill, dtype=torch.uint8, device=dev())
        d = torch.full((3, h, w), 7.0, dtype=torch.float32, device=dev())
        lab = torch.full((3, h, w), 9, dtype=torch.uint8, device=dev())
        vis = torch.full((3,), -5, dtype=torch.int32, device=dev())
        st = torch.full((3,), -5, dtype=torch.int32, device=dev())
        assert raw_call(table, [1, 3, 0], [0, 0, 2], [4, 5, 6], cuda(poses), K, 3, h, w, depth_out=d, label_out=lab, visible=vis, status=st,
                        ws=ws) == 0
        assert torch.equal(d.cpu().view(torch.int32), wd.view(torch.int32)) and torch.equal(lab.cpu(), wl)
        assert torch.equal(vis.cpu(), wv) and torch.equal(st.cpu(), wst)
        results.append((d, lab))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    # each output alone
    d = torch.full((3, h, w), 7.0, dtype=torch.float32, device=dev())
    assert raw_call(table, [1, 3, 0], [0, 0, 2], [4, 5, 6], cuda(poses), K, 3, h, w, depth_out=d) == 0
    assert torch.equal(d, results[0][0])
    lab = torch.full((3, h, w), 9, dtype=torch.uint8, device=dev())
    assert raw_call(table, [1, 3, 0], [0, 0, 2], [4, 5, 6], cuda(poses), K, 3, h, w, label_out=lab) == 0
    assert torch.equal(lab, results[0][1])
    vis = torch.full((3,), -5, dtype=torch.int32, device=dev())
    assert raw_call(table, [1, 3, 0], [0, 0, 2], [4, 5, 6], cuda(poses), K, 3, h, w, label_out=lab, visible=vis) == 0
    assert torch.equal(vis.cpu(), wv)
    # an output that starts at an odd element: the scalar stores
    d = torch.full((3 * h * w + 1,), 7.0, dtype=torch.float32, device=dev())
    lab = torch.full((3 * h * w + 1,), 9, dtype=torch.uint8, device=dev())
    assert raw_call(table, [1, 3, 0], [0, 0, 2], [4, 5, 6], cuda(poses), K, 3, h, w, depth_out=d[1:], label_out=lab[1:]) == 0
    assert torch.equal(d[1:].view(3, h, w), results[0][0]) and torch.equal(lab[1:].view(3, h, w), results[0][1])
    assert float(d[0]) == 7.0 and int(lab[0]) == 9
    # q == 0: zeros, whatever the outputs held; b == 0: empty results
    d = torch.full((2, h, w), 7.0, dtype=torch.float32, device=dev())
    lab = torch.full((2, h, w), 9, dtype=torch.uint8, device=dev())
    none = torch.empty((2, 0, 3, 4), dtype=torch.float64, device=dev())
    got = depth.render_depth(table, [], [], none, K, h, w, out_depth=d, out_labels=lab, return_visible=True, return_status=True)
    assert got[0].data_ptr() == d.data_ptr() and got[1].data_ptr() == lab.data_ptr() and not d.any() and not lab.any()
    assert tuple(got[2].shape) == (2, 0) and tuple(got[3].shape) == (2, 0)
    empty = depth.render_depth(table, [0], [1], torch.empty((0, 1, 3, 4), dtype=torch.float64, device=dev()), K, h, w)
    assert tuple(empty[0].shape) == (0, h, w) and tuple(empty[1].shape) == (0, h, w)
    with pytest.raises(RuntimeError):
        depth.render_depth(table, [0], [1], torch.zeros((1, 1, 3, 4), dtype=torch.float64), K, h, w)   # a CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        depth.render_depth(table, [0], [256], cuda(poses[:1, None]), K, h, w)


def test_visible_counts():
    h, w = 48, 64
    K = camera(h, w)
    meshes, ids, _, poses = crossing_bars()
    table = render.DeviceMeshes(meshes)
    poses = np.concatenate([poses, poses[:, ::-1]])   # b = 2
    labels = [4, 4, 2]                                  # two instances share one label: counted separately
    got = full(table, ids, labels, poses[:1], K, h, w)
    same(got, restated(meshes, ids, labels, poses[:1], K, h, w))
    assert int(got[2].sum()) == int((got[1] != 0).sum()) and (got[2] > 0).all()
    assert int(got[2][0, 0] + got[2][0, 1]) == int((got[1] == 4).sum())
    ids2 = [0, 1, 0]
    got = full(table, ids2, labels, np.stack([poses[0], poses[0][[0, 2, 1]]]), K, h, w)
    assert torch.equal(got[2].sum(1).cpu(), (got[1] != 0).sum((1, 2)).to(torch.int32).cpu())


def test_reproducible_and_graph_capture_and_replay():
    h, w = 33, 47
    K = cuda(camera(h, w))
    meshes, ids, labels, base = crossing_bars()
    table = render.DeviceMeshes(meshes)
    all_poses = []
    for k in range(3):
        p = np.concatenate([base, base])
        p[1, :, 0, 3] += 0.01 * (k + 1)
        p[:, 2, 2, 3] += 0.03 * k
        all_poses.append(p)
    a = full(table, ids, labels, all_poses[0], K, h, w)
    b = full(table, ids, labels, all_poses[0], K, h, w)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    static = cuda(all_poses[0])
    d = torch.full((2, h, w), 9.0, dtype=torch.float32, device=dev())
    lab = torch.full((2, h, w), 9, dtype=torch.uint8, device=dev())
    ws = torch.empty(depth.depth_workspace_bytes(6, 2, h, w, table), dtype=torch.uint8, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the table's upload and a first call outside the capture
        depth.render_depth(table, ids, labels, static, K, h, w, out_depth=d, out_labels=lab, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        depth.render_depth(table, ids, labels, static, K, h, w, out_depth=d, out_labels=lab, workspace=ws)
    for p in all_poses[1:] + all_poses[:1]:
        static.copy_(cuda(p))
        d.fill_(9.0)
        lab.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        eager = depth.render_depth(table, ids, labels, cuda(p), K, h, w)
        assert torch.equal(d, eager[0]) and torch.equal(lab, eager[1])
        wd, wl, _, _ = restated(meshes, ids, labels, p, camera(h, w), h, w)
        assert torch.equal(d.cpu().view(torch.int32), wd.view(torch.int32)) and torch.equal(lab.cpu(), wl)


def test_more_instances_than_one_call_takes():
    h = w = 8
    K = camera(h, w)
    mesh = render.box_mesh(0.15, 0.1, 0.2)
    table = render.DeviceMeshes([mesh])
    rng = np.random.default_rng(4)
    distinct = np.stack([pose(rng.normal(size=3), rng.uniform(0, 3), (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 0.8)))
                         for _ in range(16)])
    # m = 1: 800 images, 768 + 32;  m = 3: 260 images, 256 + 4 (an image's instances stay in one call)
    for m, b in ((1, 800), (3, 260)):
        assert b * m > _abi.DEPTH_MAX_INSTANCES
        unit = np.stack([distinct[(np.arange(m) + i) % 16] for i in range(16)])           # [16,m,3,4]
        want = restated([mesh], [0] * m, list(range(1, m + 1)), unit, K, h, w)
        reps = -(-b // 16)
        poses = np.concatenate([unit] * reps)[:b]
        got = full(table, [0] * m, list(range(1, m + 1)), poses, K, h, w)
        same(got, tuple(torch.cat([x] * reps)[:b] for x in want))
        assert got[1].any()


def test_hand_over_from_the_pose_solve_and_to_the_class_vote():
    from pvnet_amd import pnp, validation, voting
    h, w = 120, 160
    K = camera(h, w)
    meshes = [render.icosphere(2, 0.07), render.box_mesh(0.12, 0.09, 0.1), render.l_prism_mesh(0.16, 0.07)]
    table = render.DeviceMeshes(meshes)
    poses = np.stack([pose((1, 2, 3), 0.8, (-0.06, -0.02, 0.6)), pose((2, -1, 1), 2.0, (0.02, -0.01, 0.55)),
                      pose((0, 1, 1), 0.6, (0.0, 0.03, 0.5))])[None]   # they overlap
    # pnp_batch_device's float64 poses are read in place
    lo, hi = meshes[1][0].min(0), meshes[1][0].max(0)
    kp3 = np.array([(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])] + [(0.0, 0.0, 0.0)])
    kp2 = np.stack(RS.project_points(kp3, poses[0, 1], K)[:2], -1).astype(np.float64)[None]
    solved, status = pnp.pnp_batch_device(kp3, cuda(kp2), K)
    assert (status.cpu() >= 0).all() and solved.dtype == torch.float64 and tuple(solved.shape) == (1, 3, 4)
    handed = solved.view(1, 1, 3, 4)
    assert handed.data_ptr() == solved.data_ptr()
    got = depth.render_depth(table, [1], [2], handed, K, h, w, return_visible=True, return_status=True)
    same(got, restated(meshes, [1], [2], solved.cpu().numpy()[None], K, h, w))
    assert int(got[2]) > 300
    # the label image is a valid input of the class vote
    labels = depth.render_visible_labels(table, [0, 1, 2], [1, 2, 3], cuda(poses), K, h, w)
    assert set(torch.unique(labels).cpu().tolist()) == {0, 1, 2, 3}
    vn = 4
    field = torch.zeros((1, 2 * vn, h, w), dtype=torch.float32, device=dev())
    masks = []
    for k in range(3):
        mk = (labels == k + 1).to(torch.uint8)
        pts = np.concatenate([meshes[k][0][:vn - 1], np.zeros((1, 3))])
        hc = np.stack(RS.project_points(pts, poses[0, k], K)[:2], -1).astype(np.float64)
        vert, _ = validation.vertex_targets_device(mk, cuda(np.concatenate([hc, np.ones((vn, 1))], -1)[None]))
        field += vert
        masks.append(mk[0])
    view = synth.planar_to_vertex_view(field)
    voted = voting.ransac_voting_layer_v2(labels, view, 4, 64, inlier_thresh=0.99, seed=5)
    want = voting.ransac_voting_layer_v3(torch.stack(masks), view.expand(3, h, w, vn, 2), 64, inlier_thresh=0.99, seed=5)
    assert tuple(voted.shape) == (1, 3, vn, 2) and torch.equal(voted[0], want)


def test_render_mesh_depth_is_the_reference_call_form():
    h, w = 33, 47
    K = camera(h, w)
    v, f = MESHES[1]
    p = pose((1, 2, 3), 0.7, (0.02, -0.01, 0.5))
    got = depth.render_mesh_depth(p, K, v, f, h, w)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (h, w) and got.any()
    table = render.DeviceMeshes([(v, f)])
    d, _ = depth.render_depth(table, [0], [1], cuda(p[None, None]), K, h, w)
    assert np.array_equal(got.view(np.uint32), d[0].cpu().numpy().view(np.uint32))
    assert np.array_equal(got.view(np.uint32), DR.instance_depth(v, f, p, K, h, w)[0].view(np.uint32))
