"""GPU tests of the pose solve per class (pnp.pnp_classes_device -> pvnet_pose_solve_classes, pvnet_amd/csrc/pose_classes.hip;
voting.MultiPoseEvalWrapper) on the shared cases of tests/pose_classes_cases.py.

THE DEFINITION is the loop the call replaces: ``pnp_batch_device`` class by class on ``points_2d[:, k]`` with ``points_3d[k]``.  Both
kernels compile the one copy of the solver (pvnet_amd/csrc/pose_core.h) without contraction, so the comparison is ``torch.equal``: a
difference is a finding about the shared core (a contraction, another expansion of a division in one of the two kernels), to be read
from their assembly, and is not bridged with a tolerance.  The independent oracle is the host library class by class, under
tests/test_pose_device.py's ATOL, and on noise-free cases the ground-truth poses under pose_cases.BAR_POSE.

One wave per item and at most 26 items per case; the route tests run at 120 x 160 with three small meshes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pvnet_amd import _abi
from pvnet_amd import pnp as P
from tests import pose_cases
from tests import pose_classes_cases as CC

pytestmark = pytest.mark.gpu

ATOL = 1e-8   # tests/test_pose_device.py's: every [R|t] entry, device against host
# rt against pose_cases.poses_to_rt of the poses: both outputs are one pose, the poses' rotation entries are rounded to 1 ulp
# (2.2e-16 of entries <= 1) and the host's matrix -> quaternion -> angle-axis conversion divides by a quaternion norm >= 0.5 and takes
# one atan2: a few hundred ulp at worst, 1e-13; the bar is ten times that and 1e4 times below ATOL
RT_ATOL = 1e-12
layouts = pytest.mark.parametrize("layout", CC.LAYOUTS, ids=lambda l: "x".join(map(str, l)))


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def loop(X, pts, K, W=None, cov=None):
    """the definition: pnp_batch_device class by class -> (poses [b,nk,3,4], status [b,nk]) on the device"""
    poses, status = [], []
    for k in range(pts.shape[1]):
        kw = {}
        if W is not None:
            kw["weights_2d"] = W[:, k]
        if cov is not None:
            kw["covariance"] = cov[:, k]
        p, s = P.pnp_batch_device(X[k], pts[:, k], K, **kw)
        poses.append(p)
        status.append(s)
    return torch.stack(poses, 1), torch.stack(status, 1)


def same(got, want):
    torch.cuda.synchronize()
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32
    assert tuple(got[0].shape) == tuple(want[0].shape) and tuple(got[1].shape) == tuple(want[1].shape)
    assert torch.equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())
    assert torch.equal(got[0], want[0]), float((got[0] - want[0]).abs().max())


@functools.lru_cache(maxsize=None)
def noisy(layout):
    X, x2, gt = CC.case(*layout, noise=CC.NOISE)
    return X, x2, gt


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
@layouts
def test_equals_the_loop_for_f64_f32_and_strided_keypoints(layout):
    b, nk, pn = layout
    X, x2, _ = noisy(layout)
    Xd = up(X)
    for pts in (up(x2), up(x2.astype(np.float32))):
        got = P.pnp_classes_device(Xd, pts, P.LINEMOD_K)
        same(got, loop(Xd, pts, P.LINEMOD_K))
        assert (got[1] >= 0).all() and got[0].abs().sum() > 0
    flat = P.pnp_classes_device(Xd, up(x2.astype(np.float32)), P.LINEMOD_K)
    # a slice of a wider tensor, the gaps poisoned: [b,nk,pn,2] out of [b,nk+1,pn+2,4]
    wide = torch.full((b, nk + 1, pn + 2, 4), float("nan"), dtype=torch.float32, device=dev())
    wide[:, :nk, 1:pn + 1, 1::2] = up(x2.astype(np.float32))
    view = wide[:, :nk, 1:pn + 1, 1::2]
    assert not view.is_contiguous()
    same(P.pnp_classes_device(Xd, view, P.LINEMOD_K), flat)
    # a [nk,b,pn,2] tensor permuted: the class stride is the larger one
    perm = up(x2.astype(np.float32).transpose(1, 0, 2, 3)).permute(1, 0, 2, 3)
    assert tuple(perm.shape) == (b, nk, pn, 2) and (nk == 1 or b == 1 or not perm.is_contiguous())
    same(P.pnp_classes_device(Xd, perm, P.LINEMOD_K), flat)
    # a list of point sets, from numpy
    same(P.pnp_classes_device([X[k] for k in range(nk)], perm, P.LINEMOD_K), flat)


@layouts
def test_equals_the_loop_with_cameras_per_image_weights_and_covariances(layout):
    b, nk, pn = layout
    X, x2, _ = noisy(layout)
    Xd, pts = up(X), up(x2)
    Ks = up(CC.cameras(b))
    got = P.pnp_classes_device(Xd, pts, Ks)
    same(got, loop(Xd, pts, Ks))
    if b > 1:   # the cameras differ, and it shows
        assert not torch.equal(got[0], P.pnp_classes_device(Xd, pts, P.LINEMOD_K)[0])
    W = up(CC.weights(b, nk, pn))
    same(P.pnp_classes_device(Xd, pts, Ks, weights_2d=W), loop(Xd, pts, Ks, W=W))
    cov = up(CC.covariances(b, nk, pn))
    assert float(cov[0, 0, 1, 0, 0]) < 1e-6 and torch.isnan(cov[-1, -1, 3]).any()
    got = P.pnp_classes_device(Xd, pts, P.LINEMOD_K, covariance=cov)
    same(got, loop(Xd, pts, P.LINEMOD_K, cov=cov))
    assert torch.isfinite(got[0]).all() and (got[1] >= 0).all()


def raw(X, pts, K, vote_status=None, want_rt=True, want_poses=True):
    """pvnet_pose_solve_classes through ctypes (pnp_classes_device always passes rt = NULL); the outputs start as sentinels"""
    b, nk, pn = pts.shape[:3]
    rt = torch.full((b, nk, 6), 7.0, dtype=torch.float64, device=dev())
    poses = torch.full((b, nk, 3, 4), 7.0, dtype=torch.float64, device=dev())
    status = torch.full((b, nk), -7, dtype=torch.int32, device=dev())
    Xd, Kd = up(X), up(K)
    with torch.cuda.device(dev()):
        rc = _abi.load_poses_library().pvnet_pose_solve_classes(
            C.c_void_p(pts.data_ptr()), int(pts.dtype == torch.float64), (C.c_int64 * 4)(*pts.stride()), C.c_void_p(Xd.data_ptr()), None,
            _abi.POSES_W_NONE, C.c_void_p(Kd.data_ptr()), 0, C.c_void_p(vote_status.data_ptr()) if vote_status is not None else None,
            b, nk, pn, pose_cases.LIMIT, C.c_void_p(rt.data_ptr()) if want_rt else None,
            C.c_void_p(poses.data_ptr()) if want_poses else None, C.c_void_p(status.data_ptr()),
            C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream))
        torch.cuda.synchronize()
    assert rc == 0
    return rt, poses, status


@layouts
def test_rt_output_is_the_pose(layout):
    b, nk, pn = layout
    X, x2, _ = noisy(layout)
    pts = up(x2)
    rt, poses, status = raw(X, pts, P.LINEMOD_K)
    only_rt, untouched, s1 = raw(X, pts, P.LINEMOD_K, want_poses=False)
    assert (untouched == 7.0).all() and torch.equal(only_rt, rt) and torch.equal(s1, status)
    untouched, only_poses, s2 = raw(X, pts, P.LINEMOD_K, want_rt=False)
    assert (untouched == 7.0).all() and torch.equal(only_poses, poses) and torch.equal(s2, status)
    same((poses, status), P.pnp_classes_device(up(X), pts, P.LINEMOD_K))
    want = pose_cases.poses_to_rt(poses.cpu().numpy().reshape(b * nk, 3, 4)).reshape(b, nk, 6)
    d = float(np.abs(rt.cpu().numpy() - want).max())
    print(f"rt against poses_to_rt of the poses {layout}: {d:.2e}")
    assert d <= RT_ATOL


# ---- 2. the independent oracle ------------------------------------------------------------------------------------------------------------
@layouts
def test_matches_the_host_library_class_by_class(layout):
    b, nk, pn = layout
    X, x2, _ = noisy(layout)
    Ks = CC.cameras(b)
    W = CC.weights(b, nk, pn)
    for K, Wk in ((P.LINEMOD_K, None), (Ks, None), (P.LINEMOD_K, W)):
        want, hs = CC.host_loop(X, x2, K, Wk)
        got, status = P.pnp_classes_device(up(X), up(x2), up(K), weights_2d=None if Wk is None else up(Wk))
        torch.cuda.synchronize()
        d = float(np.abs(got.cpu().numpy() - want).max())
        print(f"device against host {layout} {'per-image K' if K is Ks else 'shared K'}{' weighted' if Wk is not None else ''}: {d:.2e}")
        assert (hs >= 0).all() and (status.cpu().numpy() >= 0).all()
        assert d <= ATOL
    # float32 key-points, as the vote returns them: the host on the widened values
    x32 = x2.astype(np.float32)
    want, _ = CC.host_loop(X, x32.astype(np.float64), P.LINEMOD_K)
    got, _ = P.pnp_classes_device(up(X), up(x32), P.LINEMOD_K)
    assert float(np.abs(got.cpu().numpy() - want).max()) <= ATOL


@layouts
def test_noise_free_cases_reach_the_ground_truth(layout):
    X, x2, gt = CC.case(*layout)
    got, status = P.pnp_classes_device(up(X), up(x2), P.LINEMOD_K)
    torch.cuda.synchronize()
    d = float(np.abs(got.cpu().numpy() - gt).max())
    print(f"noise-free {layout}: pose error {d:.2e}")
    assert (status.cpu().numpy() >= 0).all() and d <= pose_cases.BAR_POSE
    Ks = CC.cameras(layout[0])
    X, x2, gt = CC.case(*layout, K=Ks)
    got, _ = P.pnp_classes_device(up(X), up(x2), up(Ks))
    assert float(np.abs(got.cpu().numpy() - gt).max()) <= pose_cases.BAR_POSE


# ---- 3. the gate ------------------------------------------------------------------------------------------------------------------------------
@layouts
def test_gate_decides_and_not_the_data(layout):
    b, nk, pn = layout
    X, x2, _ = noisy(layout)
    Xd, pts = up(X), up(x2.astype(np.float32))
    ungated = P.pnp_classes_device(Xd, pts, P.LINEMOD_K)
    rng = np.random.default_rng(9)
    absent = rng.random((b, nk)) < 0.4
    absent[0, 0], absent[-1, -1] = True, False        # both kinds in every layout
    vs = np.zeros((b, nk, pn), np.int32)
    vs[absent] = _abi.S_SKIPPED                        # as the vote marks a class with too few pixels: every word
    i, k = np.argwhere(absent)[-1]
    vs[i, k] = 0
    vs[i, k, pn - 1] = _abi.S_SKIPPED | _abi.S_NO_INLIER   # a single word is enough, the last lane's, beside another bit
    vs[~absent] = rng.choice([0, _abi.S_SINGULAR, _abi.S_NO_INLIER, _abi.S_OVERFLOW, _abi.S_SINGULAR | _abi.S_OVERFLOW], size=(int((~absent).sum()), pn))
    assert not (vs[~absent] & _abi.S_SKIPPED).any() and vs[~absent].any()
    # the key-points of the absent items are valid numbers: the same call without the status solves them
    assert (ungated[1].cpu().numpy()[absent] >= 0).all() and torch.isfinite(pts).all()
    poses = torch.full((b, nk, 3, 4), float("nan"), dtype=torch.float64, device=dev())
    status = torch.full((b, nk), -9, dtype=torch.int32, device=dev())
    got = P.pnp_classes_device(Xd, pts, P.LINEMOD_K, vote_status=up(vs), out=(poses, status))
    torch.cuda.synchronize()
    assert got[0] is poses and got[1] is status
    m = up(absent)
    assert (status[m] == P.POSE_ABSENT).all() and P.POSE_ABSENT == -3
    assert torch.equal(poses[m], torch.zeros_like(poses[m])) and not torch.signbit(poses[m]).any()
    assert torch.equal(poses[~m], ungated[0][~m]) and torch.equal(status[~m], ungated[1][~m])
    # the rt output of an absent item is zeros too, and a status without SKIPPED anywhere gates nothing
    rt, rposes, rstatus = raw(X, pts, P.LINEMOD_K, vote_status=up(vs))
    assert torch.equal(rt[m], torch.zeros_like(rt[m])) and torch.equal(rposes, poses) and torch.equal(rstatus, status)
    others = np.full((b, nk, pn), _abi.S_SINGULAR | _abi.S_NO_INLIER | _abi.S_OVERFLOW, np.int32)
    same(P.pnp_classes_device(Xd, pts, P.LINEMOD_K, vote_status=up(others)), ungated)
    # an absent item reads none of its key-points: NaN in their place changes nothing
    poisoned = pts.clone()
    poisoned[m] = float("nan")
    same(P.pnp_classes_device(Xd, poisoned, P.LINEMOD_K, vote_status=up(vs)), (poses, status))


# ---- 4. isolation -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["collinear", "nan", "inf"])
def test_a_degenerate_item_between_good_ones_leaves_them_alone(fault):
    """A NaN or an infinite key-point fails the linear start: status -2 and zeros, as the host gives them.  Collinear key-points do NOT
    fail it in this solver: the host library's linear start returns a (meaningless) pose for them and its refinement runs (host status
    24 for this item), so pvnet_pose_solve's item -- which a solved item is by definition -- has a status >= 0 there as well.  That item
    is held to the definition (the per-class loop, bit for bit) and to the host's verdict on the linear start; in all three cases the
    items around it equal the same call without the fault."""
    b, nk, pn = 2, 3, 9
    X, x2, _ = noisy((b, nk, pn))
    bad = x2.copy()
    if fault == "collinear":   # all key-points of the item on one image line
        bad[0, 1] = np.stack([np.linspace(100.0, 400.0, pn), np.linspace(50.0, 350.0, pn)], 1)
    else:
        bad[0, 1, 4, 0] = np.nan if fault == "nan" else np.inf
    hp, hs, _ = pose_cases.host_solve(X[1], bad[0:1, 1], P.LINEMOD_K)
    Xd = up(X)
    got = P.pnp_classes_device(Xd, up(bad), P.LINEMOD_K)
    clean = P.pnp_classes_device(Xd, up(x2), P.LINEMOD_K)
    torch.cuda.synchronize()
    print(f"{fault}: device status {got[1].tolist()}, host status of the item {hs.tolist()}")
    assert (hs[0] == -2) == (fault != "collinear") and (hs[0] >= 0 or not hp.any())    # the case is what the docstring claims
    assert (int(got[1][0, 1]) == P.POSE_FAILED) == (hs[0] == -2)
    if hs[0] == -2:
        assert not got[0][0, 1].any()
    keep = torch.ones((b, nk), dtype=torch.bool, device=dev())
    keep[0, 1] = False
    assert torch.equal(got[0][keep], clean[0][keep]) and torch.equal(got[1][keep], clean[1][keep])
    assert (clean[1] >= 0).all() and torch.isfinite(got[0]).all()
    same(got, loop(Xd, up(bad), P.LINEMOD_K))


# ---- 5. - 7. the route end to end ---------------------------------------------------------------------------------------------------------------
H, W_ = 120, 160
HN = 128
SEED = 3
KP_BAR = 1e-3              # px: the voted key-points against the projected ones (tests/test_raster_device.py's closed chain, smoke())
HAND_OVER_BAR = 2 * 0.0    # share of differing pixels, solved poses against input poses (tests/test_raster_device.py's, unchanged)


def bbox_keypoints(v):
    lo, hi = v.min(0), v.max(0)
    return np.array([(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])] + [tuple((lo + hi) / 2)])


@functools.lru_cache(maxsize=None)
def scene():
    """three small meshes at known poses in two images; in the second the third is outside the frame.  Labels by render_visible_labels,
    the exact field composed class by class with vertex_targets_device.  Built once, never written to."""
    from pvnet_amd import depth, render, synth, validation
    from tests import raster_restatement as RS
    from tests.render_cases import camera, pose
    K = camera(H, W_)
    meshes = [render.icosphere(2, 0.07), render.box_mesh(0.12, 0.09, 0.1), render.l_prism_mesh(0.16, 0.07)]
    table = render.DeviceMeshes(meshes)
    kp3 = np.stack([bbox_keypoints(v) for v, _ in meshes])                        # [3,9,3]
    poses = np.stack([
        np.stack([pose((1, 2, 3), 0.8, (-0.10, -0.04, 0.6)), pose((2, -1, 1), 2.0, (0.05, -0.03, 0.55)), pose((0, 1, 1), 0.6, (0.0, 0.06, 0.5))]),   # each hides a part of another
        np.stack([pose((1, 2, 3), 0.8, (-0.12, -0.05, 0.6)), pose((2, -1, 1), 2.0, (0.10, -0.04, 0.55)), pose((0, 1, 0), 0.3, (1.5, 0.0, 0.5))])])   # the third: outside
    labels = depth.render_visible_labels(table, [0, 1, 2], [1, 2, 3], up(poses), K, H, W_)
    present = np.array([[True, True, True], [True, True, False]])
    proj = np.stack([np.stack([np.stack(RS.project_points(kp3[k], poses[i, k], K)[:2], -1).astype(np.float64) for k in range(3)]) for i in range(2)])
    field = torch.zeros((2, 18, H, W_), dtype=torch.float32, device=dev())
    for k in range(3):
        mk = (labels == k + 1).to(torch.uint8)
        vert, _ = validation.vertex_targets_device(mk, up(np.concatenate([proj[:, k], np.ones((2, 9, 1))], -1)))
        field += vert
    torch.cuda.synchronize()
    counts = [[int((labels[i] == k + 1).sum()) for k in range(3)] for i in range(2)]
    assert all((c > 300) == bool(p) and (p or c == 0) for cs, ps in zip(counts, present) for c, p in zip(cs, ps)), counts
    return dict(K=K, meshes=meshes, table=table, kp3=kp3, poses=poses, labels=labels, field=field, present=present, proj=proj)


def wrapper():
    from pvnet_amd import voting
    s = scene()
    return voting.MultiPoseEvalWrapper([s["kp3"][k] for k in range(3)], s["K"], round_hyp_num=HN, inlier_thresh=0.99)


@functools.lru_cache(maxsize=None)
def route_from_labels():
    s = scene()
    out = wrapper()(s["labels"], s["field"], use_argmax=False, return_all=True, seed=SEED)
    torch.cuda.synchronize()
    return out


def test_route_from_rendered_labels_to_poses_and_back():
    from pvnet_amd import depth, evaluation, voting
    s = scene()
    poses, status, kpts, vote_status = route_from_labels()
    present = up(s["present"])
    assert tuple(poses.shape) == (2, 3, 3, 4) and tuple(status.shape) == (2, 3) and tuple(kpts.shape) == (2, 3, 9, 2)
    # the vote: exact key-points for the present classes, SKIPPED for the hidden one
    err = float((kpts.double() - up(s["proj"]))[present].abs().max())
    print(f"route: voted key-points within {err:.3e} px of the projected ones")
    assert err < KP_BAR
    assert (vote_status[~present] & _abi.S_SKIPPED).all() and not (vote_status[present] & _abi.S_SKIPPED).any()
    # the solve: the hidden class is absent with a zero pose, the others are solved and equal the ungated per-class loop
    assert (status[~present] == P.POSE_ABSENT).all() and not poses[~present].any() and (status[present] >= 0).all()
    want = loop(up(s["kp3"]), kpts, s["K"])
    assert torch.equal(poses[present], want[0][present]) and torch.equal(status[present], want[1][present])
    assert torch.equal(poses, P.pnp_classes_device(up(s["kp3"]), kpts, s["K"], vote_status=vote_status)[0])
    # labels re-rendered from the solved poses (the hidden one stays where it was put: outside the frame)
    solved = torch.where(present[:, :, None, None], poses, up(s["poses"]))
    again = depth.render_visible_labels(s["table"], [0, 1, 2], [1, 2, 3], solved, s["K"], H, W_)
    differing = int((again != s["labels"]).sum())
    share = differing / float(s["labels"].numel())
    print(f"route: labels of the solved poses differ from the input poses' in {share:.6e} of the pixels ({differing} of {s['labels'].numel()})")
    assert share <= HAND_OVER_BAR, (share, HAND_OVER_BAR)
    # plug-compatibility: the flattened poses with class ids go into pose_metrics_device as they are
    names = ["sphere", "box", "prism"]
    models = evaluation.DeviceModels({n: v for n, (v, _) in zip(names, s["meshes"])},
                                     {n: float(np.linalg.norm(v.max(0) - v.min(0))) for n, (v, _) in zip(names, s["meshes"])}, dev(), symmetric=())
    flat = poses.view(6, 3, 4)
    assert flat.data_ptr() == poses.data_ptr()
    class_ids = torch.arange(3, device=dev()).repeat(2)
    errors, passed, mstatus = evaluation.pose_metrics_device(flat, s["poses"].reshape(6, 3, 4), s["K"], models, class_ids=class_ids)
    torch.cuda.synchronize()
    p = present.view(6)
    print(f"route: ADD of the present items {errors[p, 1].tolist()}")
    assert (mstatus == 0).all() and passed[p, 1].all() and passed[p].all() and not passed[~p, 1].any()
    assert isinstance(wrapper()(s["labels"], s["field"], use_argmax=False, seed=SEED), torch.Tensor)
    assert voting.MultiPoseEvalWrapper is type(wrapper())


def test_route_from_one_hot_logits_gives_the_same_bits():
    s = scene()
    poses, status, kpts, vote_status = route_from_labels()
    logits = torch.nn.functional.one_hot(s["labels"].long(), 4).permute(0, 3, 1, 2).float().contiguous()
    got = wrapper()(logits, s["field"], return_all=True, seed=SEED)
    torch.cuda.synchronize()
    assert torch.equal(got[2], kpts) and torch.equal(got[3], vote_status)
    assert torch.equal(got[0], poses) and torch.equal(got[1], status)
    # per-image cameras through forward: the same cameras, the same bits
    Ks = up(np.repeat(s["K"][None], 2, 0))
    assert torch.equal(wrapper()(logits, s["field"], K=Ks, seed=SEED), poses)


def test_vote_and_solve_captured_in_one_graph():
    from pvnet_amd import voting
    s = scene()
    wrap = wrapper()
    labels, field = s["labels"].clone(), s["field"].clone()
    L = voting.vote_layout(6, H, W_, 9, HN, 30000)
    ws = torch.zeros(L.total_bytes, dtype=torch.uint8, device=dev())
    kp = torch.zeros((2, 3, 9, 2), dtype=torch.float32, device=dev())
    poses = torch.zeros((2, 3, 3, 4), dtype=torch.float64, device=dev())
    status = torch.zeros((2, 3), dtype=torch.int32, device=dev())

    def enqueue():
        return wrap(labels, field, use_argmax=False, return_all=True, seed=SEED, workspace=ws, kpts_out=kp, out=(poses, status))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()   # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = enqueue()
    assert captured[0] is poses and captured[1] is status and captured[2] is kp
    first = route_from_labels()
    # another label batch: the two images change places (the hidden class moves to the first image)
    other = wrap(s["labels"].flip(0).contiguous(), s["field"].flip(0).contiguous(), use_argmax=False, return_all=True, seed=SEED)
    torch.cuda.synchronize()
    assert not torch.equal(other[1], first[1])
    for replay, want in enumerate((first, first, other)):
        if replay == 2:
            labels.copy_(s["labels"].flip(0))
            field.copy_(s["field"].flip(0))
        poses.fill_(float("nan"))
        status.fill_(-9)
        kp.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(kp, want[2]) and torch.equal(captured[3], want[3]), replay
        assert torch.equal(poses, want[0]) and torch.equal(status, want[1]), replay
