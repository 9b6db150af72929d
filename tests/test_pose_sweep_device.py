"""The device pose solve (pvnet_pose_solve, pvnet_amd/csrc/pose_solve.hip) over its documented range of key-point counts,
pn = 6 .. PVNET_POSE_MAX_PN = 64, against the host library on the same float64 inputs (tests/pose_cases.py).

Lane i of one wavefront owns key-point i and every sum runs serially over pn, so the sweep covers both ends of the range, the
counts around the 27 lanes that sum the normal equations, around 32 lanes and around the full wave: the ``lane < pn`` guards,
the lanes from 32 up, and the smallest null space of the 12x12 DLT matrix (pn = 6).

Bars: BAR_POSE on every [R|t] entry, and the device pose's cost on the host at most (1 + BAR_COST) times the host's final cost.
tests/test_pose_sweep_cpu.py derives them from the oracle's own spread and shows that they tell a dropped or misread key-point.
Iteration counts are not compared: the host differs from itself by up to 6 on inputs one unit in the last place apart.
The maxima of a run are recorded in profiles/pose_sweep_device.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pvnet_amd import _abi
from pvnet_amd import pnp as P
from pvnet_amd import synth, voting
from tests import pose_cases as PC

pytestmark = pytest.mark.gpu

K = P.LINEMOD_K
FORMS = ("unweighted", "weighted", "covariance")


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def device(X, x2, K, **kw):
    poses, status = P.pnp_batch_device(X, x2, K, **kw)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), status.cpu().numpy()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def form_kw(form, W, cov):
    """pnp_batch_device's keyword of one form (the weights are uploaded from numpy by the entry itself)"""
    return {"unweighted": {}, "weighted": {"weights_2d": W}, "covariance": {"covariance": up(cov)}}[form]


@functools.lru_cache(maxsize=None)
def oracle(pn, form):
    """the host's answer, once per case: (poses, status, its final cost, the weights that cost is taken with)"""
    X, x2, W, cov = PC.sweep_case(pn)
    if form == "covariance":   # Evaluator.evaluate_uncertainty image by image; status from the host solve with its weights
        Wc = PC.covariance_weights(cov)
        poses = PC.evaluator_solve(X, x2, cov, K)
        status, rt = PC.host_solve(X, x2, K, Wc)[1], PC.poses_to_rt(poses)
    else:
        Wc = W if form == "weighted" else None
        poses, status, rt = PC.host_solve(X, x2, K, Wc)
    return poses, status, PC.host_cost(X, x2, Wc, K, rt), Wc


def against_the_host(what, got, status, X, x2, Wc, want, hs, cost, stages):
    """the three assertions of the sweep; prints the figures first"""
    d_pose = float(np.abs(got - want).max())
    excess = PC.host_cost(X, x2, Wc, K, PC.poses_to_rt(got)) / cost - 1.0
    print(f"pose_sweep {what}: pose {d_pose:.2e} cost excess {float(excess.max()):.2e} iterations {int(np.abs(status - hs).max())} "
          f"apart (device most {int(status.max())}, host most {int(hs.max())})")
    assert (hs >= 0).all() and (hs < stages * PC.LIMIT).all()        # (the oracle: tests/test_pose_sweep_cpu.py)
    assert (status >= 0).all() and (status < stages * PC.LIMIT).all(), status
    assert d_pose <= PC.BAR_POSE
    assert (excess <= PC.BAR_COST).all(), float(excess.max())


@pytest.mark.parametrize("pn", PC.SWEEP_PN)
def test_sweep_matches_the_host(pn):
    X, x2, W, cov = PC.sweep_case(pn)
    pts = up(x2)
    for form in FORMS:
        want, hs, cost, Wc = oracle(pn, form)
        got, status = device(X, pts, K, **form_kw(form, W, cov))
        against_the_host(f"pn {pn:2d} {form:10s}", got, status, X, x2, Wc, want, hs, cost, 1 if form == "unweighted" else 2)
    # float32 key-points, as voting returns them: the host on the widened values
    x32 = x2.astype(np.float32)
    wide = x32.astype(np.float64)
    want, hs, rt = PC.host_solve(X, wide, K)
    got, status = device(X, up(x32), K)
    against_the_host(f"pn {pn:2d} float32   ", got, status, X, wide, None, want, hs, PC.host_cost(X, wide, None, K, rt), 1)


def raw_solve(X, pts, n, pn, want_rt, want_poses):
    """pvnet_pose_solve through ctypes on the loaded library (pnp_batch_device always passes rt = NULL): outputs start as
    sentinels, so that what comes back was written"""
    rt = torch.full((n, 6), 7.0, dtype=torch.float64, device=dev())
    poses = torch.full((n, 3, 4), 7.0, dtype=torch.float64, device=dev())
    status = torch.full((n,), -7, dtype=torch.int32, device=dev())
    Xd, Kd = up(X), up(K)
    with torch.cuda.device(dev()):
        rc = _abi.load_library().pvnet_pose_solve(
            C.c_void_p(pts.data_ptr()), int(pts.dtype == torch.float64), (C.c_int64 * 3)(*pts.stride()), C.c_void_p(Xd.data_ptr()),
            None, _abi.POSE_W_NONE, C.c_void_p(Kd.data_ptr()), 0, n, pn, PC.LIMIT, C.c_void_p(rt.data_ptr()) if want_rt else None,
            C.c_void_p(poses.data_ptr()) if want_poses else None, C.c_void_p(status.data_ptr()),
            C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream))
        torch.cuda.synchronize()
    assert rc == 0
    return rt.cpu().numpy(), poses.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("pn", [6, 64])
def test_rt_and_poses_outputs(pn):
    X, x2, _, _ = PC.sweep_case(pn)
    x2 = x2.copy()
    x2[3, pn - 1, 1] = np.nan   # the last lane's point: a failed linear start
    n = x2.shape[0]
    pts = up(x2)
    rt_a, untouched, st_a = raw_solve(X, pts, n, pn, True, False)
    assert (untouched == 7.0).all()
    untouched, poses_b, st_b = raw_solve(X, pts, n, pn, False, True)
    assert (untouched == 7.0).all()
    rt_c, poses_c, st_c = raw_solve(X, pts, n, pn, True, True)
    assert rt_a.tobytes() == rt_c.tobytes() and poses_b.tobytes() == poses_c.tobytes()
    assert (st_a == st_c).all() and (st_b == st_c).all()
    # the two outputs are one pose: the host's conversion of rt
    conv = np.empty((n, 3, 4))
    P.load_pnp_library().pvnet_pnp_poses_from_rt(P._dptr(np.ascontiguousarray(rt_c)), P._dptr(conv), n)
    np.testing.assert_allclose(poses_c, conv, rtol=0, atol=1e-15)
    assert st_c[3] == P.POSE_FAILED and not rt_c[3].any() and not poses_c[3].any()
    good = np.arange(n) != 3
    want, hs, _ = PC.host_solve(X, x2, K)
    assert hs[3] == -2 and (st_c[good] >= 0).all() and (st_c[good] < PC.LIMIT).all()
    assert np.abs(poses_c - want).max() <= PC.BAR_POSE


def test_strided_keypoints_with_poisoned_gaps():
    pn, rows = 33, 40
    X, x2, _, _ = PC.sweep_case(pn)
    n = x2.shape[0]
    x32 = x2.astype(np.float32)
    wide = torch.full((n, rows, 4), float("nan"), dtype=torch.float32, device=dev())
    wide[:, :pn, 1::2] = up(x32)
    view = wide[:, :pn, 1::2]
    assert not view.is_contiguous() and torch.isnan(wide[:, pn:]).all() and torch.isnan(wide[:, :, 0::2]).all()
    flat, flat_status = device(X, up(x32), K)
    got, status = device(X, view, K)
    assert np.isfinite(got).all() and got.tobytes() == flat.tobytes() and (status == flat_status).all()
    # the same view with intrinsics per image, against the host
    rng = np.random.default_rng(2)
    Ks = np.repeat(K[None], n, 0)
    Ks[:, 0, 0] *= rng.uniform(0.9, 1.1, n)
    Ks[:, 1, 1] *= rng.uniform(0.9, 1.1, n)
    Ks[:, :2, 2] += rng.uniform(-5, 5, (n, 2))
    x64 = x32.astype(np.float64)
    want, hs, _ = PC.host_solve(X, x64, Ks)
    got, status = device(X, view, up(Ks))
    assert (hs >= 0).all() and (hs < PC.LIMIT).all() and (status >= 0).all() and (status < PC.LIMIT).all()
    assert np.abs(got - want).max() <= PC.BAR_POSE
    assert np.abs(got - flat).max() > 100 * PC.BAR_POSE   # (the intrinsics were read per image)


@pytest.mark.parametrize("pn", [6, 32, 64])
def test_an_image_alone_equals_the_image_in_its_batch(pn):
    X, x2, W, cov = PC.sweep_case(pn)
    for form in FORMS:
        batch, batch_status = device(X, up(x2), K, **form_kw(form, W, cov))
        for i in (0, 17, 31):
            alone, status = device(X, up(x2[i:i + 1]), K, **form_kw(form, W[i:i + 1], cov[i:i + 1]))
            assert alone.tobytes() == batch[i:i + 1].tobytes(), (form, i)
            assert status[0] == batch_status[i]


@pytest.mark.parametrize("pn", PC.ILL_PN)
def test_ill_posed_images_stay_sane(pn):
    """3 px of noise: where the host converges, the device agrees (the host's own spread there is 1.2e-8; measured on the device:
    6.9e-9, 3.0e-9, 6.4e-9); where the host runs to
    its limit there is no optimum to agree on -- the output is a finite rigid pose, and the images beside it are untouched"""
    X, x2 = PC.ill_posed_case(pn)
    want, hs, _ = PC.host_solve(X, x2, K)
    ill = hs >= PC.LIMIT
    assert (hs >= 0).all() and ill.sum() <= len(x2) // 4
    got, status = device(X, up(x2), K)
    print(f"pose_sweep 3 px pn {pn:2d}: {int(ill.sum())} ill-posed; well-posed pose {float(np.abs(got - want)[~ill].max()):.2e} "
          f"iterations {int(np.abs(status - hs)[~ill].max())} apart; ill-posed status {status[ill].tolist()}")
    assert np.isfinite(got).all()
    assert (status >= 0).all() and (status <= 2 * PC.LIMIT).all()
    assert np.abs(got - want)[~ill].max() <= 3 * PC.BAR_POSE
    R = got[:, :, :3]
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-12
    without, without_status = device(X, up(x2[~ill]), K)
    assert without.tobytes() == got[~ill].tobytes() and (without_status == status[~ill]).all()


def test_graph_replay_at_33_keypoints():
    vn = 33
    mask, planar, _ = synth.make_batch(4, first_index=700, h=96, w=128, vn=vn, radius=14, noise=True)
    m = up(mask)
    v = synth.planar_to_vertex_view(up(planar))
    assert v.shape[3] == vn
    X = np.random.default_rng(1).uniform(-0.08, 0.08, size=(vn, 3))
    Xd, Kd = up(X), up(K.copy())
    L = voting.vote_layout(4, 96, 128, vn, 64, 30000)
    ws = torch.empty(L.total_bytes, dtype=torch.uint8, device=dev())
    kp = torch.zeros((4, vn, 2), device=dev())
    poses = torch.zeros((4, 3, 4), dtype=torch.float64, device=dev())
    status = torch.zeros((4,), dtype=torch.int32, device=dev())

    def enqueue():
        voting.ransac_voting_layer_v3(m, v, 64, inlier_thresh=0.99, seed=21, out=kp, workspace=ws)
        P.pnp_batch_device(Xd, kp, Kd, out=(poses, status))

    eager = []
    for _ in range(2):
        enqueue()
        torch.cuda.synchronize()
        eager.append((kp.clone(), poses.clone(), status.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*eager))   # two eager calls: bitwise identical
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    kp.zero_()
    poses.zero_()
    status.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(kp, eager[0][0]) and torch.equal(poses, eager[0][1]) and torch.equal(status, eager[0][2])
    assert poses.abs().sum() > 0


@pytest.mark.parametrize("pn", [5, 65])
def test_bounds_through_python(pn):
    rng = np.random.default_rng(pn)
    X, pts = rng.uniform(-0.08, 0.08, size=(pn, 3)), up(rng.uniform(0.0, 400.0, size=(4, pn, 2)))
    with pytest.raises(RuntimeError, match="pvnet_pose_solve"):
        P.pnp_batch_device(X, pts, K)
    poses = torch.full((4, 3, 4), 7.0, dtype=torch.float64, device=dev())
    status = torch.full((4,), -7, dtype=torch.int32, device=dev())
    for kw in ({}, {"weights_2d": np.ones((4, pn, 3))}, {"covariance": up(np.tile(np.eye(2, dtype=np.float32), (4, pn, 1, 1)))}):
        with pytest.raises(RuntimeError, match="pvnet_pose_solve"):
            P.pnp_batch_device(X, pts, K, out=(poses, status), **kw)
    torch.cuda.synchronize()
    assert (poses == 7.0).all() and (status == -7).all()
