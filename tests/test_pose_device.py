"""The device pose solve (pnp.pnp_batch_device -> pvnet_pose_solve, pvnet_amd/csrc/pose_solve.hip) against its oracle, the host
library (pnp_batch / pvnet_pnp_solve) on the same float64 inputs, and against Evaluator.evaluate_uncertainty for covariances.

Bar: every [R|t] entry within ATOL of the host.  Both sides run the same algorithm with the same operation order; only the device
math library's sin / cos / atan2 may differ from the host's in the last place, which the LM absorbs far below this bar."""
import numpy as np
import pytest
import torch

from pvnet_amd import evaluation as E
from pvnet_amd import pnp as P
from pvnet_amd import synth, voting
from tests import pose_cases
from tests.pose_cases import problems

pytestmark = pytest.mark.gpu

ATOL = 1e-8
# LM iterations, device against host, of every well-posed image.  The poses agree to ATOL; once converged, the stopping rules
# (relative decrease < 1e-16, a step below 1e-15 |x|) are decided by last-place rounding, where the device's sin / cos may differ
# from the host's: measured up to 4 apart on the weighted problems of test_explicit_weights_match_the_host (unweighted: <= 2)
ITER_SLACK = 4


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def host_solve(X, x2, K, W=None):
    """pvnet_pnp_solve image by image: (poses [n,3,4] as pnp_batch gives them, status [n] = its return values)"""
    return pose_cases.host_solve(X, x2, K, W)[:2]


def device(X, x2, K, **kw):
    poses, status = P.pnp_batch_device(X, x2, K, **kw)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), status.cpu().numpy()


def test_unweighted_matches_the_host_for_f32_f64_and_strided_keypoints():
    X, x2, _ = problems(64)
    x2_32 = x2.astype(np.float32)
    for pts, host_in in ((torch.from_numpy(x2).to(dev()), x2),
                         (torch.from_numpy(x2_32).to(dev()), x2_32.astype(np.float64))):
        want = P.pnp_batch(X, host_in, P.LINEMOD_K)
        got, status = device(X, pts, P.LINEMOD_K)
        np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
        assert (status >= 0).all() and (status <= 200).all()
    # a strided view: [n,pn,2] taken out of a wider [n,pn,4] float32 buffer, read in place
    wide = torch.zeros((64, 9, 4), dtype=torch.float32, device=dev())
    wide[:, :, 1::2] = torch.from_numpy(x2_32).to(dev())
    view = wide[:, :, 1::2]
    assert not view.is_contiguous()
    got, _ = device(X, view, P.LINEMOD_K)
    np.testing.assert_allclose(got, P.pnp_batch(X, x2_32.astype(np.float64), P.LINEMOD_K), rtol=0, atol=ATOL)
    # independent cross-check: scipy's MINPACK LM on the same problem (the native-vs-scipy bar of tests/test_pnp.py)
    for i in range(0, 64, 8):
        np.testing.assert_allclose(got[i], P.pnp(X, x2_32[i].astype(np.float64), P.LINEMOD_K, backend="scipy"), atol=2e-7)


def test_explicit_weights_match_the_host():
    X, x2, _ = problems(48, seed=3)
    rng = np.random.default_rng(4)
    W = np.abs(rng.normal(1.0, 0.3, size=(48, 9, 3)))
    W[:, :, 1] *= 0.1
    W[:, 8] = [0.01, 0.0, 0.01]   # one key-point trusted 100x less
    want = P.pnp_batch(X, x2, P.LINEMOD_K, weights_2d=W)
    got, status = device(X, torch.from_numpy(x2).to(dev()), P.LINEMOD_K, weights_2d=W)
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    _, hs = host_solve(X, x2, P.LINEMOD_K, W)
    assert np.abs(status - hs).max() <= ITER_SLACK


def _evaluator_pose(ev, kpts, cov, K):
    return ev.evaluate_uncertainty(kpts, cov, np.eye(4)[:3], "cat", intri_type="use_intrinsic", intri_matrix=K)


def test_covariance_weights_match_evaluate_uncertainty(demo_fixture):
    f = demo_fixture
    X, K = f["points_3d"].astype(np.float64), f["K"].astype(np.float64)
    n = 8
    rng = np.random.default_rng(7)
    planar = synth.field_from_keypoints(f["mask"].astype(bool), f["points_2d"])
    planars = np.stack([synth.add_noise(planar.copy(), f["mask"].astype(bool), rng, sigma_rad=0.08, outlier_frac=0.2)
                        for _ in range(n)])
    m = torch.from_numpy(np.repeat(f["mask"][None].astype(np.int64), n, 0)).to(dev())
    v = synth.planar_to_vertex_view(torch.from_numpy(planars).to(dev()))
    kpts = voting.ransac_voting_layer_v3(m, v, 512, inlier_thresh=0.99, seed=5)
    kpts, cov = voting.estimate_voting_distribution_with_mean(m, v, kpts, seed=6)
    cov_np = cov.cpu().numpy().copy()
    # hand-made cases: a tiny cov[0,0] (zero weight), a NaN entry (zero weight), an axis-aligned rank-1 covariance (the clamped
    # eigenvalue gives a weight of 1e15 along y -- axis-aligned, so that the eigen-solver's zero eigenvalue is exact on both sides)
    cov_np[1, 0] = [[1e-7, 0.0], [0.0, 3.0]]
    cov_np[2, 3] = [[2.0, np.nan], [np.nan, 1.0]]
    cov_np[3, 5] = [[0.04, 0.0], [0.0, 0.0]]
    kp_np = kpts.cpu().numpy().astype(np.float64)
    got, status = device(X, kpts, K, covariance=torch.from_numpy(cov_np).to(dev()))
    assert (status >= 0).all()
    ev = E.Evaluator(models={"cat": X}, diameters={"cat": 0.1}, points_3d={"cat": X})
    for i in range(n):
        want = _evaluator_pose(ev, kp_np[i], cov_np[i], K)
        np.testing.assert_allclose(got[i], want, rtol=0, atol=ATOL, err_msg=f"image {i}")
    assert np.isfinite(got).all()


def test_per_image_intrinsics():
    X, x2, _ = problems(16, seed=21)
    rng = np.random.default_rng(2)
    Ks = np.repeat(P.LINEMOD_K[None], 16, 0)
    Ks[:, 0, 0] *= rng.uniform(0.9, 1.1, 16)
    Ks[:, 1, 1] *= rng.uniform(0.9, 1.1, 16)
    Ks[:, :2, 2] += rng.uniform(-5, 5, (16, 2))
    want, hs = host_solve(X, x2, Ks)
    got, status = device(X, torch.from_numpy(x2).to(dev()), torch.from_numpy(Ks).to(dev()))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    assert np.abs(status - hs).max() <= ITER_SLACK


def test_rare_branches_match_the_host_image_by_image():
    """degenerate images (all-zero key-points as v3 returns them below min_num, a NaN key-point, coincident key-points, a start
    with a point on the camera plane) get the host's status and (zero) pose; the images beside them are unaffected"""
    X, x2, _ = problems(12, seed=31)
    x2 = x2.copy()
    x2[2] = 0.0                    # all-zero image: the host's LM runs to its iteration limit on it
    x2[5, 4, 0] = np.nan           # a NaN key-point: failed linear start
    x2[7] = x2[7, 0]               # coincident key-points: iteration limit as well
    want, hs = host_solve(X, x2, P.LINEMOD_K)
    got, status = device(X, torch.from_numpy(x2).to(dev()), P.LINEMOD_K)
    print("status device", status.tolist(), "host", hs.tolist())
    assert ((status == P.POSE_FAILED) == (hs == -2)).all(), (status, hs)
    assert status[5] == P.POSE_FAILED and not got[5].any()
    assert np.isfinite(got).all()
    # the degenerate images 2 and 7 have no optimum to agree on (the LM wanders for its 200 iterations); every other image must
    # equal the host and be untouched by its neighbours
    good = np.array([i not in (2, 5, 7) for i in range(12)])
    assert (status[[2, 7]] >= 0).all()
    np.testing.assert_allclose(got[good], want[good], rtol=0, atol=ATOL)
    assert np.abs(status[good] - hs[good]).max() <= ITER_SLACK
    alone, _ = device(X, torch.from_numpy(x2[good]).to(dev()), P.LINEMOD_K)
    assert alone.tobytes() == got[good].tobytes()
    # camera plane: the object's first point sits at the camera centre under the true pose of a noiseless image; the host
    # returns its linear start unrefined (status 0) when the first evaluation fails, and so must the device
    r = np.array([0.3, -0.2, 0.1])
    pose = np.concatenate([P.rodrigues(r), np.array([[0.0], [0.0], [0.8]])], 1)
    Xc = X.copy()
    Xc[0] = -P.rodrigues(r).T @ pose[:, 3]          # R X0 + t = 0
    img = P.project(Xc[1:], pose, P.LINEMOD_K)
    img = np.concatenate([P.LINEMOD_K[None, :2, 2], img], 0)[None]   # (its image: the principal point)
    want, hs = host_solve(Xc, img, P.LINEMOD_K)
    got, status = device(Xc, torch.from_numpy(img).to(dev()), P.LINEMOD_K)
    assert hs[0] == 0 and status[0] == 0
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)


def _pipeline_case(demo_fixture, n, seed):
    f = demo_fixture
    rng = np.random.default_rng(seed)
    fg = f["mask"].astype(bool)
    planar = synth.field_from_keypoints(fg, f["points_2d"])
    planars = np.stack([synth.add_noise(planar.copy(), fg, rng, sigma_rad=0.05, outlier_frac=0.1) for _ in range(n)])
    seg = torch.zeros((n, 2) + fg.shape, dtype=torch.float32)
    seg[:, 1] = torch.from_numpy(np.where(fg, 1.0, -1.0).astype(np.float32))
    vertex = torch.from_numpy(planars).to(dev())   # [n, vn*2, h, w]: the backbone's layout
    return seg.to(dev()), vertex


@pytest.mark.parametrize("use_uncertainty", [False, True])
def test_pose_eval_wrapper_pipeline(demo_fixture, use_uncertainty):
    f = demo_fixture
    X, K, gt = f["points_3d"].astype(np.float64), f["K"].astype(np.float64), f["pose"].astype(np.float64)
    seg, vertex = _pipeline_case(demo_fixture, 32, 3)
    torch.manual_seed(0)
    wrap = voting.PoseEvalWrapper(X, K, round_hyp_num=512, inlier_thresh=0.99, use_uncertainty=use_uncertainty)
    poses, status, kpts, cov = wrap(seg, vertex, return_all=True)
    torch.cuda.synchronize()
    poses, status, kp = poses.cpu().numpy(), status.cpu().numpy(), kpts.cpu().numpy().astype(np.float64)
    assert (status >= 0).all()
    if use_uncertainty:
        ev = E.Evaluator(models={"cat": X}, diameters={"cat": 0.1}, points_3d={"cat": X})
        cv = cov.cpu().numpy()
        host = np.stack([_evaluator_pose(ev, kp[i], cv[i], K) for i in range(32)])
    else:
        host = P.pnp_batch(X, kp, K)
    np.testing.assert_allclose(poses, host, rtol=0, atol=ATOL)
    for i in range(32):
        d_cm, d_deg = P.cm_degree_error(poses[i], gt)
        h_cm, h_deg = P.cm_degree_error(host[i], gt)
        assert abs(d_cm - h_cm) < 1e-5 and abs(d_deg - h_deg) < 1e-4
        assert abs(P.projection_2d_error(poses[i], gt, f["bb8_3d"], K) - P.projection_2d_error(host[i], gt, f["bb8_3d"], K)) < 1e-5


def test_graph_capture_of_voting_and_pose_is_bitwise_eager():
    mask, planar, _ = synth.make_batch(4, first_index=700, h=96, w=128, radius=14, noise=True)
    m = torch.from_numpy(np.ascontiguousarray(mask)).to(dev())
    v = synth.planar_to_vertex_view(torch.from_numpy(planar).to(dev()))
    vn = v.shape[3]
    rng = np.random.default_rng(1)
    X = rng.uniform(-0.08, 0.08, size=(vn, 3))
    Xd, Kd = torch.from_numpy(X).to(dev()), torch.from_numpy(P.LINEMOD_K.copy()).to(dev())
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
