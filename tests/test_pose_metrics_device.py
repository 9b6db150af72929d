"""The device pose metrics (evaluation.pose_metrics_device -> pvnet_pose_metrics, pvnet_amd/csrc/pose_metrics.hip) against their
oracle, the host Evaluator of this repository image by image: Evaluator._record's ADD / ADD-S, projection_2d(_sym) and
cm_degree_5 recorders, add_error / projection_2d_error and pnp.cm_degree_error.

Bars: plain metrics within rtol 1e-12 of the host (with absolute floors at the last places of the host's own BLAS products);
nearest-neighbour metrics within rtol 1e-7 of the host, and the search's indices equal to oracle/nn_oracle.py's and to pvnet_nn's
on the same float32 clouds (on lattice models, where most minima are tied, the errors then within rtol 1e-12 of the float64 mean over
those indices); pass flags equal wherever the error is not within 1e-9 (relative) of its threshold."""
import numpy as np
import pytest
import torch

from oracle import nn_oracle
from pvnet_amd import evaluation as E
from pvnet_amd import pnp as P
from pvnet_amd import synth, voting
from tests import nn_cases as NC

pytestmark = pytest.mark.gpu

RTOL = 1e-12
# absolute floors per error column (projection px, ADD, cm, degrees): the host forms its clouds with BLAS products, which may
# round differently from the term-by-term float64 expressions in the last place; arccos magnifies that near 0 and 180 degrees
ATOL = np.array([1e-10, 1e-15, 1e-12, 1e-9])
THRESH = (5.0, 0.1, 5.0, 5.0)
PASCAL_K = E.INTRINSIC_MATRIX["pascal"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def random_pose(rng, max_angle=np.pi):
    r = rng.normal(size=3)
    r *= rng.uniform(0.0, max_angle) / np.linalg.norm(r)
    t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.5)])
    return np.concatenate([P.rodrigues(r), t[:, None]], 1)


def perturbed(rng, pose, scale):
    """a prediction near `pose`: a rotation of up to 10 * scale degrees and up to 8 * scale cm (so that both sides of every
    threshold occur)"""
    r = rng.normal(size=3)
    r *= np.deg2rad(rng.uniform(0.0, 10.0 * scale)) / np.linalg.norm(r)
    out = pose.copy()
    out[:, :3] = P.rodrigues(r) @ pose[:, :3]
    d = rng.normal(size=3)
    out[:, 3] += d / np.linalg.norm(d) * rng.uniform(0.0, 0.08 * scale)
    return out


def model_cloud(rng, npts, dup=0):
    m = rng.uniform(-0.1, 0.1, (npts, 3))
    if dup:   # exact ties: the second half repeats the first `dup` points
        m[npts // 2: npts // 2 + dup] = m[:dup]
    return m


def host_metrics(ev, pred, tgt, cls, K, sym_projection):
    """one image through Evaluator._record: (errors [4], passed [3])"""
    ev._record(pred, np.asarray(tgt, np.float64), cls, K, sym_projection=sym_projection)
    tr, rot = P.cm_degree_error(pred, np.asarray(tgt, np.float64))
    return (np.array([ev.proj_mean_diffs[-1], ev.add_dists[-1], tr, rot]),
            np.array([ev.projection_2d_recorder[-1], ev.add_recorder[-1], ev.cm_degree_5_recorder[-1]]))


def run_device(preds, tgts, Ks, models, ids, sym_projection=False, workspace=None):
    d = dev()
    tg = torch.from_numpy(np.ascontiguousarray(tgts)).to(d)
    K = torch.from_numpy(np.ascontiguousarray(Ks, np.float64)).to(d)
    cid = torch.from_numpy(np.asarray(ids, np.int32)).to(d)
    err, ok, st = E.pose_metrics_device(torch.from_numpy(preds).to(d), tg, K, models, class_ids=cid,
                                        sym_projection=sym_projection, thresholds=THRESH, workspace=workspace)
    torch.cuda.synchronize()
    return err.cpu().numpy(), ok.cpu().numpy(), st.cpu().numpy()


def check_errors(got, want, rtol, msg, equal_nan=False):
    """every error column within rtol of the host, above that column's absolute floor"""
    rtol = np.broadcast_to(np.asarray(rtol, np.float64), (4,))
    for k in range(4):
        np.testing.assert_allclose(got[k], want[k], rtol=rtol[k], atol=ATOL[k], equal_nan=equal_nan,
                                   err_msg=f"{msg} column {k}: got {got.tolist()} want {want.tolist()}")


def check_flags(got_ok, want_ok, want_err, diam):
    th = np.array([THRESH[0], diam * THRESH[1]])
    far = np.abs(want_err[:2] - th) > 1e-9 * th
    assert (got_ok[:2] == want_ok[:2])[far].all(), (got_ok, want_ok, want_err)
    if abs(want_err[2] - 5) > 5e-9 and abs(want_err[3] - 5) > 5e-9:
        assert got_ok[2] == want_ok[2], (got_ok, want_ok, want_err)


SIZES = (1, 7, 255, 256, 257, 5000, 20000)


@pytest.mark.parametrize("target_f64", [True, False])
@pytest.mark.parametrize("k_kind", ["shared", "per_image", "pascal"])
def test_plain_metrics_match_the_host(target_f64, k_kind):
    rng = np.random.default_rng(3 + int(target_f64) + 7 * len(k_kind))
    names = [f"c{s}" for s in SIZES]
    models = {c: model_cloud(rng, s) for c, s in zip(names, SIZES)}
    diam = {c: rng.uniform(0.1, 0.3) for c in names}
    dm = E.DeviceModels(models, diam, dev())
    n = 3 * len(SIZES)
    ids = np.arange(n) % len(SIZES)
    rng.shuffle(ids)
    tgts = np.stack([random_pose(rng) for _ in range(n)])
    preds = np.stack([perturbed(rng, tgts[i], rng.choice([0.02, 0.3, 1.0])) for i in range(n)])
    tg = tgts if target_f64 else tgts.astype(np.float32)
    if k_kind == "shared":
        Ks = P.LINEMOD_K.copy()
    elif k_kind == "pascal":
        Ks = PASCAL_K.copy()
    else:
        Ks = np.repeat(P.LINEMOD_K[None], n, 0)
        Ks[:, 0, 0] *= rng.uniform(0.8, 1.2, n)
        Ks[:, 1, 1] *= rng.uniform(0.8, 1.2, n)
        Ks[:, 0, 1] = rng.uniform(-2, 2, n)
        Ks[:, :2, 2] += rng.uniform(-20, 20, (n, 2))
    err, ok, st = run_device(preds, tg, Ks, dm, ids)
    assert (st == 0).all()
    ev = E.Evaluator(models=models, diameters=diam)
    for i in range(n):
        c = names[ids[i]]
        K = Ks[i] if Ks.ndim == 3 else Ks
        want_err, want_ok = host_metrics(ev, preds[i], tg[i], c, K, False)
        check_errors(err[i], want_err, RTOL, f"image {i} class {c}")
        check_flags(ok[i], want_ok, want_err, diam[c])
    if k_kind == "shared":
        assert ok.any(axis=0).all() and (~ok).any(axis=0).all()   # both sides of every threshold occurred


def host_cloud(model, pose, K=None):
    """the float32 cloud the device search sees: the kernel's float64 expressions term by term (numpy's element-wise operations
    round like the device's uncontracted ones), rounded to float32; projected with z = 0 when K is given"""
    a = [model[:, 0] * pose[r, 0] + model[:, 1] * pose[r, 1] + model[:, 2] * pose[r, 2] + pose[r, 3] for r in range(3)]
    if K is None:
        return np.stack(a, 1).astype(np.float32)
    u = a[0] * K[0, 0] + a[1] * K[0, 1] + a[2] * K[0, 2]
    v = a[0] * K[1, 0] + a[1] * K[1, 1] + a[2] * K[1, 2]
    w = a[0] * K[2, 0] + a[1] * K[2, 1] + a[2] * K[2, 2]
    return np.stack([u / w, v / w], 1).astype(np.float32)


def workspace_indices(ws, n, searches, max_points):
    words = ws.view(torch.int64)[: n * searches * max_points].cpu().numpy().reshape(n, searches, max_points)
    none = np.int64(0x7F7FFFFFFFFFFFFF)
    return np.where(words == none, 0, words & 0xFFFFFFFF)


@pytest.mark.parametrize("sym_projection", [False, True])
def test_add_s_and_symmetric_projection_in_a_mixed_batch(sym_projection):
    rng = np.random.default_rng(41 + int(sym_projection))
    models = {"cat": model_cloud(rng, 1000), "eggbox": model_cloud(rng, 5000, dup=300), "glue": model_cloud(rng, 257, dup=40),
              "ape": model_cloud(rng, 7), "eggbox_small": None}
    models["eggbox_small"] = models["eggbox"][:1]
    diam = {c: 0.2 for c in models}
    dm = E.DeviceModels(models, diam, dev(), symmetric=("eggbox", "glue", "eggbox_small"))
    names = list(models)
    n = 20
    ids = np.array([1, 0, 2, 1, 3, 2, 4, 1, 0, 2, 1, 2, 3, 1, 2, 0, 1, 4, 2, 1])
    tgts = np.stack([random_pose(rng) for _ in range(n)])
    preds = np.stack([perturbed(rng, tgts[i], rng.choice([0.01, 0.2, 1.0])) for i in range(n)])
    K = P.LINEMOD_K
    S = 2 if sym_projection else 1
    ws = torch.empty(E.pose_metrics_workspace_bytes(n, dm, sym_projection), dtype=torch.uint8, device=dev())
    err, ok, st = run_device(preds, tgts, K, dm, ids, sym_projection, workspace=ws)
    assert (st == 0).all()
    idx = workspace_indices(ws, n, S, dm.max_points)
    ev = E.Evaluator(models=models, diameters=diam)
    for i in range(n):
        c = names[ids[i]]
        m = models[c]
        sym = c in ("eggbox", "glue", "eggbox_small")
        if c == "eggbox_small":   # not one of the host's SYMMETRIC_CLASSES: the host oracle is the nearest-neighbour error itself
            ev.models["eggbox"], saved = m, ev.models["eggbox"]
            want_err, want_ok = host_metrics(ev, preds[i], tgts[i], "eggbox", K, sym_projection)
            ev.models["eggbox"] = saved
        else:
            want_err, want_ok = host_metrics(ev, preds[i], tgts[i], c, K, sym_projection)
        tol = np.array([1e-7 if sym and sym_projection else RTOL, 1e-7 if sym else RTOL, RTOL, RTOL])
        check_errors(err[i], want_err, tol, f"image {i} {c}")
        check_flags(ok[i], want_ok, want_err, 0.2)
        if not sym:
            continue
        # the indices: pvnet_nn on the device's own float32 clouds (queries = target points, reference = predicted points)
        for s in range(S):
            Kc = K if s == 1 else None
            ref, que = host_cloud(m, preds[i], Kc), host_cloud(m, tgts[i], Kc)
            want_idx = E.find_nearest_point_idx(ref, que)
            np.testing.assert_array_equal(idx[i, s, : m.shape[0]], want_idx, err_msg=f"image {i} {c} search {s}")
            np.testing.assert_array_equal(idx[i, s, : m.shape[0]], nn_oracle.find_nearest_point_idx(ref, que),
                                          err_msg=f"image {i} {c} search {s} against the oracle")
            a, b = (m[want_idx] @ preds[i][:, :3].T + preds[i][:, 3]), (m @ tgts[i][:, :3].T + tgts[i][:, 3])
            if s == 1:
                a, b = P.project(m[want_idx], preds[i], K), P.project(m, tgts[i], K)
            np.testing.assert_allclose(err[i, 1 - s], np.mean(np.linalg.norm(a - b, axis=1)), rtol=1e-12)
        if c == "eggbox":
            # duplicated model points: a query whose nearest predicted point is a duplicated one gets its FIRST copy
            dup = idx[i, 0, :5000]
            assert not ((dup >= 2500) & (dup < 2800)).any()


def metrics_search_slice(n, searches, max_points):
    """pvnet_pose_metrics' plan of the search restated (it only names the path a batch takes): the slice length in points"""
    tiles = -(-max_points // NC.TILE)
    want = -(-1024 // (tiles * n * searches))
    return -(-tiles // max(1, min(want, tiles))) * NC.TILE


LATTICE_SIZES = (1, 256, 257, 513, 1100)
# proper rotations that map the lattice onto itself: the identity, a cyclic axis permutation, a half turn about z, and their product
LATTICE_ROTATIONS = [np.eye(3), np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), np.diag([-1.0, -1.0, 1.0]),
                     np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])]


def lattice_pose(rng):
    """a rotation of LATTICE_ROTATIONS and a translation in multiples of 0.25 that brings a mirrored axis back to 4096 + ...: the
    transformed cloud is exact in float64 and in float32, and its z stays positive"""
    R = LATTICE_ROTATIONS[rng.integers(len(LATTICE_ROTATIONS))]
    t = 0.25 * rng.integers(-4, 5, 3) + np.where(R.sum(axis=1) < 0, 8192.0 + 1.25, 0.0)
    assert (R[2] >= 0).all() and abs(np.linalg.det(R) - 1) < 1e-12
    return np.concatenate([R, t[:, None]], 1)


@pytest.mark.parametrize("n,sym_projection", [(3, False), (3, True), (40, False), (40, True), (120, False)])
def test_symmetric_classes_on_lattice_models(n, sym_projection):
    """models on a lattice under poses that keep them there: most queries have several predicted points at the minimal distance, in
    one tile, across tiles and across slices, and every tie must go to the first index -- oracle/nn_oracle.py on the host clouds is
    the judge of metrics_search_kernel.  The batch sizes put the search on one-tile slices (n = 3; n = 40 with one search) and on
    multi-tile slices (n = 40 with both searches: 512 points; n = 120: 768 points)."""
    S = 2 if sym_projection else 1
    assert metrics_search_slice(n, S, 1100) == {(3, 1): 256, (3, 2): 256, (40, 1): 256, (40, 2): 512, (120, 1): 768}[n, S]
    rng = np.random.default_rng(100 + n + int(sym_projection))
    names = [f"lattice{s}" for s in LATTICE_SIZES]
    models = {c: NC.clouds("lattice", 1, s, 1, 3, seed=5)[0][0] for c, s in zip(names, LATTICE_SIZES)}
    models["cat"] = model_cloud(rng, 300)   # the one class scored without a search, under ordinary poses
    classes = list(models)
    diam = {c: 0.2 for c in classes}
    dm = E.DeviceModels(models, diam, dev(), symmetric=names)
    ids = np.array([4, 5, 2]) if n == 3 else rng.permutation(np.arange(n) % len(classes))
    tgts = np.stack([lattice_pose(rng) for _ in range(n)])
    preds = np.stack([lattice_pose(rng) for _ in range(n)])
    for i in np.flatnonzero(ids == classes.index("cat")):
        tgts[i] = random_pose(rng)
        preds[i] = perturbed(rng, tgts[i], 0.3)
    K = P.LINEMOD_K
    ws = torch.empty(E.pose_metrics_workspace_bytes(n, dm, sym_projection), dtype=torch.uint8, device=dev())
    err, ok, st = run_device(preds, tgts, K, dm, ids, sym_projection, workspace=ws)
    assert (st == 0).all()
    idx = workspace_indices(ws, n, S, dm.max_points)
    tied = []
    for i in range(n):
        c = classes[ids[i]]
        m = models[c]
        tr, rot = P.cm_degree_error(preds[i], tgts[i])
        if c == "cat":
            want = np.array([E.projection_2d_error(preds[i], tgts[i], m, K), E.add_error(preds[i], tgts[i], m), tr, rot])
            check_errors(err[i], want, RTOL, f"image {i} {c}")
            continue
        want = np.array([E.projection_2d_error(preds[i], tgts[i], m, K), np.nan, tr, rot])
        for s in range(S):
            Kc = K if s == 1 else None
            ref, que = host_cloud(m, preds[i], Kc), host_cloud(m, tgts[i], Kc)
            if s == 0:   # the poses keep the lattice: the float32 clouds are the float64 ones
                assert (ref == m @ preds[i][:, :3].T + preds[i][:, 3]).all() and (que[:, 2] > 0).all()
            if s == 0 and m.shape[0] >= 513:   # several points per lattice site
                d = ((ref[None].astype(np.float64) - que[:, None]) ** 2).sum(-1)
                tied.append(((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).mean())
            want_idx = nn_oracle.find_nearest_point_idx(ref, que)
            np.testing.assert_array_equal(idx[i, s, : m.shape[0]], want_idx, err_msg=f"image {i} {c} search {s}")
            if s == 0:
                a, b = m[want_idx] @ preds[i][:, :3].T + preds[i][:, 3], m @ tgts[i][:, :3].T + tgts[i][:, 3]
            else:
                a, b = P.project(m[want_idx], preds[i], K), P.project(m, tgts[i], K)
            want[1 - s] = np.mean(np.linalg.norm(a - b, axis=1))
        check_errors(err[i], want, RTOL, f"image {i} {c}")
    assert np.min(tied) > 0.5   # the clouds do what they are for: most minima are tied


def test_failed_poses_and_bad_class_ids():
    rng = np.random.default_rng(5)
    models = {"cat": model_cloud(rng, 300), "glue": model_cloud(rng, 300)}
    diam = {"cat": 0.2, "glue": 0.2}
    dm = E.DeviceModels(models, diam, dev())
    n = 8
    tgts = np.stack([random_pose(rng) for _ in range(n)])
    preds = np.stack([perturbed(rng, tgts[i], 0.2) for i in range(n)])
    preds[[1, 2, 5]] = 0.0                 # POSE_FAILED: the solve returns zeros
    ids = np.array([0, 0, 1, 0, 5, 1, -1, 2])
    for sp in (False, True):
        err, ok, st = run_device(preds, tgts, P.LINEMOD_K, dm, ids, sp)
        assert st.tolist() == [0, 0, 0, 0, -1, 0, -1, -1]
        assert np.isnan(err[[4, 6, 7]]).all() and not ok[[4, 6, 7]].any()
        ev = E.Evaluator(models=models, diameters=diam)
        for i in (0, 1, 2, 3, 5):
            c = ["cat", "glue"][ids[i]]
            with np.errstate(invalid="ignore"):   # the host's 0 / 0 of a zero pose's projection
                want_err, want_ok = host_metrics(ev, preds[i], tgts[i], c, P.LINEMOD_K, sp)
            check_errors(err[i], want_err, 1e-7, f"image {i}", equal_nan=True)
            assert (ok[i] == want_ok).all()
        assert np.isnan(err[1, 0]) and not ok[1, 0]   # a zero pose projects to 0 / 0


def test_bitwise_reproducible_on_a_garbage_workspace():
    rng = np.random.default_rng(9)
    models = {"cat": model_cloud(rng, 3000), "eggbox": model_cloud(rng, 4000)}
    diam = {"cat": 0.2, "eggbox": 0.2}
    dm = E.DeviceModels(models, diam, dev())
    n = 16
    tgts = np.stack([random_pose(rng) for _ in range(n)])
    preds = np.stack([perturbed(rng, tgts[i], 0.5) for i in range(n)])
    ids = np.arange(n) % 2
    nbytes = E.pose_metrics_workspace_bytes(n, dm, True)
    outs = []
    for seed in (1, 2):
        g = torch.Generator(device=dev()).manual_seed(seed)
        ws = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev(), generator=g)
        outs.append(run_device(preds, tgts, P.LINEMOD_K, dm, ids, True, workspace=ws))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert np.isfinite(outs[0][0]).all()


def _batch_case(demo_fixture, n, seed):
    f = demo_fixture
    rng = np.random.default_rng(seed)
    X, K, gt = f["points_3d"].astype(np.float64), f["K"].astype(np.float64), f["pose"].astype(np.float64)
    lo, hi = f["bb8_3d"].min(0), f["bb8_3d"].max(0)
    model = rng.uniform(lo, hi, (2000, 3))
    diameter = float(np.linalg.norm(hi - lo))
    kp = f["points_2d"][None].astype(np.float64) + rng.normal(size=(n,) + f["points_2d"].shape) * rng.uniform(0.2, 6.0, (n, 1, 1))
    tgts = np.repeat(gt[None], n, 0).astype(np.float32)
    ev = lambda: E.Evaluator(models={"cat": model, "glue": model}, diameters={"cat": diameter, "glue": diameter},  # noqa: E731
                             points_3d={"cat": X, "glue": X})
    return ev, kp, tgts, K


def _compare_recorders(a, b):
    for name in ("projection_2d_recorder", "add_recorder", "cm_degree_5_recorder"):
        assert getattr(a, name) == getattr(b, name), name
    np.testing.assert_allclose(a.add_dists, b.add_dists, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(a.proj_mean_diffs, b.proj_mean_diffs, rtol=1e-6, atol=1e-4)
    assert a.average_precision(verbose=False) == b.average_precision(verbose=False)


@pytest.mark.parametrize("cls", ["cat", "glue"])
def test_evaluate_batch_equals_a_loop_of_evaluate(demo_fixture, cls):
    ev_make, kp, tgts, K = _batch_case(demo_fixture, 32, 17)
    devi = ev_make()
    kd = torch.from_numpy(kp.astype(np.float32)).to(dev())
    # the host sees the float32 key-points the device reads
    host32 = ev_make()
    want = np.stack([host32.evaluate(kp[i].astype(np.float32), tgts[i], cls, intri_type="use_intrinsic", intri_matrix=K)
                     for i in range(32)])
    poses = devi.evaluate_batch(kd, tgts, cls, intri_type="use_intrinsic", intri_matrix=K)
    assert poses.is_cuda
    np.testing.assert_allclose(poses.cpu().numpy(), want, rtol=0, atol=1e-8)
    _compare_recorders(devi, host32)
    assert 0 < np.mean(devi.add_recorder) < 1 or 0 < np.mean(devi.projection_2d_recorder) < 1
    # per-image K ('use_intrinsic' with [n,3,3]) gives the same as the shared one
    per = ev_make()
    per.evaluate_batch(kd, tgts, cls, intri_type="use_intrinsic", intri_matrix=np.repeat(K[None], 32, 0))
    assert per.add_dists == devi.add_dists and per.proj_mean_diffs == devi.proj_mean_diffs


def test_evaluate_batch_with_covariance_equals_evaluate_uncertainty(demo_fixture):
    ev_make, kp, tgts, K = _batch_case(demo_fixture, 32, 23)
    rng = np.random.default_rng(4)
    A = rng.normal(size=(32, kp.shape[1], 2, 2)) * 0.5
    cov = (A @ np.swapaxes(A, -1, -2) + rng.uniform(0.5, 2.0, (32, kp.shape[1], 1, 1)) * np.eye(2)).astype(np.float32)
    kp32 = kp.astype(np.float32)
    host, devi = ev_make(), ev_make()
    want = np.stack([host.evaluate_uncertainty(kp32[i], cov[i], tgts[i], "cat", intri_type="use_intrinsic", intri_matrix=K)
                     for i in range(32)])
    poses = devi.evaluate_batch(torch.from_numpy(kp32).to(dev()), tgts, "cat", intri_type="use_intrinsic", intri_matrix=K,
                                covariance=torch.from_numpy(cov).to(dev()))
    # the weighted solve's agreement with the host on random covariances: measured up to 1.3e-8 on less benign ones
    np.testing.assert_allclose(poses.cpu().numpy(), want, rtol=0, atol=5e-8)
    _compare_recorders(devi, host)


def test_graph_capture_of_voting_pose_and_metrics_is_bitwise_eager():
    mask, planar, _ = synth.make_batch(4, first_index=700, h=96, w=128, radius=14, noise=True)
    d = dev()
    m = torch.from_numpy(np.ascontiguousarray(mask)).to(d)
    v = synth.planar_to_vertex_view(torch.from_numpy(planar).to(d))
    vn = v.shape[3]
    rng = np.random.default_rng(1)
    X = rng.uniform(-0.08, 0.08, size=(vn, 3))
    models = E.DeviceModels({"cat": model_cloud(rng, 700), "glue": model_cloud(rng, 900)}, {"cat": 0.2, "glue": 0.2}, d)
    ids = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device=d)
    tgts = torch.from_numpy(np.stack([random_pose(rng) for _ in range(4)])).to(d)
    Xd, Kd = torch.from_numpy(X).to(d), torch.from_numpy(P.LINEMOD_K.copy()).to(d)
    L = voting.vote_layout(4, 96, 128, vn, 64, 30000)
    ws = torch.empty(L.total_bytes, dtype=torch.uint8, device=d)
    mws = torch.empty(E.pose_metrics_workspace_bytes(4, models, True), dtype=torch.uint8, device=d)
    kp = torch.zeros((4, vn, 2), device=d)
    poses = torch.zeros((4, 3, 4), dtype=torch.float64, device=d)
    status = torch.zeros((4,), dtype=torch.int32, device=d)
    errors = torch.zeros((4, 4), dtype=torch.float64, device=d)
    passed = torch.zeros((4, 3), dtype=torch.bool, device=d)
    mstatus = torch.zeros((4,), dtype=torch.int32, device=d)

    def enqueue():
        voting.ransac_voting_layer_v3(m, v, 64, inlier_thresh=0.99, seed=21, out=kp, workspace=ws)
        P.pnp_batch_device(Xd, kp, Kd, out=(poses, status))
        E.pose_metrics_device(poses, tgts, Kd, models, class_ids=ids, sym_projection=True, out=(errors, passed, mstatus),
                              workspace=mws)

    eager = []
    for _ in range(2):
        enqueue()
        torch.cuda.synchronize()
        eager.append((poses.clone(), errors.clone(), passed.clone(), mstatus.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*eager))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    poses.zero_()
    errors.fill_(-1.0)
    passed.fill_(True)
    mstatus.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(poses, eager[0][0]) and torch.equal(errors, eager[0][1])
    assert torch.equal(passed, eager[0][2]) and torch.equal(mstatus, eager[0][3])
    assert (mstatus == 0).all() and torch.isfinite(errors).all()
