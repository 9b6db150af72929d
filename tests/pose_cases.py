"""Problems, oracles and bars shared by the pose-solve tests (tests/test_pose_device.py, tests/test_pose_sweep_cpu.py,
tests/test_pose_sweep_device.py).  A plain module: it imports neither torch nor a GPU.

The oracle of the device solve (pvnet_pose_solve, pvnet_amd/csrc/pose_solve.hip) is the host library (pvnet_pnp_solve,
pvnet_amd/csrc/pvnet_pnp.cpp) on the same float64 inputs."""
import numpy as np

from pvnet_amd import evaluation as E
from pvnet_amd import pnp as P

# key-point counts of the sweep: both ends of the documented range (6 .. PVNET_POSE_MAX_PN = 64), the project's own 9, and both
# sides of 27 lanes (the normal-equation split), of 32 lanes and of the full wave
SWEEP_PN = (6, 7, 8, 9, 10, 16, 31, 32, 33, 63, 64)
SWEEP_N = 32

# Bars of the sweep, device against host: every [R|t] entry within BAR_POSE, and the device pose's cost on the host at most
# (1 + BAR_COST) times the host's final cost.  They are not chosen from what the device gives: tests/test_pose_sweep_cpu.py
# measures how far the host solver moves when its own input moves by one unit in the last place (its docstring has the numbers),
# asserts that this spread is at least 20x (pose) and 50x (cost) below the bars, and that a dropped or misread key-point moves
# every pose by more than 100 * BAR_POSE.
BAR_POSE = 1e-7
BAR_COST = 1e-11

LIMIT = 200   # LM iterations per stage (pvnet_pnp_solve; pnp_batch_device's default max_iterations)


def problems(n, seed=11, pn=9, noise=0.4):
    """random problems built like tests/test_pnp.py: rotations up to 2.8 rad, ``noise`` px of Gaussian noise"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.08, 0.08, size=(pn, 3))
    x2, poses = [], []
    for _ in range(n):
        r = rng.normal(size=3)
        r *= rng.uniform(0.1, 2.8) / np.linalg.norm(r)
        pose = np.concatenate([P.rodrigues(r), np.array([[rng.uniform(-0.2, 0.2)], [rng.uniform(-0.2, 0.2)],
                                                         [rng.uniform(0.5, 1.5)]])], 1)
        poses.append(pose)
        x2.append(P.project(X, pose, P.LINEMOD_K) + rng.normal(size=(pn, 2)) * noise)
    return X, np.stack(x2), np.stack(poses)


def sweep_case(pn):
    """(X [pn,3], x2 [32,pn,2], W [32,pn,3] explicit weights, cov [32,pn,2,2] float32 covariances) of one key-point count"""
    X, x2, _ = problems(SWEEP_N, 100 + pn, pn)
    rng = np.random.default_rng(4)
    W = np.abs(rng.normal(1.0, 0.3, size=(SWEEP_N, pn, 3)))
    W[:, :, 1] *= 0.1
    rng = np.random.default_rng(5)
    A = 0.5 * rng.normal(size=(SWEEP_N, pn, 2, 2))
    c = rng.uniform(0.5, 2.0, size=(SWEEP_N, pn))
    cov = A @ A.transpose(0, 1, 3, 2) + c[..., None, None] * np.eye(2)
    cov[..., 0, 1] = cov[..., 1, 0]
    return X, x2, W, cov.astype(np.float32)


def host_solve(X, x2, K, W=None):
    """pvnet_pnp_solve image by image: (poses [n,3,4] as pnp_batch gives them, status [n] = its return values, rt [n,6] =
    angle-axis | translation, zeros where the solve failed)"""
    lib = P.load_pnp_library()
    n = x2.shape[0]
    rt = np.zeros((n, 6))
    status = np.zeros(n, np.int32)
    X = np.ascontiguousarray(X, np.float64)
    for i in range(n):
        Ki = np.ascontiguousarray(K[i] if K.ndim == 3 else K, np.float64)
        xi = np.ascontiguousarray(x2[i], np.float64)
        Wi = None if W is None else np.ascontiguousarray(W[i], np.float64)
        out = np.zeros(6)
        status[i] = lib.pvnet_pnp_solve(P._dptr(xi), P._dptr(X), None if Wi is None else P._dptr(Wi), P._dptr(Ki),
                                        P._dptr(out), X.shape[0])
        if status[i] >= 0:
            rt[i] = out
    poses = np.empty((n, 3, 4))
    lib.pvnet_pnp_poses_from_rt(P._dptr(rt), P._dptr(poses), n)
    return poses, status, rt


def host_cost(X, x2, W, K, rt):
    """0.5 |r|^2 of every image at its pose ``rt`` [n,6], the residuals from pvnet_pnp_evaluate (the solver's own cost)"""
    K = np.asarray(K, np.float64)
    return np.array([0.5 * np.sum(P.cost_function(x2[i], X, None if W is None else W[i], K[i] if K.ndim == 3 else K, rt[i],
                                                  jacobian=False) ** 2) for i in range(x2.shape[0])])


def poses_to_rt(poses):
    """[n,3,4] (R | t) -> [n,6] through the host's pvnet_matrix_to_angle_axis"""
    lib = P.load_pnp_library()
    rt = np.empty((poses.shape[0], 6))
    for i, pose in enumerate(np.asarray(poses, np.float64)):
        R, aa = np.ascontiguousarray(pose[:, :3]), np.empty(3)
        lib.pvnet_matrix_to_angle_axis(P._dptr(R), P._dptr(aa))
        rt[i, :3], rt[i, 3:] = aa, pose[:, 3]
    return rt


def covariance_weights(cov):
    """[n,pn,2,2] covariances -> [n,pn,3] weights (wxx, wxy, wyy), formed as Evaluator.evaluate_uncertainty forms them
    (pvnet_amd/evaluation.py): the inverse matrix square root through numpy's eigh, zero below cov[0,0] < 1e-6 or with a NaN"""
    cov = np.asarray(cov, np.float64)
    out = np.zeros(cov.shape[:2] + (3,))
    for i in range(cov.shape[0]):
        for k in range(cov.shape[1]):
            if cov[i, k, 0, 0] < 1e-6 or np.isnan(cov[i, k]).any():
                continue
            w, v = np.linalg.eigh(cov[i, k])
            m = (v / np.sqrt(np.maximum(w, 1e-30))) @ v.T
            out[i, k] = m[0, 0], m[0, 1], m[1, 1]
    return out


def evaluator_solve(X, x2, cov, K):
    """Evaluator.evaluate_uncertainty image by image -> poses [n,3,4]: the oracle of ``pnp_batch_device(covariance=...)``"""
    ev = E.Evaluator(models={"cat": X}, diameters={"cat": 0.1}, points_3d={"cat": X})
    return np.stack([ev.evaluate_uncertainty(x2[i], cov[i], np.eye(4)[:3], "cat", intri_type="use_intrinsic", intri_matrix=K)
                     for i in range(x2.shape[0])])


# 3 px of noise: some images have no optimum to agree on -- the unweighted LM wanders along a flat valley until
# it reaches its iteration limit
ILL_PN = (7, 8, 10)
ILL_N = 64


def ill_posed_case(pn):
    """(X, x2 [64,pn,2] at 3 px noise)"""
    X, x2, _ = problems(ILL_N, 100 + pn, pn, noise=3.0)
    return X, x2
