"""Problems shared by the tests of the pose solve per class (tests/test_pose_classes_cpu.py, tests/test_pose_classes_device.py;
pvnet_pose_solve_classes of include/pvnet_poses.h, pnp.pnp_classes_device), built on tests/pose_cases.py.  A plain module: it imports
neither torch nor a GPU.

An item (i, k) is image i, class k + 1.  Every class has object points of its own, CLEARLY different from the others': other extents
along every axis and another shape (not one set permuted, scaled or mirrored), so that a solver which takes the wrong class's points
for an item cannot reach that item's pose.  tests/test_pose_classes_cpu.py shows this on the host, for the two mistakes a kernel
can make with the table: class 0's points for every item, and the table indexed by the image."""
import numpy as np

from pvnet_amd import pnp as P
from tests import pose_cases

# (b, nk, pn) of the device tests: the project's own 9 points; the fewest points the linear start takes, more images than classes;
# a full wave of points; the 13 classes of the "fuse" label images with a single image
LAYOUTS = ((2, 3, 9), (3, 2, 6), (2, 2, 64), (1, 13, 8))
NOISE = 0.4   # px: pose_cases.problems' own


def class_points(nk, pn, seed=5):
    """[nk,pn,3]: class k fills a box of its own extents (between 4 and 16 cm, the three axes in another proportion for every class)
    with points of its own draw, pushed outwards by a class-dependent power so that the sets differ in shape, not only in scale"""
    out = np.empty((nk, pn, 3))
    for k in range(nk):
        rng = np.random.default_rng(seed + 101 * k)
        u = rng.uniform(-1.0, 1.0, size=(pn, 3))
        u = np.sign(u) * np.abs(u) ** (0.5 + 0.25 * (k % 5))
        extent = 0.04 + 0.12 * np.array([((3 * k + 1) % 7) / 6.0, ((5 * k + 2) % 7) / 6.0, ((2 * k + 4) % 7) / 6.0])
        out[k] = u * extent
    return out


def random_pose(rng):
    """pose_cases.problems' poses: a rotation of 0.1 .. 2.8 rad about a random axis, the object 0.5 .. 1.5 m in front of the camera"""
    r = rng.normal(size=3)
    r *= rng.uniform(0.1, 2.8) / np.linalg.norm(r)
    t = np.array([[rng.uniform(-0.2, 0.2)], [rng.uniform(-0.2, 0.2)], [rng.uniform(0.5, 1.5)]])
    return np.concatenate([P.rodrigues(r), t], 1)


def case(b, nk, pn, seed=11, noise=0.0, K=P.LINEMOD_K):
    """(X [nk,pn,3], x2 [b,nk,pn,2] float64, poses [b,nk,3,4]): the ground-truth pose of every item and its points' projections,
    exact (noise = 0) or with ``noise`` px of Gaussian noise (NOISE is pose_cases.problems').  K [3,3] or [b,3,3]"""
    rng = np.random.default_rng(seed)
    X = class_points(nk, pn)
    K = np.asarray(K, np.float64)
    poses = np.stack([np.stack([random_pose(rng) for _ in range(nk)]) for _ in range(b)])
    x2 = np.stack([np.stack([P.project(X[k], poses[i, k], K[i] if K.ndim == 3 else K) for k in range(nk)]) for i in range(b)])
    assert (np.einsum("bkij,kpj->bkpi", poses[..., :3], X)[..., 2] + poses[:, :, None, 2, 3] > 0.2).all()   # in front of the camera
    if noise:
        x2 = x2 + rng.normal(size=x2.shape) * noise
    return X, x2, poses


def cameras(b, seed=2):
    """[b,3,3]: LINEMOD's camera with focal lengths within 10 % and the principal point within 5 px of it, one per image"""
    rng = np.random.default_rng(seed)
    Ks = np.repeat(P.LINEMOD_K[None], b, 0)
    Ks[:, 0, 0] *= rng.uniform(0.9, 1.1, b)
    Ks[:, 1, 1] *= rng.uniform(0.9, 1.1, b)
    Ks[:, :2, 2] += rng.uniform(-5, 5, (b, 2))
    return Ks


def weights(b, nk, pn, seed=4):
    """explicit weights [b,nk,pn,3] as pose_cases.sweep_case draws them"""
    W = np.abs(np.random.default_rng(seed).normal(1.0, 0.3, size=(b, nk, pn, 3)))
    W[..., 1] *= 0.1
    return W


def covariances(b, nk, pn, seed=5):
    """float32 covariances [b,nk,pn,2,2] as pose_cases.sweep_case draws them, with the two hand-made ones that get a zero weight: one
    with cov[0,0] below 1e-6 (item (0, 0), point 1) and one with a NaN entry (the last item, point 3)"""
    rng = np.random.default_rng(seed)
    A = 0.5 * rng.normal(size=(b, nk, pn, 2, 2))
    c = rng.uniform(0.5, 2.0, size=(b, nk, pn))
    cov = A @ np.swapaxes(A, -1, -2) + c[..., None, None] * np.eye(2)
    cov[..., 0, 1] = cov[..., 1, 0]
    cov[0, 0, 1] = [[1e-7, 0.0], [0.0, 3.0]]
    cov[-1, -1, 3] = [[2.0, np.nan], [np.nan, 1.0]]
    return cov.astype(np.float32)


def host_loop(X, x2, K, W=None, points=None):
    """the host library class by class: (poses [b,nk,3,4], status [b,nk]) of pose_cases.host_solve on x2[:, k] with X[k] -- or, with
    ``points(i, k)``, with the object points that function names for item (i, k): the planted mistakes of the CPU test"""
    b, nk = x2.shape[:2]
    poses, status = np.empty((b, nk, 3, 4)), np.empty((b, nk), np.int32)
    K = np.asarray(K, np.float64)
    for k in range(nk):
        if points is None:
            poses[:, k], status[:, k], _ = pose_cases.host_solve(X[k], x2[:, k], K, None if W is None else W[:, k])
        else:
            for i in range(b):
                p, s, _ = pose_cases.host_solve(points(i, k), x2[i:i + 1, k], K[i] if K.ndim == 3 else K,
                                                None if W is None else W[i:i + 1, k])
                poses[i, k], status[i, k] = p[0], s[0]
    return poses, status


def reprojection_cost(X, x2, K, poses):
    """0.5 |r|^2 of every item at ``poses`` [b,nk,3,4] with ITS OWN class's points: [b,nk]"""
    K = np.asarray(K, np.float64)
    b, nk = x2.shape[:2]
    return np.array([[0.5 * np.sum((P.project(X[k], poses[i, k], K[i] if K.ndim == 3 else K) - x2[i, k]) ** 2) for k in range(nk)]
                     for i in range(b)])
